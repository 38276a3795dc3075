"""GPU: mixed-adapter LoRA decode - an adapter id per row. The shrink ``t[m] = x[m] @ lora_A[ids[m]]^T`` (bitsandbytes_amd::lora_shrink_ids,
csrc/lora_shrink.hip's ids kernel, ``bitsandbytes_amd.lora_shrink_ids``) and, in the second half of the file, the expand epilogue
(bitsandbytes_amd::gemm_4bit_lora_ids, csrc/gemv4_stream.hip kLoraIds, csrc/gemm4_mfma_sm.hip IDS, ``matmul_4bit_lora_ids``,
``nn.Linear4bitMultiLoRA``).

* bit-identity with the uniform launch, per row: for each distinct id the existing kernel / op runs with that adapter at the same M,
  and the rows that carry the id are ``torch.equal`` (ordinary data: sums that round);
* rows without an adapter: zeros (shrink), the plain gemm_4bit row (expand); adapters that no row names do not exist (NaN in them -
  and in the lora_t rows of rows without an adapter - changes no bit); every element of a NaN-filled output is written;
* exact: on the operands of tests/lora_multi_cases.py the output is float64 rounded once with each row's adapter;
* the ids live on the device: one captured graph follows ids overwritten in place;
* ordinary data against float64 inside the derived tolerances; the compositions above 16 rows; opcheck.
The shrink kernel is driven through the C entry point (which does not consult the predicate) and, wherever the predicate answers 1,
through the op as well - with equal bits. No case is skipped: the cells of lora_cases.MUST_SERVE and lora_multi_cases.CASES must be
served (asserted); only where the predicate answers 0 (2002 x 1024 at 5 ... 8 rows) the raw op must raise and the function compose.
"""
import ctypes as ct
import functools

import pytest
import torch

import exact_inputs as X
import lora_cases as LC
import lora_multi_cases as C
import lora_shrink_cases as SC
from routed_sweep import gpu_ops

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _bnb():
    import bitsandbytes_amd as bnb

    return bnb


def _op():
    return torch.ops.bitsandbytes_amd.lora_shrink_ids.default


def _supported(dtype, M, A_n, R, K) -> bool:
    return _bnb().lib.bnb_mi355x_lora_shrink_ids_supported(C.DT_CODE[dtype], M, A_n, R, K) == 1


def _table(splits):
    n = 0 if splits is None else len(splits)
    return ((ct.c_int * n)(*splits) if n else None), n


def _entry(x, stack, ids, out, splits=None):
    """bnb_mi355x_lora_shrink_ids on x [M, K], stack [A_n, R, K], ids [M] into the M * R elements at ``out``."""
    M, K = x.shape
    table, n = _table(splits)
    _bnb().lib.bnb_mi355x_lora_shrink_ids(C.DT_CODE[x.dtype], x.data_ptr(), stack.data_ptr(), ids.data_ptr(), ids.element_size(), out.data_ptr(), M,
                                          stack.shape[0], stack.shape[1], K, table, n, torch.cuda.current_stream().cuda_stream)


def _uniform(x, a, splits=None):
    """The flat [M * R] output of the existing uniform launch (bnb_mi355x_lora_shrink) with ONE adapter."""
    M, K = x.shape
    flat = torch.empty(M * a.shape[0], dtype=x.dtype, device=DEV)
    table, n = _table(splits)
    _bnb().lib.bnb_mi355x_lora_shrink(C.DT_CODE[x.dtype], x.data_ptr(), a.data_ptr(), flat.data_ptr(), M, a.shape[0], K, table, n,
                                      torch.cuda.current_stream().cuda_stream)
    return flat


def _ids(vals, dtype):
    return torch.tensor(vals, dtype=dtype, device=DEV)


def _shrink(x, stack, ids, splits=None, must_serve=True):
    """The flat [M * R] output of the ids kernel, written into a NaN-filled buffer; where the predicate serves the shape, the op's as
    well (asserted equal). ``must_serve``: the predicate has to answer 1 (the coverage guard: no case is skipped)."""
    M, (A_n, R, K) = x.shape[0], stack.shape
    flat = torch.full((M * R,), float("nan"), dtype=x.dtype, device=DEV)
    _entry(x, stack, ids, flat, splits)
    served = _supported(x.dtype, M, A_n, R, K)
    assert served or not must_serve, f"the predicate refuses M={M}, A_n={A_n}, R={R}, K={K}, {x.dtype}"
    if served:
        assert torch.equal(_op()(x, stack, ids, None if splits is None else list(splits)).view(-1).view(torch.int16), flat.view(torch.int16))
    return flat


def _rows(flat, M, R, splits):
    """[M, R] with the parts of a splits call side by side."""
    if splits is None:
        return flat.view(M, R)
    return torch.cat(SC.parts_of(flat, M, splits), dim=1)


# ------------------------------------------------------------------------------------------ exact
@functools.lru_cache(maxsize=None)
def _prepared(case):
    """The case's operands on the host and on the device, computed once and never written to."""
    x, stack = C.build(case)
    return x, stack, x.to(DEV), stack.to(DEV)


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.name)
def test_exact_with_each_rows_adapter(case):
    x, stack, xd, sd = _prepared(case)
    failures = []
    for M in C.MS:
        for name, vals, idt in C.patterns(M, case.A_n):
            got = _rows(_shrink(xd[:M], sd, _ids(vals, idt), case.splits), M, case.R, case.splits).cpu()
            want = C.reference(x[:M], stack, vals)
            if not torch.equal(got.view(torch.int16), want.view(torch.int16)):   # (bits: a row without an adapter is +0)
                failures.append((M, name, X.first_mismatch(got, want)))
    assert not failures, failures[:5]


# ------------------------------------------------------------------------------------------ bit-identity, no-adapter rows, poison
@pytest.mark.parametrize("dtype", C.DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("K,A_n,R,splits", [(64, 17, 24, None), (2048, 3, 48, (16, 16, 16)), (4096, 17, 128, None), (4096, 64, 8, None),
                                             (8192, 3, 160, (8, 128, 24)), (2752, 1, 24, None)])
def test_rows_equal_the_uniform_launch(K, A_n, R, splits, dtype):
    """Ordinary data. A row with an adapter has the bits of the uniform launch with that adapter at the same M; a row without one is
    zeros; NaN in every adapter that no row names changes no bit of the output."""
    x, stack = C.ordinary(C.MAX_ROWS, A_n, R, K, dtype, K + A_n)
    xd, sd = x.to(DEV), stack.to(DEV)
    for M in C.MS:
        alone = {}
        for name, vals, idt in C.patterns(M, A_n):
            ids = _ids(vals, idt)
            got = _rows(_shrink(xd[:M], sd, ids, splits, must_serve=K <= 4096), M, R, splits)
            assert not bool(torch.isnan(got).any()), (M, name)
            used = sorted({i for i in vals if 0 <= i < A_n})
            for a in used:
                if a not in alone:
                    alone[a] = _rows(_uniform(xd[:M], sd[a], splits), M, R, splits)
                    assert not torch.equal(alone[a], torch.zeros_like(alone[a]))
            for m, i in enumerate(vals):
                if 0 <= i < A_n:
                    assert torch.equal(got[m], alone[i][m]), (M, name, m, i)
                else:
                    assert torch.equal(got[m].view(torch.int16), torch.zeros(R, dtype=torch.int16, device=DEV)), (M, name, m, i)
            poisoned = sd.clone()
            for a in range(A_n):
                if a not in used:
                    poisoned[a] = float("nan")
            again = _rows(_shrink(xd[:M], poisoned, ids, splits, must_serve=K <= 4096), M, R, splits)
            assert torch.equal(again.view(torch.int16), got.view(torch.int16)), (M, name)


def test_c_entry_point_writes_its_part_only():
    """t inside a larger NaN-filled buffer: the part is fully written whatever the ids, everything outside it is still NaN."""
    pad = 64
    for dtype in C.DTYPES:
        for A_n, R, K, splits in ((3, 24, 2048, None), (17, 160, 64, (8, 128, 24))):
            x, stack = C.ordinary(C.MAX_ROWS, A_n, R, K, dtype, 17)
            xd, sd = x.to(DEV), stack.to(DEV)
            for M in (1, 3, 16):
                for name, vals, idt in C.patterns(M, A_n):
                    big = torch.full((pad + M * R + pad,), float("nan"), dtype=dtype, device=DEV)
                    inner = big[pad:pad + M * R]
                    assert inner.data_ptr() % 16 == 0
                    _entry(xd[:M], sd, _ids(vals, idt), inner, splits)
                    torch.cuda.synchronize()
                    assert not bool(torch.isnan(inner).any()), (dtype, A_n, M, name)
                    assert bool(torch.isnan(big[:pad]).all()) and bool(torch.isnan(big[pad + M * R:]).all()), (dtype, A_n, M, name)


# ------------------------------------------------------------------------------------------ ordinary data against float64
@pytest.mark.parametrize("dtype", C.DTYPES, ids=["bf16", "fp16"])
def test_ordinary_data_against_float64(dtype):
    """Through the public function, leading dims included: inside lora_shrink_cases.tolerance around the float64 product with the
    row's adapter - at 17 rows too, where the function composes. Every figure is printed."""
    bnb = _bnb()
    K, R, A_n = 4096, 24, 17
    x, stack = C.ordinary(18, A_n, R, K, dtype, 23)
    xd, sd = x.to(DEV), stack.to(DEV)
    with torch.no_grad():
        for lead in ((1,), (2, 4), (16,), (17,)):
            M = lead[0] if len(lead) == 1 else lead[0] * lead[1]
            vals = [(5 * m + 3) % (A_n + 2) - 1 for m in range(M)]            # -1 ... A_n
            got = bnb.lora_shrink_ids(xd[:M].view(*lead, K), sd, _ids(vals, torch.int64).view(*lead))
            assert got.shape == (*lead, R) and got.dtype == dtype
            got = got.view(M, R).cpu()
            if M <= 16:
                assert torch.equal(got, _shrink(xd[:M], sd, _ids(vals, torch.int32)).view(M, R).cpu())
            worst = 0.0
            for m, i in enumerate(vals):
                if 0 <= i < A_n:
                    want = x[m:m + 1].double() @ stack[i].double().t()
                    worst = max(worst, float(((got[m:m + 1].double() - want).abs() / SC.tolerance(want, x[m:m + 1], stack[i])).max()))
                else:
                    assert torch.equal(got[m], torch.zeros(R, dtype=dtype)), (lead, m)
            print(f"{dtype} lead={lead}: worst error / bound {worst:.3f}")
            assert worst <= 1.0, (dtype, lead, worst)


# ------------------------------------------------------------------------------------------ the ids live on the device
@pytest.mark.parametrize("M", [1, 4, 16, 17])
def test_captured_graph_follows_the_ids(M):
    """One torch.cuda.graph of lora_shrink_ids - the kernel up to 16 rows, the composition at 17 -, replayed with new ids written into
    the same buffer: the host read nothing, and each replay matches its own ids."""
    bnb = _bnb()
    K, R, A_n, dtype = 2048, 24, 17, torch.bfloat16
    x, stack = C.ordinary(M, A_n, R, K, dtype, 41)
    xd, sd = x.to(DEV), stack.to(DEV)
    sets = [[(3 * m + k) % (A_n + 2) - 1 for m in range(M)] for k in (0, 5, 11)]
    with torch.no_grad():
        eager = [bnb.lora_shrink_ids(xd, sd, _ids(v, torch.int64)) for v in sets]
        assert not torch.equal(eager[1], eager[2])
        buf = _ids(sets[0], torch.int64)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                bnb.lora_shrink_ids(xd, sd, buf)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            t = bnb.lora_shrink_ids(xd, sd, buf)
        for k in (1, 2):
            buf.copy_(_ids(sets[k], torch.int64))
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(t, eager[k]), f"replay {k} did not follow the ids"


# ------------------------------------------------------------------------------------------ opcheck
def test_opcheck():
    K, r, A_n = 2048, 16, 5
    a = (torch.randn(A_n, 3 * r, K, device=DEV) / K ** 0.5).bfloat16()
    assert _supported(torch.bfloat16, 4, A_n, 3 * r, K)
    for lead in ((1,), (3,), (2, 2)):
        x = torch.randn(*lead, K, device=DEV).bfloat16()
        for idt in (torch.int32, torch.int64):
            ids = torch.randint(-1, A_n + 1, lead, device=DEV, dtype=idt)
            for kwargs in ({}, dict(splits=[r, r, r]), dict(splits=[3 * r])):
                torch.library.opcheck(_op(), (x, a, ids), kwargs, test_utils=("test_schema", "test_faketensor"))
    assert _op()(x[:0], a, ids[:0]).shape == (0, 2, 3 * r) and _op()(x[:0], a, ids[:0], [r, 2 * r]).shape == (0,)
    # what the fake kernel cannot see: a call without a kernel is an error, never another path
    with pytest.raises(ValueError, match="no kernel"):
        _op()(torch.randn(17, K, device=DEV).bfloat16(), a, torch.zeros(17, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="no kernel"):
        _op()(torch.randn(1, K, device=DEV), a.float(), torch.zeros(1, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="no kernel"):
        _op()(x, a, ids, [r + 4, 2 * r - 4])


# ========================================================================================== expand: gemm_4bit_lora_ids
# The mixed-adapter epilogue of the streaming kernel (kLoraIds) and of the streaming MFMA kernel (IDS), matmul_4bit_lora_ids and
# nn.Linear4bitMultiLoRA.


def _eop():
    return torch.ops.bitsandbytes_amd.gemm_4bit_lora_ids.default


def _uop():
    return torch.ops.bitsandbytes_amd.gemm_4bit_lora.default


def _plain_op():
    return torch.ops.bitsandbytes.gemm_4bit.default


def _esupported(dtype, M, N, K, bs, nested, r, A_n) -> bool:
    return _bnb().lib.bnb_mi355x_gemm_4bit_lora_ids_supported(C.DT_CODE[dtype], M, N, K, bs, 1 if nested else 0, r, A_n) == 1


def _usupported(dtype, M, N, K, bs, nested, r) -> bool:
    return _bnb().lib.bnb_mi355x_gemm_4bit_lora_supported(C.DT_CODE[dtype], M, N, K, bs, 1 if nested else 0, r) == 1


@functools.lru_cache(maxsize=None)
def _base(base_case):
    """The base layer of an exact case on the device, shared by the expand cases on it; computed once, never written to."""
    Fn = _bnb().functional
    ex = LC.build_case(base_case)
    packed = X.check_quantization(ex, gpu_ops(), DEV)
    absmax, a8, code, off = ex.stats_args(DEV)
    x = ex.x.to(DEV)[:C.MAX_ROWS]
    y64 = (x.double() @ ex.W.to(DEV).double().t()).cpu()
    shape = torch.Size((base_case.N, base_case.K))
    code4 = Fn.get_4bit_type("fp4", device=DEV)
    if base_case.nested:
        state2 = Fn.QuantState(absmax=absmax, code=code, blocksize=256, dtype=torch.float32)
        state = Fn.QuantState(absmax=a8, shape=shape, code=code4, blocksize=base_case.blocksize, quant_type="fp4", dtype=base_case.dtype, offset=off,
                              state2=state2)
    else:
        state = Fn.QuantState(absmax=absmax, shape=shape, code=code4, blocksize=base_case.blocksize, quant_type="fp4", dtype=base_case.dtype)
    return dict(packed=packed, absmax=absmax, stats=dict(absmax_8bit=a8, absmax_code=code, absmax_offset=off), x=x, bias=ex.bias.to(DEV), y64=y64,
                bias64=ex.bias.double(), state=state)


@pytest.mark.parametrize("case", C.EXPAND_CASES, ids=lambda c: c.name)
def test_expand_exact_with_each_rows_adapter(case):
    """Exact operands: the op (where the predicate serves the cell - never on 2002 x 1024 at 5 ... 8 rows, where it raises) and the
    public function equal T(x64 W64^T + bias64 + s_id t64 B_id64^T) per row, the plain result for a row without an adapter; the launch
    is the plain op's family. Where the public function composes, it is inside lora_cases.tolerance per row."""
    bnb = _bnb()
    b = case.base
    N, K, bs = b.N, b.K, b.blocksize
    d = _base(b)
    t, stack, sc = C.build_expand_adapters(case)
    td, sd, scd = t.to(DEV), stack.to(DEV), sc.to(DEV)
    failures, fused, composed = [], 0, 0
    for M in C.expand_ms(case):
        _plain_op()(d["x"][:M], d["packed"], [N, K], d["absmax"], bs, "fp4", None, *d["stats"].values())
        plain_family = bnb.lib.bnb_mi355x_last_gemm_kernel()
        served = _esupported(b.dtype, M, N, K, bs, b.nested, case.r, case.A_n)
        assert served == _usupported(b.dtype, M, N, K, bs, b.nested, case.r)
        assert served == (plain_family in (LC.K_STREAM, LC.K_SM)), (M, served, plain_family)
        for n, (name, vals, idt) in enumerate(C.patterns(M, case.A_n)):
            ids = _ids(vals, idt)
            bias = d["bias"] if n % 2 else None
            want = C.expand_reference(d["y64"][:M], d["bias64"] if n % 2 else None, t[:M], stack, sc, vals, b.dtype)
            args = (d["x"][:M], d["packed"], [N, K], d["absmax"], bs, "fp4", td[:M].contiguous(), sd, scd, ids, bias)
            y2 = bnb.matmul_4bit_lora_ids(d["x"][:M], d["packed"], d["state"], td[:M], sd, scd, ids, bias=bias)
            assert y2.shape == (M, N) and y2.dtype == b.dtype
            if served:
                y = _eop()(*args, **d["stats"])
                assert bnb.lib.bnb_mi355x_last_gemm_kernel() == plain_family
                fused += 1
                for nm, got in (("op", y), ("matmul_4bit_lora_ids", y2)):
                    if not torch.equal(got.cpu(), want):
                        failures.append((M, name, nm, plain_family, X.first_mismatch(got.cpu(), want)))
            else:
                with pytest.raises(ValueError, match="no kernel"):
                    _eop()(*args, **d["stats"])
                composed += 1
                yp = _plain_op()(d["x"][:M], d["packed"], [N, K], d["absmax"], bs, "fp4", bias, *d["stats"].values()).cpu()
                for m, i in enumerate(vals):
                    if 0 <= i < case.A_n:
                        s = float(sc[i])
                        want64 = yp[m:m + 1].double() + LC.adapter_term64(t[m:m + 1], stack[i], s)
                        if bool(((y2[m:m + 1].cpu().double() - want64).abs() > LC.tolerance(want64, yp[m:m + 1], t[m:m + 1], stack[i], s, b.dtype)).any()):
                            failures.append((M, name, "composition", m))
                    elif not torch.equal(y2[m].cpu(), yp[m]):
                        failures.append((M, name, "composition: a row without an adapter is not the plain row", m))
    print(f"{case.name}: {fused} fused and {composed} composed cells, {len(failures)} wrong")
    assert fused >= 8
    if (N, K, bs) in C.EXPAND_OTHER:
        assert composed >= 8
    assert not failures, failures[:5]


def _random_weight(N, K, dtype, seed):
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(N, K, generator=gen) * (3.0 / K ** 0.5)).to(dtype).to(DEV)


def _state_args(state):
    if not state.nested:
        return state.absmax, {}
    return state.state2.absmax, dict(absmax_8bit=state.absmax, absmax_code=state.state2.code, absmax_offset=state.offset)


_CELLS = [(shape, ms, i) for i, (shape, ms) in enumerate(C.EXPAND_MUST_SERVE)]


@pytest.mark.parametrize("shape,ms,i", _CELLS, ids=[f"{s[0]}x{s[1]}-bs{s[2]}" for s, _, _ in _CELLS])
def test_expand_rows_equal_the_uniform_op(shape, ms, i):
    """Every cell of lora_cases.MUST_SERVE (streaming kernel at one row, streaming MFMA kernel at 2 / 4 / 8 / 16 - every skeleton the
    uniform op has), ordinary NF4 / FP4 data, plain and nested statistics, with and without bias. For each distinct id the existing op
    runs with that adapter at the same M: rows that carry the id are torch.equal. Rows without an adapter equal the plain gemm_4bit
    row. With NaN in every adapter no row names - lora_b and scalings - and in the lora_t rows of rows without an adapter, the output
    keeps its bits and holds no NaN. No cell is skipped: the predicate must answer 1."""
    bnb = _bnb()
    N, K, bs = shape
    dtype = C.DTYPES[i % 2]
    r, A_n = LC.RANKS[i % 3], (17, 3, 1)[i % 3]
    for nested in (False, True):
        qt = "nf4" if nested == bool(i % 2) else "fp4"
        packed, state = bnb.functional.quantize_4bit(_random_weight(N, K, dtype, N + K + i), blocksize=bs, quant_type=qt, compress_statistics=nested)
        absmax, kw = _state_args(state)
        gen = torch.Generator().manual_seed(N + 3)
        x = torch.randn(C.MAX_ROWS, K, generator=gen).to(dtype).to(DEV)
        bias_t = torch.randn(N, generator=gen).to(dtype).to(DEV)
        t, stack, sc = (v.to(DEV) for v in C.ordinary_expand(C.MAX_ROWS, A_n, N, r, dtype, N + K))
        for M in ms:
            for A_cnt in sorted({A_n, 1, 17, 64} if M == ms[0] else {A_n}):
                assert _esupported(dtype, M, N, K, bs, nested, r, A_cnt), (shape, M, nested, r, A_cnt)
            alone = {}
            for n, (name, vals, idt) in enumerate(C.patterns(M, A_n)):
                bias = bias_t if (n + int(nested)) % 2 else None
                ids = _ids(vals, idt)
                got = _eop()(x[:M], packed, [N, K], absmax, bs, qt, t[:M].contiguous(), stack, sc, ids, bias, **kw)
                family = bnb.lib.bnb_mi355x_last_gemm_kernel()
                assert family == (LC.K_STREAM if M == 1 else LC.K_SM), (shape, M, family)
                assert not bool(torch.isnan(got).any())
                plain = _plain_op()(x[:M], packed, [N, K], absmax, bs, qt, bias, *kw.values())
                used = sorted({v for v in vals if 0 <= v < A_n})
                for a in used:
                    if (a, bias is None) not in alone:
                        alone[a, bias is None] = _uop()(x[:M], packed, [N, K], absmax, bs, qt, t[:M].contiguous(), stack[a].contiguous(), float(sc[a]), bias, **kw)
                for m, v in enumerate(vals):
                    if 0 <= v < A_n:
                        assert torch.equal(got[m], alone[v, bias is None][m]), (shape, nested, M, name, m, v)
                        assert not torch.equal(got[m], plain[m])
                    else:
                        assert torch.equal(got[m], plain[m]), (shape, nested, M, name, m, v)
                pstack, psc, pt = stack.clone(), sc.clone(), t[:M].clone()
                for a in range(A_n):
                    if a not in used:
                        pstack[a] = float("nan")
                        psc[a] = float("nan")
                for m, v in enumerate(vals):
                    if not 0 <= v < A_n:
                        pt[m] = float("nan")
                again = _eop()(x[:M], packed, [N, K], absmax, bs, qt, pt, pstack, psc, ids, bias, **kw)
                assert torch.equal(again.view(torch.int16), got.view(torch.int16)), (shape, nested, M, name)


def _multi_module(N, K, A_n, ranks, dtype, nested, bias, seed):
    bnb = _bnb()
    gen = torch.Generator().manual_seed(seed)
    layer = bnb.nn.Linear4bit(K, N, bias=bias, quant_type="nf4", compress_statistics=nested, compute_dtype=dtype)
    W = (torch.randn(N, K, generator=gen) * (3.0 / K ** 0.5)).to(dtype)
    layer.weight = bnb.nn.Params4bit(W, requires_grad=False, quant_type="nf4", compress_statistics=nested, blocksize=64, module=layer)
    if bias:
        layer.bias.data = torch.randn(N, generator=gen).to(dtype)
    layer = layer.to(DEV)
    adapters = []
    for a in range(A_n):
        r = ranks[a % len(ranks)]
        adapters.append((torch.randn(r, K, generator=gen) / K ** 0.5, torch.randn(N, r, generator=gen) * 0.5, 0.5 + 0.25 * a))
    with torch.no_grad():
        return layer, adapters, bnb.nn.Linear4bitMultiLoRA.from_adapters(layer, adapters)


@pytest.mark.parametrize("nested,dtype,bias", [(True, torch.bfloat16, True), (False, torch.float16, False)], ids=["nested-bf16-bias", "plain-fp16"])
def test_module_on_ordinary_data(nested, dtype, bias):
    """nn.Linear4bitMultiLoRA.from_adapters (ranks 8, 12 and 24 padded to 24) against the per-row float64 reference with the UNPADDED
    adapter, inside lora_cases.tolerance around (plain output + adapter term with the module's own t): 1 ... 16 rows fused, 17 rows
    composed, leading dims. Every figure is printed."""
    bnb = _bnb()
    N, K, A_n = 4096, 4096, 5
    layer, adapters, mod = _multi_module(N, K, A_n, (8, 12, 24), dtype, nested, bias, 7)
    assert tuple(mod.lora_A.shape) == (A_n, 24, K) and tuple(mod.lora_B.shape) == (A_n, N, 24) and mod.scalings.dtype == torch.float32
    gen = torch.Generator().manual_seed(9)
    with torch.no_grad():
        for lead in ((1,), (2, 2), (16,), (17,)):
            x = torch.randn(*lead, K, generator=gen).to(dtype).to(DEV)
            M = x.numel() // K
            vals = [(3 * m + 1) % (A_n + 2) - 1 for m in range(M)]
            ids = _ids(vals, torch.int64).view(*lead)
            got = mod(x, ids)
            assert got.shape == (*lead, N) and got.dtype == dtype
            t = bnb.lora_shrink_ids(x, mod.lora_A, ids)
            assert torch.equal(got, bnb.matmul_4bit_lora_ids(x, layer.weight, layer.weight.quant_state, t, mod.lora_B, mod.scalings, ids,
                                                             bias=layer.bias.detach() if bias else None))
            assert torch.equal(mod(x, ids, t=t), got)
            yp = layer(x).view(M, N)
            got, t = got.view(M, N), t.view(M, -1)
            worst = 0.0
            for m, v in enumerate(vals):
                if 0 <= v < A_n:
                    a_, b_, s = adapters[v]
                    r = a_.shape[0]
                    bd = b_.to(dtype).to(DEV)
                    # the padded columns of t are exact zeros: the unpadded adapter's term from the module's own t
                    assert not bool(t[m, r:].any())
                    want64 = yp[m:m + 1].double() + LC.adapter_term64(t[m:m + 1, :r], bd, s)
                    tol = LC.tolerance(want64, yp[m:m + 1], t[m:m + 1, :r], bd, s, dtype)
                    worst = max(worst, float(((got[m:m + 1].double() - want64).abs() / tol).max()))
                else:
                    assert torch.equal(got[m], yp[m]), (lead, m)
            print(f"{dtype} nested={nested} lead={lead}: worst error / bound {worst:.3f}")
            assert worst <= 1.0, (lead, worst)


@pytest.mark.parametrize("M", [1, 4, 16])
def test_captured_layer_follows_the_ids(M):
    """Shrink + expand of one layer in ONE torch.cuda.graph (a plain chain of two launches), ids overwritten in place between the
    replays: each replay matches the eager result for its own ids."""
    layer, adapters, mod = _multi_module(2816 if M == 1 else 4096, 2048 if M == 1 else 4096, 5, (16,), torch.bfloat16, True, True, 11)
    K = layer.in_features
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(13)).bfloat16().to(DEV)
    sets = [[(3 * m + k) % 7 - 1 for m in range(M)] for k in (0, 2, 5)]
    with torch.no_grad():
        eager = [mod(x, _ids(v, torch.int32)) for v in sets]
        assert not torch.equal(eager[1], eager[2])
        buf = _ids(sets[0], torch.int32)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                mod(x, buf)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            y = mod(x, buf)
        for k in (1, 2):
            buf.copy_(_ids(sets[k], torch.int32))
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(y, eager[k]), f"replay {k} did not follow the ids"


def test_shrink_group_parts_equal_the_members():
    """Two layers that share x: one lora_shrink_ids launch over the per-adapter concatenation gives each member the bits of its own
    shrink, and forward(x, ids, t=part) the bits of forward(x, ids)."""
    bnb = _bnb()
    l1, _, m1 = _multi_module(2816, 2048, 3, (16,), torch.bfloat16, False, False, 21)
    l2, _, m2 = _multi_module(4096, 2048, 3, (8, 24), torch.bfloat16, False, True, 22)
    x = torch.randn(4, 2048, generator=torch.Generator().manual_seed(5)).bfloat16().to(DEV)
    ids = _ids([2, -1, 0, 1], torch.int32)
    with torch.no_grad():
        p1, p2 = bnb.nn.Linear4bitMultiLoRA.shrink_group(x, [m1, m2], ids)
        assert p1.shape == (4, 16) and p2.shape == (4, 24) and p1.is_contiguous() and p2.is_contiguous()
        assert torch.equal(p1, bnb.lora_shrink_ids(x, m1.lora_A, ids)) and torch.equal(p2, bnb.lora_shrink_ids(x, m2.lora_A, ids))
        assert torch.equal(m1(x, ids, t=p1), m1(x, ids)) and torch.equal(m2(x, ids, t=p2), m2(x, ids))


def test_expand_opcheck():
    bnb = _bnb()
    N, K, r, A_n = 4096, 4096, 16, 5
    dtype = torch.bfloat16
    packed, state = bnb.functional.quantize_4bit(_random_weight(N, K, dtype, 3), blocksize=64, quant_type="nf4", compress_statistics=True)
    absmax, kw = _state_args(state)
    stack = (torch.randn(A_n, N, r, device=DEV) * 0.5).to(dtype)
    sc = torch.rand(A_n, device=DEV) + 0.5
    for lead in ((1,), (3,), (2, 2)):
        x = torch.randn(*lead, K, device=DEV).to(dtype)
        t = torch.randn(*lead, r, device=DEV).to(dtype)
        for idt in (torch.int32, torch.int64):
            ids = torch.randint(-1, A_n + 1, lead, device=DEV, dtype=idt)
            torch.library.opcheck(_eop(), (x, packed, [N, K], absmax, 64, "nf4", t, stack, sc, ids), kw, test_utils=("test_schema", "test_faketensor"))
    assert _eop()(x[:0], packed, [N, K], absmax, 64, "nf4", t[:0], stack, sc, ids[:0], **kw).shape == (0, 2, N)
    with pytest.raises(ValueError, match="no kernel"):
        _eop()(torch.randn(17, K, device=DEV).to(dtype), packed, [N, K], absmax, 64, "nf4", torch.randn(17, r, device=DEV).to(dtype), stack, sc,
               torch.zeros(17, dtype=torch.int32, device=DEV), **kw)
