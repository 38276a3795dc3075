"""GPU: the fused expert FFN - the gated-SiLU and routing-weight epilogues of the expert-indexed kernel
(bitsandbytes_amd::gemm_4bit_experts_ffn, csrc/gemm4_experts.hip) and the block ``moe_ffn_4bit``.

* gated, exact: on the operands of tests/exact_inputs.py (tests/moe_ffn_cases.py) the output equals ``F.silu(ref_g) * ref_u`` - torch's
  own kernels on the GPU, on the two halves of the float64 reference rounded once - bit for bit, for both layouts, both forms of ``x``,
  both id dtypes, P in {1, 2, 5, 16, 65} and five id patterns, with and without bias. The interleaved stack of a plain-statistics
  case is the chunked one with its rows permuted before quantization. With nested statistics that stack cannot be built exactly (a
  permuted block lands in another group of 256 blocks, and ``code2 * absmax2`` of the new group does not reach the old scale), so
  there the SAME stack is read as interleaved: gate = its even rows, up = its odd rows.
* gated equals plain, on ordinary NF4 / FP4 data: ``F.silu(h[..., :I]) * h[..., I:]`` of the existing op's output ``h``, bit for bit.
* row scale, exact: ``(ref64.float() * w.float()).to(T)`` bit for bit; a NaN scale on a dropped pair gives zeros.
* the block against the parent-ops composition, graph capture, determinism, isolation, opcheck, the parametrize helper.
The preconditions are asserted on the CPU by tests/test_moe_ffn_host.py.
"""
import copy
import functools

import pytest
import torch
import torch.nn.functional as TF

import exact_inputs as X
import moe_ffn_cases as C
from conftest import rel_err
from routed_sweep import gpu_ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
K_EXPERTS = 9
PARITY_BAR = 1e-2   # README "Parity bars": fused matmuls against the oracle


def _bnb():
    import bitsandbytes_amd as bnb

    return bnb


def _op():
    return torch.ops.bitsandbytes_amd.gemm_4bit_experts_ffn.default


def _old_op():
    return torch.ops.bitsandbytes_amd.gemm_4bit_experts.default


# ------------------------------------------------------------------------------------------ exact
@functools.lru_cache(maxsize=None)
def _prepared(case):
    """Everything of a case that its tests share, computed once and never written to: the quantized stacks, the statistics, the
    activations, the biases and the float64 products of every activation row with every expert."""
    E, N, K = case.E, case.N, case.K
    ex = C.build_case(case)
    ops = gpu_ops()
    packed = X.check_quantization(ex, ops, DEV)
    absmax, a8, code, off = ex.stats_args(DEV)
    W = ex.W.to(DEV).view(E, N, K)
    x_all = ex.x.to(DEV)
    y64 = torch.stack([x_all.double() @ W[e].double().t() for e in range(E)])        # [E, rows, N]; exact (exact_inputs.py)
    bias = ex.bias.view(E, N).to(DEV)
    d = dict(ex=ex, packed=packed, stats=(absmax, a8, code, off), x=x_all, y64=y64, bias=bias)
    if not case.nested:
        Wi = C.interleave_rows(ex.W, E, N).contiguous().to(DEV)
        packed_i, absmax_i = ops.quantize_4bit(Wi, case.blocksize)
        bpr = K // case.blocksize
        assert torch.equal(absmax_i.flatten().cpu(), C.interleave_rows(ex.scale.view(-1, bpr), E, N).reshape(-1))
        back = ops.dequantize_4bit(packed_i, absmax_i, case.blocksize, (E * N, K), case.dtype)
        assert torch.equal(back.view(torch.uint8), Wi.view(torch.uint8)), "the interleaved stack does not survive quantization"
        d.update(packed_i=packed_i, absmax_i=absmax_i.flatten(), bias_i=C.interleave_rows(ex.bias, E, N).view(E, N).to(DEV))
    return d


def _gated_operands(case, d, layout):
    """(packed, absmax, bias [E, 2 I] in the stack's layout, g64, u64 [E, rows, I], gate bias, up bias [E, I])."""
    I = case.N // 2
    y64, bias = d["y64"], d["bias"]
    if layout == "chunked":
        return d["packed"], d["stats"][0], bias, y64[..., :I], y64[..., I:], bias[:, :I], bias[:, I:]
    if not case.nested:   # the permuted stack: the same (gate, up) values at other rows
        return d["packed_i"], d["absmax_i"], d["bias_i"], y64[..., :I], y64[..., I:], bias[:, :I], bias[:, I:]
    return d["packed"], d["stats"][0], bias, y64[..., 0::2], y64[..., 1::2], bias[:, 0::2], bias[:, 1::2]


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.name)
def test_gated_exact_for_every_id_pattern(case):
    lib = _bnb().lib
    E, N, K = case.E, case.N, case.K
    I = N // 2
    d = _prepared(case)
    _, a8, code, off = d["stats"]
    x_all = d["x"]
    gen = torch.Generator().manual_seed(case.seed)
    failures, calls = [], 0
    for P in C.P_VALUES:
        T, S = C.TS_OF_P[P]
        for pattern in C.ID_PATTERNS:
            ids_cpu = C.make_ids(pattern, P, E, gen)
            ids64 = ids_cpu.to(DEV)
            valid = (ids64 >= 0) & (ids64 < E)
            safe = ids64.clamp(0, E - 1)
            pair = torch.arange(P, device=DEV)
            for layout in ("chunked", "interleaved"):
                packed, absmax, bias, g64, u64, bg, bu = _gated_operands(case, d, layout)
                for per_slot in (False, True):
                    x = x_all[:P].view(T, S, K) if per_slot else x_all[:T]
                    xrow = pair if per_slot else pair // S
                    for with_bias in (False, True):
                        g = g64[safe, xrow] + (bg.double()[safe] if with_bias else 0.0)
                        u = u64[safe, xrow] + (bu.double()[safe] if with_bias else 0.0)
                        want = TF.silu(g.to(case.dtype)) * u.to(case.dtype)          # torch's kernels on T-valued tensors
                        want = torch.where(valid[:, None], want, torch.zeros_like(want))
                        for idt in (torch.int32, torch.int64):
                            ids = ids64.to(idt).view(T, S)
                            y = _op()(x, packed, [E, N, K], absmax, ids, case.blocksize, "fp4", bias if with_bias else None, a8, code, off,
                                      None, layout)
                            calls += 1
                            assert lib.bnb_mi355x_last_gemm_kernel() == K_EXPERTS
                            assert y.shape == (T, S, I) and y.dtype == case.dtype
                            y = y.view(P, I)
                            if not torch.equal(y, want):
                                r, c, got, exp = X.first_mismatch(y.cpu(), want.cpu())
                                failures.append(f"P={P} {pattern} {layout} x={'TSK' if per_slot else 'TK'} bias={int(with_bias)} {idt}: "
                                                f"pair {r} (id {int(ids_cpu[r])}) column {c}: got {got!r}, want {exp!r}")
    print(f"{case.name}: {calls} gated calls, {len(failures)} not bit-equal")
    assert not failures, f"{len(failures)} of {calls} calls differ; first: {failures[:5]}"


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.name)
def test_row_scale_exact_for_every_id_pattern(case):
    lib = _bnb().lib
    E, N, K = case.E, case.N, case.K
    d = _prepared(case)
    absmax, a8, code, off = d["stats"]
    packed, x_all, y64, bias = d["packed"], d["x"], d["y64"], d["bias"]
    gen = torch.Generator().manual_seed(case.seed + 1)
    failures, calls = [], 0
    for P in C.P_VALUES:
        T, S = C.TS_OF_P[P]
        for pattern in C.ID_PATTERNS:
            ids_cpu = C.make_ids(pattern, P, E, gen)
            ids64 = ids_cpu.to(DEV)
            valid = (ids64 >= 0) & (ids64 < E)
            safe = ids64.clamp(0, E - 1)
            pair = torch.arange(P, device=DEV)
            w32 = (torch.rand(P, generator=gen) * 2 - 0.5).to(DEV)
            for sdt in (torch.float32, case.dtype):
                w = w32.to(sdt)
                w_poisoned = torch.where(valid, w, torch.full_like(w, float("nan")))   # a NaN scale on every dropped pair
                for per_slot in (False, True):
                    x = x_all[:P].view(T, S, K) if per_slot else x_all[:T]
                    xrow = pair if per_slot else pair // S
                    for with_bias in (False, True):
                        ref64 = y64[safe, xrow] + (bias.double()[safe] if with_bias else 0.0)
                        want = (ref64.float() * w.float()[:, None]).to(case.dtype)
                        want = torch.where(valid[:, None], want, torch.zeros_like(want))
                        for idt in (torch.int32, torch.int64):
                            ids = ids64.to(idt).view(T, S)
                            y = _op()(x, packed, [E, N, K], absmax, ids, case.blocksize, "fp4", bias if with_bias else None, a8, code, off,
                                      w_poisoned.view(T, S), "none")
                            calls += 1
                            assert lib.bnb_mi355x_last_gemm_kernel() == K_EXPERTS
                            assert y.shape == (T, S, N) and y.dtype == case.dtype
                            y = y.view(P, N)
                            if not torch.equal(y, want):
                                r, c, got, exp = X.first_mismatch(y.cpu(), want.cpu())
                                failures.append(f"P={P} {pattern} w={sdt} x={'TSK' if per_slot else 'TK'} bias={int(with_bias)} {idt}: pair {r} "
                                                f"(id {int(ids_cpu[r])}, scale {float(w_poisoned[r])!r}) column {c}: got {got!r}, want {exp!r}")
            # neither option through the new op: the old op's bits
            ids = ids64.view(T, S)
            new = _op()(x_all[:T], packed, [E, N, K], absmax, ids, case.blocksize, "fp4", bias, a8, code, off)
            old = _old_op()(x_all[:T], packed, [E, N, K], absmax, ids, case.blocksize, "fp4", bias, a8, code, off)
            calls += 1
            if not torch.equal(new, old):
                failures.append(f"P={P} {pattern}: the new op without options differs from gemm_4bit_experts")
    print(f"{case.name}: {calls} row-scale calls, {len(failures)} not bit-equal")
    assert not failures, f"{len(failures)} of {calls} calls differ; first: {failures[:5]}"


# ------------------------------------------------------------------------------------------ ordinary data
def _quantize(W, nested, qt, bs=64):
    return _bnb().functional.quantize_4bit(W, blocksize=bs, compress_statistics=nested, quant_type=qt)


def _random_stack(E, N, K, dtype, seed):
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(E, N, K, generator=gen) / K ** 0.5).to(dtype).to(DEV)


_ids = lambda v: "-".join(str(x).replace("torch.", "") for x in v)
GATED_SHAPES = [(torch.bfloat16, False, "nf4"), (torch.bfloat16, True, "fp4"), (torch.float16, True, "nf4"), (torch.float32, False, "fp4")]


@pytest.mark.parametrize("cfg", GATED_SHAPES, ids=_ids)
def test_gated_equals_silu_mul_of_the_plain_output(cfg):
    """6 x 400 x 2560 (I = 200: twelve 16-column tiles and one of 8; K = one full and one partial segment), ordinary data: the gated
    call's bits are torch's ``F.silu(g) * u`` on the existing op's output, in both layouts, with and without bias."""
    bnb = _bnb()
    dtype, nested, qt = cfg
    E, N, K = 6, 400, 2560
    I = N // 2
    W = _random_stack(E, N, K, dtype, 11)
    gen = torch.Generator().manual_seed(12)
    T, S = 7, 3
    x = torch.randn(T, K, generator=gen).to(dtype).to(DEV)
    ids = torch.randint(-1, E + 1, (T, S), generator=gen).to(DEV)
    bias = torch.randn(E, N, generator=gen).to(dtype).to(DEV)
    for layout in ("chunked", "interleaved"):
        if layout == "interleaved":
            Wl = C.interleave_rows(W.view(E * N, K), E, N).contiguous().view(E, N, K)
            bl = C.interleave_rows(bias.view(E * N), E, N).contiguous().view(E, N)
        else:
            Wl, bl = W, bias
        packed, state = _quantize(Wl, nested, qt)
        for b in (None, bl):
            h = bnb.matmul_4bit_experts(x, packed, state, ids, bias=b)
            g, u = (h[..., 0::2], h[..., 1::2]) if layout == "interleaved" else (h[..., :I], h[..., I:])
            want = TF.silu(g) * u
            got = bnb.matmul_4bit_experts(x, packed, state, ids, bias=b, gated=layout)
            assert bnb.lib.bnb_mi355x_last_gemm_kernel() == K_EXPERTS
            assert got.shape == (T, S, I) and torch.isfinite(got).all()
            assert torch.equal(got, want), (layout, b is not None, X.first_mismatch(got.view(-1, I).cpu(), want.reshape(-1, I).cpu()))
            assert float(want.abs().max()) > 0


# ------------------------------------------------------------------------------------------ the block
# E = 6, H = 512, S = 2, T in {1, 5}. I = 192, not 200: I is the K of the down projection, and the kernel (like the parent's) needs
# K % blocksize == 0 with a power-of-two blocksize >= 32 - no such blocksize divides 200, so neither the block nor the parent-ops
# composition it is compared with can run there; 192 = 3 x 64 is the nearest size both serve. (A partial column tile, which I = 200
# would also have given, is covered by I = 72 of the exact cases and I = 200 of the gated-equals-plain test.)
BLOCK = dict(E=6, I=192, H=512, S=2)


@functools.lru_cache(maxsize=None)
def _block(dtype, nested=True, qt="nf4"):
    E, I, H = BLOCK["E"], BLOCK["I"], BLOCK["H"]
    Wgu = _random_stack(E, 2 * I, H, dtype, 21)
    Wdn = _random_stack(E, H, I, dtype, 22)
    gu, gu_state = _quantize(Wgu, nested, qt)
    dn, dn_state = _quantize(Wdn, nested, qt)
    gen = torch.Generator().manual_seed(23)
    bgu = (torch.randn(E, 2 * I, generator=gen) * 0.1).to(dtype).to(DEV)
    bdn = (torch.randn(E, H, generator=gen) * 0.1).to(dtype).to(DEV)
    return gu, gu_state, dn, dn_state, bgu, bdn


def _routing(T, S, E, seed, masked=True):
    gen = torch.Generator().manual_seed(seed)
    ids = torch.randint(-1 if masked else 0, E + (1 if masked else 0), (T, S), generator=gen).to(DEV)
    w = torch.softmax(torch.randn(T, S, generator=gen), dim=-1).to(DEV)
    return ids, w


def _parent_block(x, gu, gu_state, dn, dn_state, ids, w, bgu, bdn):
    """The block from the operations of the parent commit: two plain launches and the caller's glue."""
    bnb = _bnb()
    h = bnb.matmul_4bit_experts(x, gu, gu_state, ids, bias=bgu)
    g, u = h.chunk(2, dim=-1)
    a = TF.silu(g) * u
    y = bnb.matmul_4bit_experts(a, dn, dn_state, ids, bias=bdn)
    return (y * w.unsqueeze(-1).to(y.dtype)).sum(dim=1)


@pytest.mark.parametrize("T", [1, 5])
def test_block_fp32_is_bit_equal_to_the_parent_ops(T):
    bnb = _bnb()
    gu, gu_state, dn, dn_state, bgu, bdn = _block(torch.float32)
    ids, w = _routing(T, BLOCK["S"], BLOCK["E"], 30 + T)
    x = torch.randn(T, BLOCK["H"], generator=torch.Generator().manual_seed(31)).to(DEV)
    y = bnb.moe_ffn_4bit(x, gu, gu_state, dn, dn_state, ids, w, gate_up_bias=bgu, down_bias=bdn)
    ref = _parent_block(x, gu, gu_state, dn, dn_state, ids, w, bgu, bdn)
    assert y.shape == (T, BLOCK["H"]) and y.dtype == torch.float32
    assert torch.equal(y, ref), X.first_mismatch(y.cpu(), ref.cpu())


@pytest.mark.parametrize("T", [1, 5])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_block_16bit_is_no_worse_than_the_parent_ops(dtype, T):
    """Relative Frobenius error against a float64 block built from the dequantized weights: the fused form (one rounding fewer: the
    routing weight enters in fp32 in front of the down projection's rounding) at most 1.5 x the parent-ops composition's - the margin
    covers rounding noise at this size (T * 512 outputs)."""
    bnb = _bnb()
    F = bnb.functional
    E, I, H, S = BLOCK["E"], BLOCK["I"], BLOCK["H"], BLOCK["S"]
    gu, gu_state, dn, dn_state, bgu, bdn = _block(dtype)
    ids, w = _routing(T, S, E, 40 + T)
    x = torch.randn(T, H, generator=torch.Generator().manual_seed(41)).to(dtype).to(DEV)
    y = bnb.moe_ffn_4bit(x, gu, gu_state, dn, dn_state, ids, w, gate_up_bias=bgu, down_bias=bdn)
    parent = _parent_block(x, gu, gu_state, dn, dn_state, ids, w, bgu, bdn)
    assert y.shape == (T, H) and y.dtype == dtype
    Wgu = F.dequantize_4bit(gu, gu_state).double().view(E, 2 * I, H)
    Wdn = F.dequantize_4bit(dn, dn_state).double().view(E, H, I)
    valid = ((ids >= 0) & (ids < E)).double()
    safe = ids.clamp(0, E - 1)
    h = torch.einsum("tsnk,tk->tsn", Wgu[safe], x.double()) + bgu.double()[safe]
    a = TF.silu(h[..., :I]) * h[..., I:]
    o = torch.einsum("tshi,tsi->tsh", Wdn[safe], a) + bdn.double()[safe]
    ref = (o * (w.double() * valid).unsqueeze(-1)).sum(dim=1)
    err_new, err_parent = rel_err(y, ref), rel_err(parent, ref)
    print(f"block {dtype} T={T}: relative error fused {err_new:.3e}, parent ops {err_parent:.3e}")
    assert err_new <= 1.5 * err_parent


def test_captured_block_follows_ids_and_weights():
    """One torch.cuda.graph of the whole block, replayed with ids and routing weights rewritten in place: the host read neither."""
    bnb = _bnb()
    E, H, S, T = BLOCK["E"], BLOCK["H"], BLOCK["S"], 5
    gu, gu_state, dn, dn_state, bgu, bdn = _block(torch.bfloat16)
    x = torch.randn(T, H, generator=torch.Generator().manual_seed(51)).bfloat16().to(DEV)
    sets = [_routing(T, S, E, 52 + k) for k in range(4)]
    call = lambda i, w: bnb.moe_ffn_4bit(x, gu, gu_state, dn, dn_state, i, w, gate_up_bias=bgu, down_bias=bdn)
    eager = [call(i, w) for i, w in sets]
    assert not torch.equal(eager[1], eager[2])
    ids_buf, w_buf = sets[0][0].clone(), sets[0][1].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            call(ids_buf, w_buf)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = call(ids_buf, w_buf)
    for k in (1, 2, 3):
        ids_buf.copy_(sets[k][0])
        w_buf.copy_(sets[k][1])
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(y, eager[k]), f"replay {k} did not follow the ids and weights"


# ------------------------------------------------------------------------------------------ other properties
def test_twenty_launches_give_equal_bits():
    bnb = _bnb()
    E, H, S, T = BLOCK["E"], BLOCK["H"], BLOCK["S"], 5
    gu, gu_state, dn, dn_state, bgu, bdn = _block(torch.bfloat16)
    x = torch.randn(T, H, generator=torch.Generator().manual_seed(61)).bfloat16().to(DEV)
    ids, w = _routing(T, S, E, 62)
    first_h = bnb.matmul_4bit_experts(x, gu, gu_state, ids, bias=bgu, gated="chunked")
    first_y = bnb.matmul_4bit_experts(first_h, dn, dn_state, ids, bias=bdn, row_scale=w)
    first = bnb.moe_ffn_4bit(x, gu, gu_state, dn, dn_state, ids, w, gate_up_bias=bgu, down_bias=bdn)
    for _ in range(20):
        assert torch.equal(bnb.matmul_4bit_experts(x, gu, gu_state, ids, bias=bgu, gated="chunked"), first_h)
        assert torch.equal(bnb.matmul_4bit_experts(first_h, dn, dn_state, ids, bias=bdn, row_scale=w), first_y)
        assert torch.equal(bnb.moe_ffn_4bit(x, gu, gu_state, dn, dn_state, ids, w, gate_up_bias=bgu, down_bias=bdn), first)


def test_unselected_experts_do_not_reach_the_output():
    """Plain statistics: the absmax of every expert nobody selected is NaN in both stacks - no output bit changes."""
    bnb = _bnb()
    E, I, H, S = BLOCK["E"], BLOCK["I"], BLOCK["H"], BLOCK["S"]
    gu, gu_state, dn, dn_state, bgu, bdn = _block(torch.bfloat16, False, "fp4")
    x = torch.randn(4, H, generator=torch.Generator().manual_seed(71)).bfloat16().to(DEV)
    ids = torch.tensor([[1, 4], [4, 1], [1, -1], [E, 4]], dtype=torch.int32, device=DEV)
    w = torch.tensor([[0.5, 0.5], [0.25, 0.75], [1.0, float("nan")], [float("nan"), 1.0]], device=DEV)
    clean = bnb.moe_ffn_4bit(x, gu, gu_state, dn, dn_state, ids, w, gate_up_bias=bgu, down_bias=bdn)
    assert torch.isfinite(clean).all()
    poisoned = []
    for state in (gu_state, dn_state):
        p = copy.deepcopy(state)
        am = p.absmax.view(E, -1)
        for e in range(E):
            if e not in (1, 4):
                am[e] = float("nan")
        poisoned.append(p)
    y = bnb.moe_ffn_4bit(x, gu, poisoned[0], dn, poisoned[1], ids, w, gate_up_bias=bgu, down_bias=bdn)
    assert torch.equal(y, clean)
    h = bnb.matmul_4bit_experts(x, gu, poisoned[0], ids, gated="chunked")
    assert h.shape == (4, S, I) and bool((h[2, 1] == 0).all()) and bool((h[3, 0] == 0).all()) and torch.isfinite(h).all()


def test_opcheck():
    E, N, K = 4, 96, 256
    for nested in (False, True):
        W = _random_stack(E, N, K, torch.bfloat16, 81)
        packed, state = _quantize(W, nested, "nf4")
        x = torch.randn(3, 2, K, device=DEV).bfloat16()
        ids = torch.randint(0, E, (3, 2), device=DEV)
        bias = torch.randn(E, N, device=DEV).bfloat16()
        if nested:
            args = (x, packed, [E, N, K], state.state2.absmax, ids, 64, "nf4")
            kwargs = dict(bias=bias, absmax_8bit=state.absmax, absmax_code=state.state2.code, absmax_offset=state.offset)
        else:
            args = (x, packed, [E, N, K], state.absmax, ids, 64, "nf4")
            kwargs = dict(bias=bias)
        for extra in (dict(gated="chunked"), dict(gated="interleaved"), dict(row_scale=torch.rand(3, 2, device=DEV)),
                      dict(row_scale=torch.rand(3, 2, device=DEV).bfloat16()), dict()):
            torch.library.opcheck(_op(), args, {**kwargs, **extra}, test_utils=("test_schema", "test_faketensor"))
    # what the fake kernel cannot see: a geometry the kernel does not serve is an error, never another path
    bnb = _bnb()
    Kbig = 1 << 18
    pb, sb = _quantize(torch.randn(1, 32, Kbig, device=DEV).bfloat16(), False, "nf4")
    with pytest.raises(ValueError, match="no kernel"):
        bnb.matmul_4bit_experts(torch.randn(1, Kbig, device=DEV).bfloat16(), pb, sb, ids[:1, :1], gated="chunked")
    # P = 0: an empty tensor
    assert bnb.matmul_4bit_experts(x[:0], packed, state, ids[:0], gated="chunked").shape == (0, 2, N // 2)


def _experts_module(dtype=torch.bfloat16, nested=True, blocksize=64):
    from bitsandbytes_amd.nn import parametrize as bp

    E, I, H = BLOCK["E"], BLOCK["I"], BLOCK["H"]

    class Experts(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.gate_up_proj = torch.nn.Parameter(_random_stack(E, 2 * I, H, dtype, 21))
            self.down_proj = torch.nn.Parameter(_random_stack(E, H, I, dtype, 22))

    m = Experts()
    for name in ("gate_up_proj", "down_proj"):
        bp.replace_parameter_4bit(m, name, compress_statistics=nested, quant_type="nf4", blocksize=blocksize)
    return m


def test_parametrize_helper_equals_the_functional_call():
    import torch.nn.utils.parametrize as P

    bnb = _bnb()
    from bitsandbytes_amd.nn import parametrize as bp

    E, H, S, T = BLOCK["E"], BLOCK["H"], BLOCK["S"], 5
    m = _experts_module()
    gu, gu_state, dn, dn_state, bgu, bdn = _block(torch.bfloat16)     # (the same weights, quantized the same way)
    x = torch.randn(T, H, generator=torch.Generator().manual_seed(91)).bfloat16().to(DEV)
    ids, w = _routing(T, S, E, 92)
    P._cache.clear()
    y = bp.moe_ffn_4bit(m, "gate_up_proj", "down_proj", x, ids, w, gate_up_bias=bgu, down_bias=bdn)
    assert bnb.lib.bnb_mi355x_last_gemm_kernel() == K_EXPERTS and len(P._cache) == 0
    ref = bnb.moe_ffn_4bit(x, gu, gu_state, dn, dn_state, ids, w, gate_up_bias=bgu, down_bias=bdn)
    assert y.shape == (T, H) and torch.equal(y, ref)
    with pytest.raises(ValueError, match="not a parametrized"):
        bp.moe_ffn_4bit(torch.nn.Linear(4, 4), "weight", "bias", x, ids, w)


@pytest.mark.parametrize("gated", ["chunked", "interleaved"])
def test_parametrize_helper_unfused_fallback(monkeypatch, gated):
    """Where the library refuses the geometry the helper composes its own matmul_4bit_experts with torch's silu, * and sum: the same
    block at the project's parity bar (the composition rounds once more), a NaN weight on a dropped slot still gives zeros."""
    from bitsandbytes_amd.backends import hip
    from bitsandbytes_amd.nn import parametrize as bp

    E, H, S, T = BLOCK["E"], BLOCK["H"], BLOCK["S"], 5
    m = _experts_module()
    x = torch.randn(T, H, generator=torch.Generator().manual_seed(93)).bfloat16().to(DEV)
    ids, w = _routing(T, S, E, 94)
    w = torch.where((ids >= 0) & (ids < E), w, torch.full_like(w, float("nan")))
    fused = bp.moe_ffn_4bit(m, "gate_up_proj", "down_proj", x, ids, w, gated=gated)
    calls = []
    monkeypatch.setattr(hip, "gemm_4bit_experts_ffn_supported", lambda *a, **k: calls.append(a) or False)
    unfused = bp.moe_ffn_4bit(m, "gate_up_proj", "down_proj", x, ids, w, gated=gated)
    assert calls, "the helper did not ask the library"
    assert unfused.shape == fused.shape and torch.isfinite(unfused).all() and torch.isfinite(fused).all()
    err = rel_err(unfused, fused)
    print(f"unfused fallback ({gated}) against the fused block: relative error {err:.3e} (bar {PARITY_BAR})")
    assert err <= PARITY_BAR
