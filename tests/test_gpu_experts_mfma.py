"""GPU: the expert-indexed MFMA kernel (csrc/gemm4_experts_mfma.hip, family 12) - ``matmul_4bit_experts_batched`` and the block
``moe_ffn_4bit_batched``. Exact: on the operands of tests/exact_inputs.py (tests/experts_mfma_cases.py; the CPU premise is
tests/test_experts_mfma_host.py) every output is the float64 product rounded once, bit for bit."""
import copy
import ctypes as ct

import pytest
import torch
import torch.nn.functional as TF

import exact_inputs as X
import experts_mfma_cases as C
from conftest import rel_err
from experts_cases import make_ids
from test_gpu_moe_combine import _float64_block
from test_gpu_moe_ffn import BLOCK, PARITY_BAR, _block, _bnb, _experts_module, _gated_operands, _prepared, _quantize, _random_stack, _routing

pytestmark = pytest.mark.gpu

DEV = "cuda"
K_MFMA = 12
EPILOGUES = ("none", "chunked", "interleaved", "scale")

_op = lambda: torch.ops.bitsandbytes_amd.gemm_4bit_experts_mfma.default


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.name)
def test_exact_for_every_epilogue_and_id_pattern(case):
    lib = _bnb().lib
    E, N, K = case.E, case.N, case.K
    d = _prepared(case)
    absmax, a8, code, off = d["stats"]
    gen = torch.Generator().manual_seed(case.seed)
    failures, calls = [], 0
    for pattern, P in C.ID_SETS:
        T, S = C.TS_OF_P[P]
        ids_cpu = make_ids(pattern, P, E, gen)
        if pattern == "masked":
            ids_cpu[0], ids_cpu[1] = -1, E
        ids64 = ids_cpu.to(DEV)
        valid, safe, pair = ((ids64 >= 0) & (ids64 < E))[:, None], ids64.clamp(0, E - 1), torch.arange(P, device=DEV)
        w = (torch.rand(P, generator=gen) * 2 - 0.5).to(DEV)
        for epi in EPILOGUES:
            gated = epi if epi in ("chunked", "interleaved") else "none"
            packed, am, bias, g64, u64, bg, bu = _gated_operands(case, d, gated if gated != "none" else "chunked")
            for sdt in ((torch.float32, case.dtype) if epi == "scale" else (None,)):
                scale = None if sdt is None else torch.where(valid[:, 0], w.to(sdt), torch.full_like(w.to(sdt), float("nan")))
                for per_slot in (False, True):
                    x = d["x"][:P].view(T, S, K) if per_slot else d["x"][:T]
                    xrow = pair if per_slot else pair // S
                    for with_bias in (False, True):
                        if gated != "none":
                            g = g64[safe, xrow] + (bg.double()[safe] if with_bias else 0.0)
                            u = u64[safe, xrow] + (bu.double()[safe] if with_bias else 0.0)
                            want = TF.silu(g.to(case.dtype)) * u.to(case.dtype)       # torch's kernels on T-valued tensors
                        else:
                            ref64 = d["y64"][safe, xrow] + (d["bias"].double()[safe] if with_bias else 0.0)
                            want = ref64.to(case.dtype) if scale is None else (ref64.float() * w.to(sdt).float()[:, None]).to(case.dtype)
                        want = torch.where(valid, want, torch.zeros_like(want))
                        for idt in (torch.int32, torch.int64):
                            y = _op()(x, packed, [E, N, K], am, ids64.to(idt).view(T, S), case.blocksize, "fp4", bias if with_bias else None,
                                      a8, code, off, None if scale is None else scale.view(T, S), gated)
                            calls += 1
                            assert lib.bnb_mi355x_last_gemm_kernel() == K_MFMA and y.shape == (T, S, want.shape[1]) and y.dtype == case.dtype
                            if not torch.equal(y.view(P, -1), want):
                                failures.append((pattern, P, epi, sdt, per_slot, with_bias, idt, X.first_mismatch(y.view(P, -1).cpu(), want.cpu())))
    print(f"{case.name}: {calls} calls, {len(failures)} not bit-equal")
    assert calls and not failures, f"{len(failures)} of {calls} calls differ; first: {failures[:5]}"


def test_a_rows_bits_do_not_depend_on_its_company(request):
    """3 x 400 x 1344, NF4, nested, bf16: every row of a 33-pair call is the row of a call of that pair alone, and the call planned for
    32 compute units (seven 16-row tiles per workgroup instead of two) returns the default plan's bits."""
    bnb = _bnb()
    E, N, K, T, S = 3, 400, 1344, 11, 3
    packed, state = _quantize(_random_stack(E, N, K, torch.bfloat16, 5), True, "nf4")
    gen = torch.Generator().manual_seed(6)
    x = torch.randn(T, K, generator=gen).bfloat16().to(DEV)
    bias = torch.randn(E, N, generator=gen).bfloat16().to(DEV)
    ids, w = _routing(T, S, E, 7)
    request.addfinalizer(lambda: bnb.lib.bnb_mi355x_set_cu_count(0))
    for kw in (dict(), dict(gated="chunked"), dict(gated="interleaved"), dict(row_scale=w)):
        call = lambda xs, i, k: bnb.matmul_4bit_experts_batched(xs, packed, state, i, bias=bias, **k)
        full = call(x, ids, kw)
        assert float(full.abs().max()) > 0
        for t in range(T):
            for s in range(S):
                k1 = dict(kw, row_scale=w[t:t + 1, s:s + 1]) if "row_scale" in kw else kw
                assert torch.equal(call(x[t:t + 1], ids[t:t + 1, s:s + 1], k1)[0, 0], full[t, s]), (kw.keys(), t, s)
        bnb.lib.bnb_mi355x_set_cu_count(32)
        assert torch.equal(call(x, ids, kw), full), kw.keys()
        bnb.lib.bnb_mi355x_set_cu_count(0)


@pytest.mark.parametrize("T", [5, 40])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_batched_block_on_ordinary_data(dtype, T):
    """NF4, nested, against the float64 block, at the project's parity bar for fused matmuls."""
    bnb = _bnb()
    ids, w = _routing(T, BLOCK["S"], BLOCK["E"], 40 + T)
    x = torch.randn(T, BLOCK["H"], generator=torch.Generator().manual_seed(41)).to(dtype).to(DEV)
    gu, gu_state, dn, dn_state, bgu, bdn = _block(dtype)
    y = bnb.moe_ffn_4bit_batched(x, gu, gu_state, dn, dn_state, ids, w, gate_up_bias=bgu, down_bias=bdn)
    assert bnb.lib.bnb_mi355x_last_gemm_kernel() == K_MFMA and y.shape == (T, BLOCK["H"]) and y.dtype == dtype
    err = rel_err(y, _float64_block(x, gu, gu_state, dn, dn_state, ids, w, bgu, bdn))
    print(f"batched block {dtype} T={T}: relative error {err:.3e} (bar {PARITY_BAR})")
    assert err <= PARITY_BAR


def test_captured_batched_block_follows_ids_and_weights():
    bnb = _bnb()
    E, H, S, T = BLOCK["E"], BLOCK["H"], BLOCK["S"], 40
    gu, gu_state, dn, dn_state, bgu, bdn = _block(torch.bfloat16)
    x = torch.randn(T, H, generator=torch.Generator().manual_seed(51)).bfloat16().to(DEV)
    sets = [_routing(T, S, E, 52 + k) for k in range(4)]
    call = lambda i, w: bnb.moe_ffn_4bit_batched(x, gu, gu_state, dn, dn_state, i, w, gate_up_bias=bgu, down_bias=bdn)
    eager = [call(i, w) for i, w in sets]
    assert not torch.equal(eager[1], eager[2])
    ids_buf, w_buf = sets[0][0].clone(), sets[0][1].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
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


def test_isolation_and_bounds():
    """A NaN absmax on every unselected expert changes no bit; nothing around a [P, I] in the middle of a NaN-filled buffer is touched."""
    bnb = _bnb()
    E, I, H = BLOCK["E"], BLOCK["I"], BLOCK["H"]
    gu, gu_state, _, _, bgu, _ = _block(torch.bfloat16, False, "fp4")
    x = torch.randn(4, H, generator=torch.Generator().manual_seed(71)).bfloat16().to(DEV)
    ids = torch.tensor([[1, 4], [4, 1], [1, -1], [E, 4]], dtype=torch.int32, device=DEV)
    clean = bnb.matmul_4bit_experts_batched(x, gu, gu_state, ids, bias=bgu, gated="chunked")
    assert clean.shape == (4, 2, I) and torch.isfinite(clean).all() and float(clean[0].abs().max()) > 0
    assert bool((clean[2, 1] == 0).all()) and bool((clean[3, 0] == 0).all())
    poisoned = copy.deepcopy(gu_state)
    poisoned.absmax.view(E, -1)[[0, 2, 3, 5]] = float("nan")
    assert torch.equal(bnb.matmul_4bit_experts_batched(x, gu, poisoned, ids, bias=bgu, gated="chunked"), clean)
    band, n = 4096, 4 * 2 * I
    buf = torch.full((band + n + band,), float("nan"), dtype=torch.bfloat16, device=DEV)
    from bitsandbytes_amd.cextension import ExpertsMfmaArgs as A
    args = A(ct.sizeof(A), 2, 1, gu_state.blocksize, 4, 1, 0, 2, E, 2 * I, H, 8, 0, x.data_ptr(), gu.data_ptr(), gu_state.absmax.data_ptr(), None,
             None, None, bgu.data_ptr(), ids.data_ptr(), None, buf[band:].data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert bnb.lib.bnb_mi355x_gemm_4bit_experts_mfma(ct.byref(args)) == 0
    torch.cuda.synchronize()
    assert torch.equal(buf[band:band + n].view(4, 2, I), clean)
    assert bool(buf[:band].isnan().all()) and bool(buf[band + n:].isnan().all())


def test_opcheck_and_error_paths():
    bnb = _bnb()
    E, N, K = 4, 96, 256
    x = torch.randn(3, 2, K, device=DEV).bfloat16()
    ids = torch.randint(0, E, (3, 2), device=DEV)
    bias = torch.randn(E, N, device=DEV).bfloat16()
    for nested in (False, True):
        packed, state = _quantize(_random_stack(E, N, K, torch.bfloat16, 81), nested, "nf4")
        kwargs = dict(bias=bias, absmax_8bit=state.absmax, absmax_code=state.state2.code, absmax_offset=state.offset) if nested else dict(bias=bias)
        args = (x, packed, [E, N, K], state.state2.absmax if nested else state.absmax, ids, 64, "nf4")
        for extra in (dict(), dict(gated="chunked"), dict(gated="interleaved"), dict(row_scale=torch.rand(3, 2, device=DEV))):
            torch.library.opcheck(_op(), args, {**kwargs, **extra}, test_utils=("test_schema", "test_faketensor"))
    assert bnb.matmul_4bit_experts_batched(x[:0], packed, state, ids[:0], gated="chunked").shape == (0, 2, N // 2)
    # declined: fp32, blocksize 32, gated together with row_scale, inputs that require grad
    p32, s32 = _quantize(_random_stack(E, N, K, torch.bfloat16, 82), False, "nf4", bs=32)
    with pytest.raises(ValueError, match="no kernel"):
        bnb.matmul_4bit_experts_batched(x.float(), packed, state, ids)
    with pytest.raises(ValueError, match="no kernel"):
        bnb.matmul_4bit_experts_batched(x, p32, s32, ids)
    with pytest.raises(ValueError, match="together"):
        bnb.matmul_4bit_experts_batched(x, packed, state, ids, gated="chunked", row_scale=torch.rand(3, 2, device=DEV))
    with pytest.raises(RuntimeError, match="inference only"):
        bnb.matmul_4bit_experts_batched(x.clone().requires_grad_(), packed, state, ids)
    # the block where the predicate declines both stages (fp32): moe_ffn_4bit's launches and bits
    gu, gu_state, dn, dn_state, bgu, bdn = _block(torch.float32)
    ids2, w2 = _routing(5, BLOCK["S"], BLOCK["E"], 91)
    xf = torch.randn(5, BLOCK["H"], device=DEV)
    y = bnb.moe_ffn_4bit_batched(xf, gu, gu_state, dn, dn_state, ids2, w2, gate_up_bias=bgu, down_bias=bdn)
    assert bnb.lib.bnb_mi355x_last_gemm_kernel() == 9
    assert torch.equal(y, bnb.moe_ffn_4bit(xf, gu, gu_state, dn, dn_state, ids2, w2, gate_up_bias=bgu, down_bias=bdn))
    # the parametrize helper's keyword
    from bitsandbytes_amd.nn import parametrize as bp
    gu, gu_state, dn, dn_state, bgu, bdn = _block(torch.bfloat16)
    xb = xf.bfloat16()
    y = bp.moe_ffn_4bit(_experts_module(), "gate_up_proj", "down_proj", xb, ids2, w2, gate_up_bias=bgu, down_bias=bdn, combine="batched")
    assert bnb.lib.bnb_mi355x_last_gemm_kernel() == K_MFMA and not torch.equal(y, torch.zeros_like(y))
    assert torch.equal(y, bnb.moe_ffn_4bit_batched(xb, gu, gu_state, dn, dn_state, ids2, w2, gate_up_bias=bgu, down_bias=bdn))
