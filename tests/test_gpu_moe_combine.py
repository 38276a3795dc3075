"""GPU: the token-major MoE down projection with the slot sum in the launch (csrc/gemm4_experts_combine.hip). Exact: on the operands of
tests/moe_combine_cases.py (premise: tests/test_moe_combine_host.py) the output is the float64 block rounded once, bit for bit."""
import copy
import ctypes as ct
import functools

import pytest
import torch
import torch.nn.functional as TF

import exact_inputs as X
import moe_combine_cases as C
from conftest import rel_err
from routed_sweep import gpu_ops
from test_gpu_moe_ffn import BLOCK, _block, _bnb, _experts_module, _quantize, _random_stack, _routing

pytestmark = pytest.mark.gpu

DEV = "cuda"
K_COMBINE = 10


_op = lambda: torch.ops.bitsandbytes_amd.gemm_4bit_experts_combine.default


@functools.lru_cache(maxsize=None)
def _prepared(case):
    ex = C.build_case(case)
    packed = X.check_quantization(ex, gpu_ops(), DEV)
    W = ex.W.to(DEV).view(case.E, case.N, case.K)
    x = ex.x.to(DEV)
    y64 = torch.stack([x.double() @ W[e].double().t() for e in range(case.E)])   # [E, rows, N]; exact (exact_inputs.py)
    return ex, packed, ex.stats_args(DEV), x, y64, ex.bias.view(case.E, case.N).to(DEV)


@pytest.mark.parametrize("cu_count", C.CU_COUNTS, ids=lambda c: f"cus{c}")
@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.name)
def test_exact_for_every_id_pattern(case, cu_count, request):
    lib = _bnb().lib
    lib.bnb_mi355x_set_cu_count(cu_count)
    request.addfinalizer(lambda: lib.bnb_mi355x_set_cu_count(0))
    E, N, K = case.E, case.N, case.K
    ex, packed, (absmax, a8, code, off), x, y64, bias = _prepared(case)
    failures, calls, tiles = [], 0, set()
    for T, S in C.ts_of(case, ex):
        h = x[:T * S].view(T, S, K)
        pair = torch.arange(T * S, device=DEV).view(T, S)
        w32 = C.weights(T, S).to(DEV)
        plan = (ct.c_int * 4)()
        assert lib.bnb_mi355x_gemm_4bit_experts_combine_plan(T, S, N, K, plan) == 1
        tiles.add((plan[3], 64 // plan[0]))
        assert cu_count != 1 or (plan[3] >= 20 and plan[3] >= 5 * (64 // plan[0])), list(plan)   # several row groups per tile
        for pattern in C.ID_PATTERNS:
            ids64 = C.make_ids(pattern, T, S, E).to(DEV)
            valid = (ids64 >= 0) & (ids64 < E)
            safe = ids64.clamp(0, E - 1)
            w_poisoned = torch.where(valid, w32, torch.full_like(w32, float("nan")))   # a NaN weight on every dropped slot
            for with_bias in (False, True):
                o = y64[safe, pair] + (bias.double()[safe] if with_bias else 0.0)          # [T, S, N]
                want = (o * (w32.double() * valid).unsqueeze(-1)).sum(dim=1).to(case.dtype)
                for idt in (torch.int32, torch.int64):
                    for wdt in (torch.float32, case.dtype):
                        y = _op()(h, packed, [E, N, K], absmax, ids64.to(idt), w_poisoned.to(wdt), case.blocksize, "fp4",
                                  bias if with_bias else None, a8, code, off)
                        calls += 1
                        assert lib.bnb_mi355x_last_gemm_kernel() == K_COMBINE and y.shape == (T, N) and y.dtype == case.dtype
                        if not torch.equal(y, want):
                            failures.append((T, S, pattern, with_bias, idt, wdt, X.first_mismatch(y.cpu(), want.cpu())))
    print(f"{case.name}: {calls} calls, {len(failures)} not bit-equal; (tile rows, rows per group) {sorted(tiles)}")
    assert calls and not failures, f"{len(failures)} of {calls} calls differ; first: {failures[:5]}"


def _float64_block(x, gu, gu_state, dn, dn_state, ids, w, bgu, bdn):
    """The float64 block from the dequantized weights (test_block_16bit_is_no_worse_than_the_parent_ops)."""
    F, E, I, H = _bnb().functional, BLOCK["E"], BLOCK["I"], BLOCK["H"]
    Wgu = F.dequantize_4bit(gu, gu_state).double().view(E, 2 * I, H)
    Wdn = F.dequantize_4bit(dn, dn_state).double().view(E, H, I)
    valid, safe = ((ids >= 0) & (ids < E)).double(), ids.clamp(0, E - 1)
    h = torch.einsum("tsnk,tk->tsn", Wgu[safe], x.double()) + bgu.double()[safe]
    a = TF.silu(h[..., :I]) * h[..., I:]
    o = torch.einsum("tshi,tsi->tsh", Wdn[safe], a) + bdn.double()[safe]
    return (o * (w.double() * valid).unsqueeze(-1)).sum(dim=1)


@pytest.mark.parametrize("T", [1, 5])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32], ids=["bf16", "fp16", "fp32"])
def test_fused_block_on_ordinary_data(dtype, T):
    """NF4, nested, against the float64 block: in 16 bits 1.5 x the error of ``moe_ffn_4bit`` (noise at T * 512 outputs), in fp32 1e-5."""
    bnb = _bnb()
    ids, w = _routing(T, BLOCK["S"], BLOCK["E"], 40 + T)
    x = torch.randn(T, BLOCK["H"], generator=torch.Generator().manual_seed(41)).to(dtype).to(DEV)
    gu, gu_state, dn, dn_state, bgu, bdn = _block(dtype)
    base = bnb.moe_ffn_4bit(x, gu, gu_state, dn, dn_state, ids, w, gate_up_bias=bgu, down_bias=bdn)
    assert bnb.lib.bnb_mi355x_last_gemm_kernel() != K_COMBINE
    y = bnb.moe_ffn_4bit_fused(x, gu, gu_state, dn, dn_state, ids, w, gate_up_bias=bgu, down_bias=bdn)
    assert bnb.lib.bnb_mi355x_last_gemm_kernel() == K_COMBINE and y.shape == (T, BLOCK["H"]) and y.dtype == dtype
    ref = _float64_block(x, gu, gu_state, dn, dn_state, ids, w, bgu, bdn)
    err_fused, err_sum = rel_err(y, ref), rel_err(base, ref)
    print(f"block {dtype} T={T}: relative error fused {err_fused:.3e}, moe_ffn_4bit {err_sum:.3e}")
    assert err_fused <= (1e-5 if dtype == torch.float32 else 1.5 * err_sum)


def test_captured_fused_block_follows_ids_and_weights():
    bnb = _bnb()
    E, H, S, T = BLOCK["E"], BLOCK["H"], BLOCK["S"], 5
    gu, gu_state, dn, dn_state, bgu, bdn = _block(torch.bfloat16)
    x = torch.randn(T, H, generator=torch.Generator().manual_seed(51)).bfloat16().to(DEV)
    sets = [_routing(T, S, E, 52 + k) for k in range(4)]
    call = lambda i, w: bnb.moe_ffn_4bit_fused(x, gu, gu_state, dn, dn_state, i, w, gate_up_bias=bgu, down_bias=bdn)
    eager = [call(i, w) for i, w in sets]
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
    """A NaN absmax on every unselected expert changes no bit; nothing around a [T, N] in the middle of a NaN-filled buffer is touched."""
    bnb = _bnb()
    E, I, H = BLOCK["E"], BLOCK["I"], BLOCK["H"]
    _, _, dn, dn_state, _, bdn = _block(torch.bfloat16, False, "fp4")
    h = torch.randn(4, 2, I, generator=torch.Generator().manual_seed(71)).bfloat16().to(DEV)
    ids = torch.tensor([[1, 4], [4, 1], [1, -1], [E, 4]], dtype=torch.int32, device=DEV)
    w = torch.tensor([[0.5, 0.5], [0.25, 0.75], [1.0, float("nan")], [float("nan"), 1.0]], device=DEV)
    clean = bnb.matmul_4bit_experts_combine(h, dn, dn_state, ids, w, bias=bdn)
    assert clean.shape == (4, H) and torch.isfinite(clean).all() and float(clean.abs().max()) > 0
    poisoned = copy.deepcopy(dn_state)
    poisoned.absmax.view(E, -1)[[0, 2, 3, 5]] = float("nan")
    assert torch.equal(bnb.matmul_4bit_experts_combine(h, dn, poisoned, ids, w, bias=bdn), clean)
    band = 4096
    buf = torch.full((band + 4 * H + band,), float("nan"), dtype=torch.bfloat16, device=DEV)
    from bitsandbytes_amd.cextension import ExpertsCombineArgs as A
    args = A(ct.sizeof(A), 2, 1, dn_state.blocksize, 4, 0, 2, E, H, I, 4, h.data_ptr(), dn.data_ptr(), dn_state.absmax.data_ptr(), None, None, None,
             bdn.data_ptr(), ids.data_ptr(), w.data_ptr(), buf[band:].data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert bnb.lib.bnb_mi355x_gemm_4bit_experts_combine(ct.byref(args)) == 0
    torch.cuda.synchronize()
    assert torch.equal(buf[band:band + 4 * H].view(4, H), clean)
    assert bool(buf[:band].isnan().all()) and bool(buf[band + 4 * H:].isnan().all())


def test_opcheck_and_error_paths():
    bnb = _bnb()
    E, N, K = 4, 96, 256
    x = torch.randn(3, 2, K, device=DEV).bfloat16()
    ids = torch.randint(0, E, (3, 2), device=DEV)
    w = torch.rand(3, 2, device=DEV)
    bias = torch.randn(E, N, device=DEV).bfloat16()
    for nested in (False, True):
        packed, state = _quantize(_random_stack(E, N, K, torch.bfloat16, 81), nested, "nf4")
        kwargs = dict(bias=bias, absmax_8bit=state.absmax, absmax_code=state.state2.code, absmax_offset=state.offset) if nested else dict(bias=bias)
        args = (x, packed, [E, N, K], state.state2.absmax if nested else state.absmax, ids, w, 64, "nf4")
        torch.library.opcheck(_op(), args, kwargs, test_utils=("test_schema", "test_faketensor"))
    assert bnb.matmul_4bit_experts_combine(x[:0], packed, state, ids[:0], w[:0]).shape == (0, N)
    # a declined geometry (S = 17): an error from the function, the "sum" path's bits from the block
    gu, gu_state, dn, dn_state, bgu, bdn = _block(torch.bfloat16)
    ids17, w17 = _routing(2, 17, BLOCK["E"], 90)
    h17 = torch.randn(2, 17, BLOCK["I"], device=DEV).bfloat16()
    with pytest.raises(ValueError, match="no kernel"):
        bnb.matmul_4bit_experts_combine(h17, dn, dn_state, ids17, w17)
    xb = torch.randn(2, BLOCK["H"], device=DEV).bfloat16()
    fused = bnb.moe_ffn_4bit_fused(xb, gu, gu_state, dn, dn_state, ids17, w17, gate_up_bias=bgu, down_bias=bdn)
    assert bnb.lib.bnb_mi355x_last_gemm_kernel() != K_COMBINE
    assert torch.equal(fused, bnb.moe_ffn_4bit(xb, gu, gu_state, dn, dn_state, ids17, w17, gate_up_bias=bgu, down_bias=bdn))
    # the parametrize helper's keyword: "fused" is moe_ffn_4bit_fused on the module's packed stacks, anything else an error
    from bitsandbytes_amd.nn import parametrize as bp
    m = _experts_module()
    ids2, w2 = _routing(2, 2, BLOCK["E"], 91)
    y = bp.moe_ffn_4bit(m, "gate_up_proj", "down_proj", xb, ids2, w2, gate_up_bias=bgu, down_bias=bdn, combine="fused")
    assert bnb.lib.bnb_mi355x_last_gemm_kernel() == K_COMBINE
    assert torch.equal(y, bnb.moe_ffn_4bit_fused(xb, gu, gu_state, dn, dn_state, ids2, w2, gate_up_bias=bgu, down_bias=bdn))
    with pytest.raises(ValueError, match="combine"):
        bp.moe_ffn_4bit(m, "gate_up_proj", "down_proj", xb, ids2, w2, combine="x")
