"""GPU: the token-major MoE gate / up projection with gated SiLU in the launch (csrc/gemm4_experts_gate_up.hip) and the block
``moe_ffn_4bit_tokens``. Exact: on the operands of tests/moe_gate_up_cases.py (premise: tests/test_moe_gate_up_host.py) the output is
torch's ``F.silu(g) * u`` on the two float64 products rounded once, bit for bit."""
import copy
import ctypes as ct

import pytest
import torch
import torch.nn.functional as TF

import exact_inputs as X
import moe_gate_up_cases as C
from conftest import rel_err
from test_gpu_moe_combine import K_COMBINE, _float64_block
from test_gpu_moe_ffn import BLOCK, _block, _bnb, _experts_module, _gated_operands, _prepared, _quantize, _random_stack, _routing

pytestmark = pytest.mark.gpu

DEV = "cuda"
K_GATE_UP = 11

_op = lambda: torch.ops.bitsandbytes_amd.gemm_4bit_experts_gate_up.default


@pytest.mark.parametrize("cu_count", C.CU_COUNTS, ids=lambda c: f"cus{c}")
@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.name)
def test_exact_for_every_id_pattern(case, cu_count, request):
    lib = _bnb().lib
    lib.bnb_mi355x_set_cu_count(cu_count)
    request.addfinalizer(lambda: lib.bnb_mi355x_set_cu_count(0))
    E, N, K = case.E, case.N, case.K
    d = _prepared(case)
    _, a8, code, off = d["stats"]
    failures, calls, tiles = [], 0, set()
    for T, S in C.TS:
        x = d["x"][:T]
        tok = torch.arange(T, device=DEV)[:, None]
        plan = (ct.c_int * 4)()
        assert lib.bnb_mi355x_gemm_4bit_experts_gate_up_plan(T, S, N, K, plan) == 1
        tiles.add((plan[3], 64 // plan[0]))
        assert cu_count != 1 or 2 * plan[3] >= 5 * (64 // plan[0]), list(plan)   # several row groups per tile
        for pattern in C.ID_PATTERNS:
            ids64 = C.make_ids(pattern, T, S, E).to(DEV)
            valid = ((ids64 >= 0) & (ids64 < E)).unsqueeze(-1)
            safe = ids64.clamp(0, E - 1)
            for layout in ("chunked", "interleaved"):
                packed, absmax, bias, g64, u64, bg, bu = _gated_operands(case, d, layout)
                for with_bias in (False, True):
                    g = g64[safe, tok] + (bg.double()[safe] if with_bias else 0.0)             # [T, S, I]
                    u = u64[safe, tok] + (bu.double()[safe] if with_bias else 0.0)
                    want = TF.silu(g.to(case.dtype)) * u.to(case.dtype)                       # torch's kernels on T-valued tensors
                    want = torch.where(valid, want, torch.zeros_like(want))
                    for idt in (torch.int32, torch.int64):
                        y = _op()(x, packed, [E, N, K], absmax, ids64.to(idt), case.blocksize, "fp4", bias if with_bias else None, a8, code,
                                  off, layout)
                        calls += 1
                        assert lib.bnb_mi355x_last_gemm_kernel() == K_GATE_UP and y.shape == (T, S, N // 2) and y.dtype == case.dtype
                        if not torch.equal(y, want):
                            failures.append((T, S, pattern, layout, with_bias, idt, X.first_mismatch(y.view(T * S, -1).cpu(), want.view(T * S, -1).cpu())))
    print(f"{case.name}: {calls} calls, {len(failures)} not bit-equal; (tile columns, rows per group) {sorted(tiles)}")
    assert calls and not failures, f"{len(failures)} of {calls} calls differ; first: {failures[:5]}"


@pytest.mark.parametrize("T", [1, 5])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32], ids=["bf16", "fp16", "fp32"])
def test_tokens_block_on_ordinary_data(dtype, T, monkeypatch):
    """NF4, nested, against the float64 block: in 16 bits 1.5 x the error of ``moe_ffn_4bit``, in fp32 1e-5 (test_gpu_moe_combine.py)."""
    bnb = _bnb()
    import bitsandbytes_amd.autograd._functions as AF

    families, real = [], AF.matmul_4bit_experts_gate_up
    monkeypatch.setattr(AF, "matmul_4bit_experts_gate_up", lambda *a, **k: (real(*a, **k), families.append(bnb.lib.bnb_mi355x_last_gemm_kernel()))[0])
    ids, w = _routing(T, BLOCK["S"], BLOCK["E"], 40 + T)
    x = torch.randn(T, BLOCK["H"], generator=torch.Generator().manual_seed(41)).to(dtype).to(DEV)
    gu, gu_state, dn, dn_state, bgu, bdn = _block(dtype)
    base = bnb.moe_ffn_4bit(x, gu, gu_state, dn, dn_state, ids, w, gate_up_bias=bgu, down_bias=bdn)
    y = bnb.moe_ffn_4bit_tokens(x, gu, gu_state, dn, dn_state, ids, w, gate_up_bias=bgu, down_bias=bdn)
    assert families == [K_GATE_UP] and bnb.lib.bnb_mi355x_last_gemm_kernel() == K_COMBINE
    assert y.shape == (T, BLOCK["H"]) and y.dtype == dtype
    ref = _float64_block(x, gu, gu_state, dn, dn_state, ids, w, bgu, bdn)
    err_tokens, err_sum = rel_err(y, ref), rel_err(base, ref)
    print(f"block {dtype} T={T}: relative error tokens {err_tokens:.3e}, moe_ffn_4bit {err_sum:.3e}")
    assert err_tokens <= (1e-5 if dtype == torch.float32 else 1.5 * err_sum)


def test_captured_tokens_block_follows_ids_and_weights():
    bnb = _bnb()
    E, H, S, T = BLOCK["E"], BLOCK["H"], BLOCK["S"], 5
    gu, gu_state, dn, dn_state, bgu, bdn = _block(torch.bfloat16)
    x = torch.randn(T, H, generator=torch.Generator().manual_seed(51)).bfloat16().to(DEV)
    sets = [_routing(T, S, E, 52 + k) for k in range(4)]
    call = lambda i, w: bnb.moe_ffn_4bit_tokens(x, gu, gu_state, dn, dn_state, i, w, gate_up_bias=bgu, down_bias=bdn)
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
    """A NaN absmax on every unselected expert changes no bit; nothing around a [T, S, I] in the middle of a NaN-filled buffer is touched."""
    bnb = _bnb()
    E, I, H = BLOCK["E"], BLOCK["I"], BLOCK["H"]
    gu, gu_state, _, _, bgu, _ = _block(torch.bfloat16, False, "fp4")
    x = torch.randn(4, H, generator=torch.Generator().manual_seed(71)).bfloat16().to(DEV)
    ids = torch.tensor([[1, 4], [4, 1], [1, -1], [E, 4]], dtype=torch.int32, device=DEV)
    clean = bnb.matmul_4bit_experts_gate_up(x, gu, gu_state, ids, bias=bgu)
    assert clean.shape == (4, 2, I) and torch.isfinite(clean).all() and float(clean[0].abs().max()) > 0
    assert bool((clean[2, 1] == 0).all()) and bool((clean[3, 0] == 0).all())
    poisoned = copy.deepcopy(gu_state)
    poisoned.absmax.view(E, -1)[[0, 2, 3, 5]] = float("nan")
    assert torch.equal(bnb.matmul_4bit_experts_gate_up(x, gu, poisoned, ids, bias=bgu), clean)
    band, n = 4096, 4 * 2 * I
    buf = torch.full((band + n + band,), float("nan"), dtype=torch.bfloat16, device=DEV)
    from bitsandbytes_amd.cextension import ExpertsGateUpArgs as A
    args = A(ct.sizeof(A), 2, 1, gu_state.blocksize, 4, 1, 2, E, 2 * I, H, 4, x.data_ptr(), gu.data_ptr(), gu_state.absmax.data_ptr(), None, None,
             None, bgu.data_ptr(), ids.data_ptr(), buf[band:].data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert bnb.lib.bnb_mi355x_gemm_4bit_experts_gate_up(ct.byref(args)) == 0
    torch.cuda.synchronize()
    assert torch.equal(buf[band:band + n].view(4, 2, I), clean)
    assert bool(buf[:band].isnan().all()) and bool(buf[band + n:].isnan().all())


def test_opcheck_and_error_paths():
    bnb = _bnb()
    E, N, K = 4, 96, 256
    x = torch.randn(3, K, device=DEV).bfloat16()
    ids = torch.randint(0, E, (3, 2), device=DEV)
    bias = torch.randn(E, N, device=DEV).bfloat16()
    for nested in (False, True):
        packed, state = _quantize(_random_stack(E, N, K, torch.bfloat16, 81), nested, "nf4")
        kwargs = dict(bias=bias, absmax_8bit=state.absmax, absmax_code=state.state2.code, absmax_offset=state.offset) if nested else dict(bias=bias)
        args = (x, packed, [E, N, K], state.state2.absmax if nested else state.absmax, ids, 64, "nf4")
        for gated in ("chunked", "interleaved"):
            torch.library.opcheck(_op(), args, dict(kwargs, gated=gated), test_utils=("test_schema", "test_faketensor"))
    assert bnb.matmul_4bit_experts_gate_up(x[:0], packed, state, ids[:0]).shape == (0, 2, N // 2)
    # a declined geometry (S = 17): an error from the function, moe_ffn_4bit_fused's bits from the block
    gu, gu_state, dn, dn_state, bgu, bdn = _block(torch.bfloat16)
    ids17, w17 = _routing(2, 17, BLOCK["E"], 90)
    xb = torch.randn(2, BLOCK["H"], device=DEV).bfloat16()
    with pytest.raises(ValueError, match="no kernel"):
        bnb.matmul_4bit_experts_gate_up(xb, gu, gu_state, ids17)
    tokens = bnb.moe_ffn_4bit_tokens(xb, gu, gu_state, dn, dn_state, ids17, w17, gate_up_bias=bgu, down_bias=bdn)
    assert bnb.lib.bnb_mi355x_last_gemm_kernel() not in (K_GATE_UP, K_COMBINE)
    assert torch.equal(tokens, bnb.moe_ffn_4bit_fused(xb, gu, gu_state, dn, dn_state, ids17, w17, gate_up_bias=bgu, down_bias=bdn))
    # the parametrize helper's keyword: "tokens" is moe_ffn_4bit_tokens on the module's packed stacks, anything else an error
    from bitsandbytes_amd.nn import parametrize as bp
    m = _experts_module()
    ids2, w2 = _routing(2, 2, BLOCK["E"], 91)
    y = bp.moe_ffn_4bit(m, "gate_up_proj", "down_proj", xb, ids2, w2, gate_up_bias=bgu, down_bias=bdn, combine="tokens")
    assert torch.equal(y, bnb.moe_ffn_4bit_tokens(xb, gu, gu_state, dn, dn_state, ids2, w2, gate_up_bias=bgu, down_bias=bdn))
    assert not torch.equal(y, torch.zeros_like(y))
    with pytest.raises(ValueError, match="combine"):
        bp.moe_ffn_4bit(m, "gate_up_proj", "down_proj", xb, ids2, w2, combine="x")
