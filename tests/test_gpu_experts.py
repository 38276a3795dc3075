"""GPU: the expert-indexed fused matmul (bitsandbytes_amd::gemm_4bit_experts, csrc/gemm4_experts.hip).

* exact: on the operands of tests/exact_inputs.py (the stack is ``build(E * N, K, ...)`` viewed as ``[E, N, K]``) every ``y[t, s, :]``
  equals the float64 product of the constructed operands, rounded once - bit for bit, no tolerance - for both forms of ``x``, both
  id dtypes, P in {1, 2, 5, 16, 64, 65, 200} and five id patterns, with and without bias. The preconditions are asserted on the CPU
  by tests/test_experts_host.py.
* properties on ordinary NF4 / FP4 data: parity with the oracle, determinism, isolation, graph capture, opcheck, the parametrize
  helper.
"""
import ctypes as ct

import pytest
import torch

import exact_inputs as X
import experts_cases as C
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
    return torch.ops.bitsandbytes_amd.gemm_4bit_experts.default


# ------------------------------------------------------------------------------------------ exact
@pytest.mark.parametrize("case", C.EXACT_CASES, ids=lambda c: c.name)
def test_exact_for_every_id_pattern(case):
    lib = _bnb().lib
    E, N, K = case.E, case.N, case.K
    ex = C.build_case(case)
    packed = X.check_quantization(ex, gpu_ops(), DEV)   # one quantize_4bit over the contiguous stack
    absmax, a8, code, off = ex.stats_args(DEV)
    x_all = ex.x.to(DEV)
    bias = ex.bias.view(E, N).to(DEV)
    W = ex.W.to(DEV).view(E, N, K)
    # float64 products of every activation row with every expert (exact: integers times multiples of the unit, far below 2^53)
    x64 = x_all.double()
    y64 = torch.stack([x64 @ W[e].double().t() for e in range(E)])        # [E, rows, N]
    del W
    bias64 = bias.double()
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
            for per_slot in (False, True):
                x = x_all[:P].view(T, S, K) if per_slot else x_all[:T]
                xrow = pair if per_slot else pair // S
                want0 = y64[safe, xrow]                                    # [P, N]
                for with_bias in (False, True):
                    want = ((want0 + bias64[safe]) if with_bias else want0).to(case.dtype)
                    want = torch.where(valid[:, None], want, torch.zeros_like(want))   # ids that name no expert: zeros, no bias
                    for idt in (torch.int32, torch.int64):
                        ids = ids64.to(idt).view(T, S)
                        y = _op()(x, packed, [E, N, K], absmax, ids, case.blocksize, "fp4", bias if with_bias else None, a8, code, off)
                        calls += 1
                        assert lib.bnb_mi355x_last_gemm_kernel() == K_EXPERTS
                        assert y.shape == (T, S, N) and y.dtype == case.dtype
                        y = y.view(P, N)
                        if not torch.equal(y, want):
                            r, c, got, exp = X.first_mismatch(y.cpu(), want.cpu())
                            failures.append(f"P={P} {pattern} x={'TSK' if per_slot else 'TK'} bias={int(with_bias)} {idt}: pair {r} "
                                            f"(id {int(ids_cpu[r])}) column {c}: got {got!r}, want {exp!r}")
    print(f"{case.name}: {calls} calls, {len(failures)} not bit-equal")
    assert not failures, f"{len(failures)} of {calls} calls differ; first: {failures[:5]}"


# ------------------------------------------------------------------------------------------ ordinary data
def _stack(E, N, K, dtype, nested, qt, bs=64, seed=0):
    F = _bnb().functional
    gen = torch.Generator().manual_seed(seed)
    W = (torch.randn(E, N, K, generator=gen) / K ** 0.5).to(dtype).to(DEV)
    packed, state = F.quantize_4bit(W, blocksize=bs, compress_statistics=nested, quant_type=qt)
    return W, packed, state


def _unnested_absmax(state) -> torch.Tensor:
    """fp32 absmax of every block on the CPU: what the nested reconstruction gives (two roundings)."""
    from oracle import oracle as O

    if not state.nested:
        return state.absmax.float().cpu()
    s2 = state.state2
    am = O.dequantize_blockwise(state.absmax.cpu(), s2.absmax.cpu(), s2.code.cpu(), 256, torch.float32)
    return (am + state.offset.cpu()).float()


PROPERTY_SHAPES = [
    (8, 320, 4096, torch.bfloat16, False, "nf4"),
    (8, 320, 4096, torch.bfloat16, True, "fp4"),
    (6, 200, 2560, torch.float16, True, "nf4"),
    (6, 200, 2560, torch.float32, False, "fp4"),
]
_ids = lambda v: "-".join(str(x).replace("torch.", "") for x in v)


@pytest.mark.parametrize("shape", PROPERTY_SHAPES, ids=_ids)
def test_parity_with_the_oracle_per_pair(shape):
    """Each pair's row against the oracle's gemm_4bit on that expert's slice (un-nested statistics: the oracle takes one matrix),
    at the bar of the dense fused matmuls (1e-2 relative). Observed on MI355X, worst pair: bf16 2.2e-3 (NF4) / 2.6e-3 (FP4, nested),
    fp16 3.5e-4, fp32 8.7e-8."""
    from oracle import oracle as O

    bnb = _bnb()
    E, N, K, dtype, nested, qt = shape
    _, packed, state = _stack(E, N, K, dtype, nested, qt)
    T, S = 6, 3
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(T, S, K, generator=gen).to(dtype)
    bias = torch.randn(E, N, generator=gen).to(dtype)
    ids = torch.randint(0, E, (T, S), generator=gen)
    y = bnb.matmul_4bit_experts(x.to(DEV), packed, state, ids.to(DEV), bias=bias.to(DEV)).cpu()
    am = _unnested_absmax(state).view(E, -1)
    pk = packed.cpu().view(E, -1)
    worst = 0.0
    for t in range(T):
        for s in range(S):
            e = int(ids[t, s])
            ref = O.gemm_4bit(x[t, s:s + 1], pk[e].reshape(-1, 1), (N, K), am[e], state.blocksize, qt, bias[e])[0]
            worst = max(worst, rel_err(y[t, s:s + 1], ref))
    print(f"parity {_ids(shape)}: worst per-pair relative error {worst:.3e} (bar {PARITY_BAR})")
    assert worst <= PARITY_BAR


@pytest.mark.parametrize("shape", PROPERTY_SHAPES[:2], ids=_ids)
def test_deterministic_and_order_free(shape):
    bnb = _bnb()
    E, N, K, dtype, nested, qt = shape
    _, packed, state = _stack(E, N, K, dtype, nested, qt)
    gen = torch.Generator().manual_seed(2)
    P = 64
    x = torch.randn(P, 1, K, generator=gen).to(dtype).to(DEV)
    ids = torch.randint(0, E, (P, 1), generator=gen).to(DEV)
    bias = torch.randn(E, N, generator=gen).to(dtype).to(DEV)
    y1 = bnb.matmul_4bit_experts(x, packed, state, ids, bias=bias)
    y2 = bnb.matmul_4bit_experts(x, packed, state, ids, bias=bias)
    assert torch.equal(y1, y2), "the same call twice"
    perm = torch.randperm(P, generator=gen).to(DEV)
    yp = bnb.matmul_4bit_experts(x[perm], packed, state, ids[perm], bias=bias)
    assert torch.equal(yp, y1[perm]), "permuting the pairs permutes the rows"
    for p in (0, 17, 63):
        alone = bnb.matmul_4bit_experts(x[p:p + 1], packed, state, ids[p:p + 1], bias=bias)
        assert torch.equal(alone[0], y1[p]), f"pair {p} alone against one of 64"


@pytest.mark.parametrize("nested", [False, True], ids=["plain", "nested"])
def test_unselected_experts_are_not_read_and_the_output_is_fully_written(nested):
    bnb = _bnb()
    lib = bnb.lib
    E, N, K, bs = 8, 320, 4096, 64
    dtype = torch.bfloat16
    _, packed, state = _stack(E, N, K, dtype, nested, "nf4")
    gen = torch.Generator().manual_seed(3)
    T, S = 5, 2
    x = torch.randn(T, K, generator=gen).to(dtype).to(DEV)
    ids = torch.tensor([[1, 6], [6, 1], [1, 1], [6, -1], [E, 6]], dtype=torch.int32, device=DEV)
    clean = bnb.matmul_4bit_experts(x, packed, state, ids)
    assert torch.isfinite(clean).all()
    # statistics of every expert nobody selected: NaN (nested: the second-level absmax of the groups of 256 blocks that lie wholly
    # inside such experts - the 8-bit codes and their table are shared with the selected ones)
    import copy

    poisoned = copy.deepcopy(state)
    bpe = N * K // bs
    selected = (1, 6)
    if nested:
        groups = poisoned.state2.absmax
        for g in range(groups.numel()):
            owners = {b // bpe for b in (g * 256, min(g * 256 + 255, E * bpe - 1))}
            if not owners & set(selected):
                groups[g] = float("nan")
        assert torch.isnan(groups).any()
    else:
        am = poisoned.absmax.view(E, bpe)
        for e in range(E):
            if e not in selected:
                am[e] = float("nan")
    y = bnb.matmul_4bit_experts(x, packed, poisoned, ids)
    assert torch.isfinite(y).all() and torch.equal(y, clean)
    assert bool((y[3, 1] == 0).all()) and bool((y[4, 0] == 0).all())
    # the C entry point into a NaN-filled buffer: every element is overwritten
    out = torch.full((T, S, N), float("nan"), dtype=dtype, device=DEV)
    vp = lambda t: None if t is None else ct.c_void_p(t.data_ptr())
    if nested:
        stats = (state.state2.absmax, state.absmax, state.state2.code.float(), state.offset.float())
    else:
        stats = (state.absmax, None, None, None)
    lib.bnb_mi355x_gemm_4bit_experts(2, vp(x), 0, vp(packed), vp(stats[0]), vp(stats[1]), vp(stats[2]), vp(stats[3]), None, vp(ids), 4,
                                     vp(out), T * S, S, E, N, K, bs, 2, ct.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert not torch.isnan(out).any() and torch.equal(out, clean)


def test_captured_call_follows_the_ids_buffer():
    """One torch.cuda.graph (single stream), replayed with the ids rewritten in place: the host never read them."""
    bnb = _bnb()
    E, N, K = 8, 320, 4096
    dtype = torch.bfloat16
    _, packed, state = _stack(E, N, K, dtype, True, "nf4")
    gen = torch.Generator().manual_seed(4)
    T, S = 4, 2
    x = torch.randn(T, K, generator=gen).to(dtype).to(DEV)
    id_sets = [torch.randint(-1, E + 1, (T, S), generator=gen).to(DEV) for _ in range(4)]
    eager = [bnb.matmul_4bit_experts(x, packed, state, i) for i in id_sets]
    assert not torch.equal(eager[1], eager[2])
    ids_buf = id_sets[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            bnb.matmul_4bit_experts(x, packed, state, ids_buf)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = bnb.matmul_4bit_experts(x, packed, state, ids_buf)
    for k in (1, 2, 3):
        ids_buf.copy_(id_sets[k])
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(y, eager[k]), f"replay {k} did not follow the ids"


def test_opcheck_and_empty_call():
    bnb = _bnb()
    E, N, K = 4, 96, 256
    for nested in (False, True):
        _, packed, state = _stack(E, N, K, torch.bfloat16, nested, "nf4")
        x = torch.randn(3, 2, K, device=DEV).bfloat16()
        ids = torch.randint(0, E, (3, 2), device=DEV)
        bias = torch.randn(E, N, device=DEV).bfloat16()
        if nested:
            args = (x, packed, [E, N, K], state.state2.absmax, ids, 64, "nf4")
            kwargs = dict(bias=bias, absmax_8bit=state.absmax, absmax_code=state.state2.code, absmax_offset=state.offset)
        else:
            args = (x, packed, [E, N, K], state.absmax, ids, 64, "nf4")
            kwargs = dict(bias=bias)
        torch.library.opcheck(_op(), args, kwargs, test_utils=("test_schema", "test_faketensor"))
    # P = 0: an empty tensor, no launch (the family of the last launch stays the dense call's)
    torch.ops.bitsandbytes.gemm_4bit.default(x[0, :1], packed.view(E, -1)[0].reshape(-1, 1), [N, K],
                                             _unnested_absmax(state).view(E, -1)[0].to(DEV), 64, "nf4")
    before = bnb.lib.bnb_mi355x_last_gemm_kernel()
    assert before != K_EXPERTS
    y = bnb.matmul_4bit_experts(x[:0], packed, state, ids[:0])
    assert y.shape == (0, 2, N) and bnb.lib.bnb_mi355x_last_gemm_kernel() == before
    # flat ids
    y = bnb.matmul_4bit_experts(x.view(6, K), packed, state, ids.view(6))
    assert y.shape == (6, N) and torch.equal(y, bnb.matmul_4bit_experts(x, packed, state, ids).view(6, N))


def test_op_errors():
    bnb = _bnb()
    _, packed, state = _stack(2, 32, 256, torch.bfloat16, False, "nf4")
    x = torch.randn(3, 256, device=DEV).bfloat16()
    ids = torch.zeros((3, 1), dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError, match="inference only"):
        bnb.matmul_4bit_experts(x.clone().requires_grad_(), packed, state, ids)
    # a geometry that passes the argument checks and that the kernel does not serve: a ValueError, never another path
    Kbig = 1 << 18
    Wb = torch.randn(1, 32, Kbig, device=DEV).bfloat16()
    pb, sb = bnb.functional.quantize_4bit(Wb, blocksize=64, quant_type="nf4")
    with pytest.raises(ValueError, match="no kernel"):
        bnb.matmul_4bit_experts(torch.randn(1, Kbig, device=DEV).bfloat16(), pb, sb, ids[:1])


def test_parametrize_helper():
    import torch.nn.utils.parametrize as P

    bnb = _bnb()
    from bitsandbytes_amd.nn import parametrize as bp

    E, N, K = 8, 256, 2048
    gen = torch.Generator().manual_seed(6)

    class Experts(torch.nn.Module):
        def __init__(self, e, n, k):
            super().__init__()
            self.w = torch.nn.Parameter((torch.randn(e, n, k, generator=gen) / k ** 0.5).bfloat16().to(DEV))

    m = Experts(E, N, K)
    bp.replace_parameter_4bit(m, "w", compress_statistics=True, quant_type="nf4")
    x = torch.randn(5, K, generator=gen).bfloat16().to(DEV)
    ids = torch.tensor([[0, 7], [3, 3], [-1, 2], [5, E], [1, 6]], device=DEV)
    P._cache.clear()
    y = bp.matmul_4bit_experts(m, "w", x, ids)
    assert bnb.lib.bnb_mi355x_last_gemm_kernel() == K_EXPERTS
    assert len(P._cache) == 0 and y.shape == (5, 2, N)
    W = getattr(m, "w")
    valid = ((ids >= 0) & (ids < E))[..., None]
    ref = torch.matmul(W[ids.clamp(0, E - 1)].float(), x.float()[:, None, :, None]).squeeze(-1) * valid
    err = rel_err(y, ref)
    print(f"parametrize helper against indexed matmul: relative error {err:.3e}")
    assert err <= PARITY_BAR and bool((y[2, 0] == 0).all()) and bool((y[3, 1] == 0).all())
    # a geometry the kernel does not serve (K % blocksize != 0): the dequantized attribute, indexed - same convention
    m2 = Experts(4, 32, 96)
    bp.replace_parameter_4bit(m2, "w", quant_type="nf4", blocksize=64)
    x2 = torch.randn(3, 2, 96, generator=gen).bfloat16().to(DEV)
    ids2 = torch.tensor([[0, 3], [4, 1], [-1, 2]], device=DEV)
    y2 = bp.matmul_4bit_experts(m2, "w", x2, ids2)
    W2 = getattr(m2, "w")
    ref2 = torch.matmul(W2[ids2.clamp(0, 3)].float(), x2.float()[..., None]).squeeze(-1) * ((ids2 >= 0) & (ids2 < 4))[..., None]
    assert y2.shape == (3, 2, 32) and rel_err(y2, ref2) <= PARITY_BAR and bool((y2[1, 0] == 0).all())
