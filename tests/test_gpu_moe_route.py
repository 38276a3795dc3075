"""GPU: the MoE router's scoring + top-k launch (bitsandbytes_amd::moe_topk, csrc/moe_route.hip), ``bitsandbytes_amd.moe_topk`` /
``moe_route`` and ``nn.MoERouter``.

* ids: on the cases of tests/moe_route_cases.py (rankings unambiguous in float64 by construction, planted ties) the kernel's ids ARE
  the float64 ranking, ties to the lower index;
* weights: against float64 on the same logits, at most four times the error of torch's own fp32 composition on this GPU, with a
  floor of 2^-20 (moe_route_cases: WEIGHT_FACTOR, WEIGHT_FLOOR);
* a row's bits do not depend on the batch: every row of a 37-row call equals the 1-row call on that row;
* a NaN or +inf logit stays in its row, and that row's ids are the documented ranking (NaN keys last, by index);
* the C entry point between guard bands at a 1-element offset: bands and input untouched, every output byte written;
* graph replay of ``moe_route``; its logits are ``lora_shrink``'s; its outputs feed ``moe_ffn_4bit`` with no conversion.
The preconditions of the cases are asserted on the CPU by tests/test_moe_route_host.py.
"""
import ctypes as ct
import functools

import pytest
import torch

import guard_bands as GB
import moe_ffn_cases as FC
import moe_route_cases as C

pytestmark = pytest.mark.gpu

DEV = "cuda"
DT_CODE = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}


def _bnb():
    import bitsandbytes_amd as bnb

    return bnb


def _op():
    return torch.ops.bitsandbytes_amd.moe_topk.default


def _kernel(case, logits, bias):
    """The launch, through the op (no fall-back: the op raises where it has no kernel)."""
    return _op()(logits, case.S, case.scoring, case.renormalize, case.scale, bias)


@functools.lru_cache(maxsize=None)
def _result(case):
    """One case, once: (kernel ids, kernel weights, composition ids, composition weights), on the CPU."""
    from bitsandbytes_amd.autograd._functions import _moe_topk_composition

    b = C.build(case)
    logits = b.logits.to(DEV)
    bias = None if b.bias is None else b.bias.to(DEV)
    ids, w = _kernel(case, logits, bias)
    cids, cw = _moe_topk_composition(logits, case.S, case.scoring, case.renormalize, case.scale, bias)
    return ids.cpu(), w.cpu(), cids.cpu(), cw.cpu()


_CountedEntry = C.CountedEntry


# ------------------------------------------------------------------------------------------ ids and weights
@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.name)
def test_ids_are_the_float64_ranking(case):
    b = C.build(case)
    from bitsandbytes_amd.backends import hip

    ids, w, cids, _ = _result(case)
    assert ids.dtype == torch.int32 and w.dtype == torch.float32 and ids.shape == w.shape == (case.T, case.S)
    assert torch.equal(ids, b.ids), f"first differing row: {int((ids != b.ids).any(-1).nonzero()[0])}"
    assert torch.equal(cids, b.ids), "the torch composition on the GPU does not give the float64 ranking"
    # the public function takes the launch for these classes - one call of the C entry, not the composition - with the same bits
    assert hip.moe_topk_supported(case.dtype, case.T, case.E, case.S)
    with _CountedEntry() as entry:
        pids, pw = _bnb().moe_topk(b.logits.to(DEV), case.S, case.scoring, case.renormalize, case.scale, None if b.bias is None else b.bias.to(DEV))
    assert entry.calls == 1
    assert torch.equal(pids.cpu(), ids) and torch.equal(pw.cpu(), w)


def test_weights_within_four_times_the_composition_error():
    """Max relative error against float64 over every weight of every case: the kernel's at most WEIGHT_FACTOR x the torch fp32
    composition's on this GPU, floor WEIGHT_FLOOR."""
    res = {c: _result(c) for c in C.CASES}
    err_kernel = max(C.max_rel_err(res[c][1], C.build(c).weights) for c in C.CASES)
    err_torch = max(C.max_rel_err(res[c][3], C.build(c).weights) for c in C.CASES)
    bound = max(C.WEIGHT_FACTOR * err_torch, C.WEIGHT_FLOOR)
    print(f"moe_topk weights, max relative error against float64 over {len(C.CASES)} cases: kernel {err_kernel:.3e}, "
          f"torch fp32 composition {err_torch:.3e}, bound {bound:.3e}")
    assert all(bool(torch.isfinite(res[c][1]).all()) for c in C.CASES)
    assert err_kernel <= bound


# ------------------------------------------------------------------------------------------ rows do not see each other
T37 = [c for c in C.CASES if c.T == 37]


@pytest.mark.parametrize("case", T37, ids=lambda c: c.name)
def test_every_row_of_a_37_row_call_has_the_bits_of_its_own_call(case):
    """37 rows = nine full workgroups of four wavefronts and one with a single live wavefront: every wavefront position, a partly
    empty last workgroup."""
    b = C.build(case)
    logits = b.logits.to(DEV)
    bias = None if b.bias is None else b.bias.to(DEV)
    ids, w = _kernel(case, logits, bias)
    for t in range(case.T):
        i1, w1 = _kernel(case, logits[t:t + 1].contiguous(), bias)
        assert torch.equal(i1[0], ids[t]) and torch.equal(w1[0].view(torch.int32), w[t].view(torch.int32)), t
    assert len(T37) >= 3 and {c.scoring for c in T37} == set(C.SCORINGS)


@pytest.mark.parametrize("scoring", C.SCORINGS)
@pytest.mark.parametrize("poison", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_a_non_finite_logit_stays_in_its_row(scoring, poison):
    case = C.RouteCase(72, 8, 16, torch.float32, scoring, True, True)
    b = C.build(case)
    logits = b.logits.to(DEV)
    bias = b.bias.to(DEV)
    clean_ids, clean_w = _kernel(case, logits, bias)
    for row, col in ((5, 70), (15, 0)):   # (second register slot of lane 6; the first expert of the last row)
        dirty = logits.clone()
        dirty[row, col] = poison
        ids, w = _kernel(case, dirty, bias)
        others = [t for t in range(case.T) if t != row]
        assert torch.equal(ids[others], clean_ids[others])
        assert torch.equal(w[others].view(torch.int32), clean_w[others].view(torch.int32))
        got = ids[row].tolist()
        assert len(set(got)) == case.S and all(0 <= i < case.E for i in got), got
        # ... and they are the documented ranking: NaN keys last by index (a poisoned softmax row is all NaN: 0, 1, ..., S - 1)
        want_ids, _ = C.reference(dirty[row:row + 1].cpu(), case.S, scoring, True, case.scale, b.bias)
        assert got == want_ids[0].tolist(), (got, want_ids[0].tolist())
        if scoring == "sigmoid" and poison == float("inf"):   # sigmoid(+inf) = 1: an ordinary score, and the best one of its bias class
            assert bool(torch.isfinite(w[row]).all())


# ------------------------------------------------------------------------------------------ the C entry point between guard bands
@pytest.mark.parametrize("dtype", C.DTYPES, ids=lambda d: str(d).replace("torch.", ""))
@pytest.mark.parametrize("scoring", C.SCORINGS)
def test_entry_point_between_guard_bands(dtype, scoring):
    """bnb_mi355x_moe_topk on operands carved between guard bands, each ONE element past a 256-byte boundary; E = 60: lanes 60 ... 63
    hold no expert. The bands (NaN / -1 around the inputs) and the inputs are untouched; every output byte is written: the call on
    outputs pre-filled with 0xA5 and with 0x5A leaves the same bytes, the op's."""
    from bitsandbytes_amd.cextension import MoeTopkArgs

    lib = _bnb().lib
    case = C.RouteCase(60, 8, 5, dtype, scoring, True, True)
    b = C.build(case)
    es = b.logits.element_size()
    want_ids, want_w = _kernel(case, b.logits.to(DEV), b.bias.to(DEV))
    torch.cuda.synchronize()
    n = case.T * case.S
    seen = []
    for fill in (GB.PAT, 0x5A):
        lg = GB.carve_in(b.logits.to(DEV), None, fill=GB.NAN_PAT, off=es)
        sb = GB.carve_in(b.bias.to(DEV), None, fill=GB.NAN_PAT, off=4)
        ids = GB.carve_out(n * 4, None, 4, off=4, after=GB.after_band(16 * 16 * 4))
        ws = GB.carve_out(n * 4, None, 4, off=4, after=GB.after_band(16 * 16 * 4))
        ids.view.fill_(fill)
        ws.view.fill_(fill)
        assert lg.ptr() % 256 == es and ids.ptr() % 256 == 4 and ws.ptr() % 256 == 4 and sb.ptr() % 256 == 4
        before = (lg.bytes(), sb.bytes())
        args = MoeTopkArgs(ct.sizeof(MoeTopkArgs), DT_CODE[dtype], 0 if scoring == "softmax" else 1, 1, case.T, case.E, case.S, case.scale,
                           lg.ptr(), sb.ptr(), ids.ptr(), ws.ptr(), torch.cuda.current_stream().cuda_stream)
        assert lib.bnb_mi355x_moe_topk(ct.byref(args)) == 0
        torch.cuda.synchronize()
        for c in (lg, sb, ids, ws):
            assert c.guards_ok()
        assert torch.equal(lg.bytes(), before[0]) and torch.equal(sb.bytes(), before[1])
        seen.append((ids.bytes(), ws.bytes()))
        assert torch.equal(GB.read(ids, torch.int32, n).view(case.T, case.S), want_ids)
        assert torch.equal(GB.read(ws, torch.int32, n).view(case.T, case.S), want_w.view(torch.int32))
    assert torch.equal(seen[0][0], seen[1][0]) and torch.equal(seen[0][1], seen[1][1]), "an output byte kept its fill"
    assert torch.equal(want_ids.cpu(), b.ids)


def test_entry_point_refuses_on_the_device_too():
    """A refused call launches nothing: the outputs keep their fill."""
    from bitsandbytes_amd.cextension import MoeTopkArgs

    logits = torch.zeros(4, 64, device=DEV)
    ids = torch.full((4, 2), -7, dtype=torch.int32, device=DEV)
    w = torch.full((4, 2), -7.0, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    for over in (dict(struct_bytes=8), dict(experts=1025), dict(top_k=17), dict(scoring=2)):
        args = MoeTopkArgs(ct.sizeof(MoeTopkArgs), 0, 0, 1, 4, 64, 2, 1.0, logits.data_ptr(), None, ids.data_ptr(), w.data_ptr(), stream)
        for k, v in over.items():
            setattr(args, k, v)
        assert _bnb().lib.bnb_mi355x_moe_topk(ct.byref(args)) != 0
    torch.cuda.synchronize()
    assert bool((ids == -7).all()) and bool((w == -7.0).all())
    with pytest.raises(ValueError, match="no kernel"):
        _op()(torch.zeros(2, 1025, device=DEV), 2, "softmax", True, 1.0)


# ------------------------------------------------------------------------------------------ the whole router
def _router(E, K, dtype, seed):
    gen = torch.Generator().manual_seed(seed)
    W = (torch.randn(E, K, generator=gen) / K ** 0.5).to(dtype).to(DEV)
    xs = [torch.randn(16, K, generator=gen).to(dtype).to(DEV) for _ in range(3)]
    return W, xs


@pytest.mark.parametrize("T", [1, 4, 16])
def test_route_logits_are_lora_shrinks_and_the_outputs_are_moe_topks(T):
    bnb = _bnb()
    from bitsandbytes_amd.backends import hip

    E, K, S = 64, 256, 4
    W, xs = _router(E, K, torch.bfloat16, 70)
    x = xs[0][:T].contiguous()
    assert hip.lora_shrink_supported(x.dtype, T, E, K), "the shape is meant to be one the shrink kernel serves"
    ids, w, logits = bnb.moe_route(x, W, S, scoring="sigmoid", renormalize=True, scale=2.5, return_logits=True)
    assert torch.equal(logits, bnb.lora_shrink(x, W)) and torch.equal(logits, torch.ops.bitsandbytes_amd.lora_shrink.default(x, W))
    want = _op()(logits, S, "sigmoid", True, 2.5)
    assert torch.equal(ids, want[0]) and torch.equal(w, want[1])
    # an E the shrink kernel does not take (60 is no multiple of 8) and a logit bias: F.linear's logits, the same launch behind them
    W60, b60 = W[:60].contiguous(), torch.linspace(-1, 1, 60, device=DEV).bfloat16()
    for bias in (None, b60):
        ids, w, logits = bnb.moe_route(x, W60, S, bias=bias, return_logits=True)
        assert torch.equal(logits, torch.nn.functional.linear(x, W60, bias))
        want = _op()(logits, S, "softmax", True, 1.0)
        assert torch.equal(ids, want[0]) and torch.equal(w, want[1])
    router = bnb.nn.MoERouter(K, E, S, scoring="sigmoid", renormalize=True, scale=2.5, dtype=torch.bfloat16).to(DEV)
    router.load_state_dict({"weight": W})
    mids, mw = router(x)
    ids, w = bnb.moe_route(x, W, S, scoring="sigmoid", renormalize=True, scale=2.5)
    assert torch.equal(mids, ids) and torch.equal(mw, w)


def test_captured_route_follows_x():
    """One torch.cuda.graph of moe_route (two launches), replayed with new x in the same buffer: the bits of the eager call."""
    bnb = _bnb()
    E, K, S, T = 64, 256, 4, 4
    W, xs = _router(E, K, torch.bfloat16, 71)
    sb = (torch.arange(E, device=DEV) % 3 - 1).float()
    call = lambda x: bnb.moe_route(x, W, S, scoring="sigmoid", renormalize=True, scale=2.5, select_bias=sb)
    eager = [call(x[:T].contiguous()) for x in xs]
    assert not torch.equal(eager[1][0], eager[2][0])
    buf = xs[0][:T].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            call(buf)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ids, w = call(buf)
    for k in (1, 2, 0):
        buf.copy_(xs[k][:T])
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(ids, eager[k][0]) and torch.equal(w, eager[k][1]), f"replay {k} did not follow x"


def test_outputs_feed_the_expert_ffn_with_no_conversion():
    """moe_route's (ids, weights) go into the expert launches as they are. On the smallest shape of tests/moe_ffn_cases.py,
    4 x 96 x 96 at blocksize 32, into the gated launch and the routing-weight launch; that shape cannot form a whole block (its
    I = 48 is no multiple of a blocksize, so no down projection exists for it), so ``moe_ffn_4bit`` itself runs on the smallest shape
    of that list that can: 8 x 512 x 1024 at blocksize 64 (H = 1024, I = 256). Both against the same calls on converted copies
    (int64 ids, weights of x's dtype where that is exact)."""
    bnb = _bnb()
    F = bnb.functional
    smallest = min(FC.SHAPES, key=lambda s: s[0] * s[1] * s[2])
    assert smallest == (4, 96, 96, 32)
    gen = torch.Generator().manual_seed(80)
    T, S = 5, 2
    for (E, N, K, bs), whole_block in ((smallest, False), ((8, 512, 1024, 64), True)):
        I = N // 2
        x = torch.randn(T, K, generator=gen).bfloat16().to(DEV)
        Wr = (torch.randn(E, K, generator=gen) / K ** 0.5).bfloat16().to(DEV)
        ids, w = bnb.moe_route(x, Wr, S)
        assert ids.dtype == torch.int32 and w.dtype == torch.float32 and ids.is_contiguous() and w.is_contiguous()
        Wgu = (torch.randn(E, N, K, generator=gen) / K ** 0.5).bfloat16().to(DEV)
        gu, gu_state = F.quantize_4bit(Wgu, blocksize=bs, compress_statistics=False, quant_type="nf4")
        h = bnb.matmul_4bit_experts(x, gu, gu_state, ids, gated="chunked")
        assert h.shape == (T, S, I) and bool(torch.isfinite(h).all())
        assert torch.equal(h, bnb.matmul_4bit_experts(x, gu, gu_state, ids.to(torch.int64), gated="chunked"))
        y = bnb.matmul_4bit_experts(x, gu, gu_state, ids, row_scale=w)
        plain = bnb.matmul_4bit_experts(x, gu, gu_state, ids)
        assert y.shape == plain.shape == (T, S, N) and not torch.equal(y, plain)
        assert torch.equal(y, bnb.matmul_4bit_experts(x, gu, gu_state, ids.to(torch.int64), row_scale=w.clone()))
        if whole_block:
            Wdn = (torch.randn(E, K, I, generator=gen) / I ** 0.5).bfloat16().to(DEV)
            dn, dn_state = F.quantize_4bit(Wdn, blocksize=bs, compress_statistics=False, quant_type="nf4")
            out = bnb.moe_ffn_4bit(x, gu, gu_state, dn, dn_state, ids, w)
            assert out.shape == (T, K) and out.dtype == x.dtype and bool(torch.isfinite(out).all()) and float(out.abs().max()) > 0
            assert torch.equal(out, bnb.moe_ffn_4bit(x, gu, gu_state, dn, dn_state, ids.to(torch.int64), w.clone()))
