"""GPU: group-limited MoE routing as one launch (bitsandbytes_amd::moe_topk_grouped, csrc/moe_route.hip: moe_topk_grouped_kernel),
``bitsandbytes_amd.moe_topk_grouped`` / ``moe_route_grouped`` and ``nn.MoERouter(n_group=...)``.

* ids: on the cases of tests/moe_route_grouped_cases.py (keys AND group scores unambiguous in float64 by construction, planted group
  ties cut at topk_group, ids that the ungrouped ranking does not give) the kernel's ids ARE the float64 ranking of the five rules;
* weights: against float64, at most four times the error of torch's own fp32 composition on this GPU, floor 2^-20
  (moe_route_cases: WEIGHT_FACTOR, WEIGHT_FLOOR);
* n_group == 1 and topk_group == n_group: the bits of bitsandbytes_amd::moe_topk;
* a row's bits do not depend on the batch; non-finite logits and biases stay in their row and follow the rules (a NaN group goes
  last, a -inf group in front of it);
* the C entry point between guard bands at a 1-element offset; graph replay of ``moe_route_grouped``; its outputs feed the expert FFN.
The kernel has ONE path for every group size (no special case for powers of two), so there is no second path to compare bits with:
the geometries reach groups of 1, 2, 8, 10, 16, 20, 32, 36 and 64 experts. The preconditions of the cases are asserted on the CPU by
tests/test_moe_route_grouped_host.py.
"""
import ctypes as ct
import functools

import pytest
import torch

import guard_bands as GB
import moe_ffn_cases as FC
import moe_route_cases as C
import moe_route_grouped_cases as GC

pytestmark = pytest.mark.gpu

DEV = "cuda"
DT_CODE = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
MODE_CODE = {"max": 0, "top2sum": 1}


def _bnb():
    import bitsandbytes_amd as bnb

    return bnb


def _op():
    return torch.ops.bitsandbytes_amd.moe_topk_grouped.default


def _kernel(case, logits, bias):
    """The launch, through the op (no fall-back: the op raises where it has no kernel)."""
    return _op()(logits, case.S, case.n_group, case.topk_group, case.group_score, case.scoring, case.renormalize, case.scale, bias)


@functools.lru_cache(maxsize=None)
def _result(case):
    """One case, once: (kernel ids, kernel weights, composition ids, composition weights), on the CPU."""
    from bitsandbytes_amd.autograd._functions import _moe_topk_grouped_composition

    b = GC.build(case)
    logits = b.logits.to(DEV)
    bias = None if b.bias is None else b.bias.to(DEV)
    ids, w = _kernel(case, logits, bias)
    cids, cw = _moe_topk_grouped_composition(logits, case.S, case.n_group, case.topk_group, case.group_score, case.scoring, case.renormalize,
                                             case.scale, bias)
    return ids.cpu(), w.cpu(), cids.cpu(), cw.cpu()


# ------------------------------------------------------------------------------------------ ids and weights
@pytest.mark.parametrize("case", GC.CASES, ids=lambda c: c.name)
def test_ids_are_the_float64_ranking(case):
    b = GC.build(case)
    from bitsandbytes_amd.backends import hip

    ids, w, cids, _ = _result(case)
    assert ids.dtype == torch.int32 and w.dtype == torch.float32 and ids.shape == w.shape == (case.T, case.S)
    assert torch.equal(ids, b.ids), f"first differing row: {int((ids != b.ids).any(-1).nonzero()[0])}"
    assert torch.equal(cids, b.ids), "the torch composition on the GPU does not give the float64 ranking"
    assert bool(b.kept.gather(-1, (ids // case.G).long()).all())
    # the public function takes the launch for these classes - one call of the grouped C entry, none of the ungrouped one, not the
    # composition - with the same bits
    assert hip.moe_topk_grouped_supported(case.dtype, case.T, case.E, case.S, case.n_group, case.topk_group, case.group_score)
    with GC.CountedEntry() as entry:
        pids, pw = _bnb().moe_topk_grouped(b.logits.to(DEV), case.S, case.n_group, case.topk_group, case.group_score, case.scoring,
                                           case.renormalize, case.scale, None if b.bias is None else b.bias.to(DEV))
    assert (entry.calls, entry.plain) == (1, 0)
    assert torch.equal(pids.cpu(), ids) and torch.equal(pw.cpu(), w)


def test_weights_within_four_times_the_composition_error():
    """Max relative error against float64 over every weight of every case: the kernel's at most WEIGHT_FACTOR x the torch fp32
    composition's on this GPU, floor WEIGHT_FLOOR."""
    res = {c: _result(c) for c in GC.CASES}
    err_kernel = max(C.max_rel_err(res[c][1], GC.build(c).weights) for c in GC.CASES)
    err_torch = max(C.max_rel_err(res[c][3], GC.build(c).weights) for c in GC.CASES)
    bound = max(C.WEIGHT_FACTOR * err_torch, C.WEIGHT_FLOOR)
    print(f"moe_topk_grouped weights, max relative error against float64 over {len(GC.CASES)} cases: kernel {err_kernel:.3e}, "
          f"torch fp32 composition {err_torch:.3e}, bound {bound:.3e}")
    assert all(bool(torch.isfinite(res[c][1]).all()) for c in GC.CASES)
    assert err_kernel <= bound


@pytest.mark.parametrize("scoring", C.SCORINGS)
def test_one_group_or_every_group_kept_has_the_bits_of_moe_topk(scoring):
    """On the (E, S) of the geometries: n_group == 1, and topk_group == n_group for every n_group the geometries pair with that E
    (and 2), in both modes, against bitsandbytes_amd::moe_topk - ids and weight bits."""
    plain = torch.ops.bitsandbytes_amd.moe_topk.default
    gen = torch.Generator().manual_seed(4)
    for E, S in sorted({(g[0], g[3]) for g in GC.GEOMETRIES}):
        logits = (torch.randint(-32, 33, (9, E), generator=gen) / 8).bfloat16().to(DEV)
        sb = (torch.randint(-2, 3, (E,), generator=gen) / 4).float().to(DEV)
        want = plain(logits, S, scoring, True, 2.5, sb)
        for n_group in sorted({1, 2 if E % 2 == 0 else 1, *(g[1] for g in GC.GEOMETRIES if g[0] == E)}):
            for mode in GC.GROUP_SCORES:
                if mode == "top2sum" and E // n_group < 2:
                    continue
                ids, w = _op()(logits, S, n_group, n_group, mode, scoring, True, 2.5, sb)
                assert torch.equal(ids, want[0]) and torch.equal(w.view(torch.int32), want[1].view(torch.int32)), (E, n_group, mode)


# ------------------------------------------------------------------------------------------ rows do not see each other
T37 = [c for c in GC.CASES if c.T == 37]


@pytest.mark.parametrize("case", T37, ids=lambda c: c.name)
def test_every_row_of_a_37_row_call_has_the_bits_of_its_own_call(case):
    """37 rows = nine full workgroups of four wavefronts and one with a single live wavefront."""
    b = GC.build(case)
    logits = b.logits.to(DEV)
    bias = None if b.bias is None else b.bias.to(DEV)
    ids, w = _kernel(case, logits, bias)
    for t in range(case.T):
        i1, w1 = _kernel(case, logits[t:t + 1].contiguous(), bias)
        assert torch.equal(i1[0], ids[t]) and torch.equal(w1[0].view(torch.int32), w[t].view(torch.int32)), t
    assert len(T37) >= 3 and {c.scoring for c in T37} == set(C.SCORINGS) and {c.group_score for c in T37} == set(GC.GROUP_SCORES)


NAN, INF = float("nan"), float("inf")


def _poisons(E, G):
    """(name, row, write(logits, bias)) on E = 72 in 6 groups of 12: group 5 reaches over lane 63 into the second register slot."""
    def nan_logit(l, sb):
        l[5, 70] = NAN

    def inf_logit(l, sb):
        l[5, 70] = INF

    def nan_group(l, sb):            # a whole group of NaN logits: sigmoid drops it, behind the -inf group as well
        l[5, 2 * G:3 * G] = NAN
        sb[4 * G:5 * G] = -INF

    def minus_inf_group(l, sb):      # select_bias = -inf on a whole group: behind every finite group
        sb[5 * G:6 * G] = -INF

    def one_finite_key(l, sb):       # a group whose only finite key is one expert: "max" is that key, "top2sum" the sum with -inf
        sb[5 * G:6 * G] = -INF
        sb[5 * G + 3] = 1.0

    def one_key_not_nan(l, sb):      # ... and with NaN for the others: "max" finite, "top2sum" NaN - the group goes last
        l[5, 5 * G:6 * G] = NAN
        l[5, 5 * G + 11] = 4.0

    return [(f.__name__, f) for f in (nan_logit, inf_logit, nan_group, minus_inf_group, one_finite_key, one_key_not_nan)]


@pytest.mark.parametrize("group_score", GC.GROUP_SCORES)
@pytest.mark.parametrize("scoring", C.SCORINGS)
def test_non_finite_inputs_stay_in_their_row_and_follow_the_rules(scoring, group_score):
    E, n_group, topk_group, S, T = 72, 6, 3, 8, 16
    G = E // n_group
    case = GC.GroupedCase((E, n_group, topk_group, S), T, torch.float32, scoring, group_score, True, True)
    b = GC.build(case)
    clean_ids, clean_w = _kernel(case, b.logits.to(DEV), b.bias.to(DEV))
    assert torch.equal(clean_ids.cpu(), b.ids)
    for name, write in _poisons(E, G):
        dirty, sb = b.logits.clone(), b.bias.clone()
        write(dirty, sb)
        ids, w = _kernel(case, dirty.to(DEV), sb.to(DEV))
        ids, w = ids.cpu(), w.cpu()
        want_ids, _, kept = GC.reference(dirty, S, n_group, topk_group, group_score, scoring, True, case.scale, sb)
        rows_touched = [5] if torch.equal(sb, b.bias) else list(range(T))
        others = [t for t in range(T) if t not in rows_touched]
        assert torch.equal(ids[others], clean_ids.cpu()[others]), name
        assert torch.equal(w[others].view(torch.int32), clean_w.cpu()[others].view(torch.int32)), name
        for t in range(T):
            got = ids[t].tolist()
            assert len(set(got)) == S and all(0 <= i < E for i in got), (name, t, got)
            assert got == want_ids[t].tolist(), (name, t, got, want_ids[t].tolist())
            assert all(bool(kept[t, i // G]) for i in got), (name, t)
    # what the float64 reference says about the documented cases, so that the comparison above pins them (sigmoid: a NaN stays local)
    if scoring == "sigmoid":
        l, sb = b.logits.clone(), b.bias.clone()
        _poisons(E, G)[2][1](l, sb)
        kept = GC.reference(l, S, n_group, 5, group_score, scoring, True, 1.0, sb)[2][5]
        assert kept.tolist() == [True, True, False, True, True, True], "5 of 6 kept: the NaN group is the one dropped, behind the -inf group"
        l, sb = b.logits.clone(), b.bias.clone()
        _poisons(E, G)[5][1](l, sb)
        kept = GC.reference(l, S, n_group, 5, group_score, scoring, True, 1.0, sb)[2][5]
        assert bool(kept[5]) == (group_score == "max")
        got, _ = _op()(l.to(DEV), S, n_group, 5, group_score, scoring, True, 1.0, sb.to(DEV))
        assert torch.equal(got.cpu(), GC.reference(l, S, n_group, 5, group_score, scoring, True, 1.0, sb)[0])


# ------------------------------------------------------------------------------------------ the C entry point between guard bands
@pytest.mark.parametrize("dtype", C.DTYPES, ids=lambda d: str(d).replace("torch.", ""))
@pytest.mark.parametrize("group_score", GC.GROUP_SCORES)
def test_entry_point_between_guard_bands(dtype, group_score):
    """bnb_mi355x_moe_topk_grouped on operands carved between guard bands, each ONE element past a 256-byte boundary; E = 60 in 6
    groups of 10: lanes 60 ... 63 hold no expert. The bands (NaN / -1 around the inputs) and the inputs are untouched; every output
    byte is written: the call on outputs pre-filled with 0xA5 and with 0x5A leaves the same bytes, the op's."""
    from bitsandbytes_amd.cextension import MoeTopkGroupedArgs

    lib = _bnb().lib
    case = GC.GroupedCase((60, 6, 2, 4), 5, dtype, "sigmoid" if group_score == "top2sum" else "softmax", group_score, True, True)
    b = GC.build(case)
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
        args = MoeTopkGroupedArgs(ct.sizeof(MoeTopkGroupedArgs), DT_CODE[dtype], 0 if case.scoring == "softmax" else 1, 1, case.T, case.E, case.S,
                                  case.n_group, case.topk_group, MODE_CODE[group_score], case.scale, lg.ptr(), sb.ptr(), ids.ptr(), ws.ptr(),
                                  torch.cuda.current_stream().cuda_stream)
        assert lib.bnb_mi355x_moe_topk_grouped(ct.byref(args)) == 0
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
    from bitsandbytes_amd.cextension import MoeTopkGroupedArgs

    logits = torch.zeros(4, 64, device=DEV)
    ids = torch.full((4, 2), -7, dtype=torch.int32, device=DEV)
    w = torch.full((4, 2), -7.0, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    for over in (dict(struct_bytes=80), dict(n_group=3), dict(topk_group=9), dict(top_k=17), dict(group_score=2), dict(n_group=64, topk_group=8)):
        args = MoeTopkGroupedArgs(ct.sizeof(MoeTopkGroupedArgs), 0, 1, 1, 4, 64, 2, 8, 4, 1, 1.0, logits.data_ptr(), None, ids.data_ptr(),
                                  w.data_ptr(), stream)
        for k, v in over.items():
            setattr(args, k, v)
        assert _bnb().lib.bnb_mi355x_moe_topk_grouped(ct.byref(args)) != 0
    torch.cuda.synchronize()
    assert bool((ids == -7).all()) and bool((w == -7.0).all())
    with pytest.raises(ValueError, match="no kernel"):
        _op()(torch.zeros(2, 2048, device=DEV), 2, 8, 4, "top2sum", "sigmoid", True, 1.0)
    # ... which the public function serves by the composition, on the device, with no call of either entry
    big = torch.randn(3, 2048, generator=torch.Generator().manual_seed(2)).to(DEV)
    with GC.CountedEntry() as entry:
        got, _ = _bnb().moe_topk_grouped(big, 8, 128, 16)
    assert (entry.calls, entry.plain) == (0, 0)
    assert torch.equal(got.cpu(), GC.reference(big.cpu(), 8, 128, 16, "top2sum", "sigmoid", True, 1.0, None)[0])


# ------------------------------------------------------------------------------------------ the whole router
def _router(E, K, dtype, seed):
    gen = torch.Generator().manual_seed(seed)
    W = (torch.randn(E, K, generator=gen) / K ** 0.5).to(dtype).to(DEV)
    xs = [torch.randn(16, K, generator=gen).to(dtype).to(DEV) for _ in range(3)]
    return W, xs


def test_route_logits_are_moe_routes_and_the_module_routes_like_the_function():
    bnb = _bnb()
    E, K, S = 64, 256, 6
    W, xs = _router(E, K, torch.bfloat16, 72)
    sb = (torch.arange(E, device=DEV) % 3 - 1).float() / 4
    for T in (1, 4, 16):
        x = xs[0][:T].contiguous()
        ids, w, logits = bnb.moe_route_grouped(x, W, S, 8, 3, scale=2.5, select_bias=sb, return_logits=True)
        assert torch.equal(logits, bnb.moe_route(x, W, S, return_logits=True)[2]) and torch.equal(logits, bnb.lora_shrink(x, W))
        want = _op()(logits, S, 8, 3, "top2sum", "sigmoid", True, 2.5, sb)
        assert torch.equal(ids, want[0]) and torch.equal(w, want[1])
        assert all(len(set((row // 8).tolist())) <= 3 for row in ids.cpu())
    router = bnb.nn.MoERouter(K, E, S, scoring="sigmoid", renormalize=True, scale=2.5, select_bias=True, dtype=torch.bfloat16, n_group=8,
                              topk_group=3).to(DEV)
    router.load_state_dict({"weight": W, "e_score_correction_bias": sb})
    with GC.CountedEntry() as entry:
        mids, mw = router(x)
    assert (entry.calls, entry.plain) == (1, 0)
    assert torch.equal(mids, ids) and torch.equal(mw, w)


def test_captured_route_follows_x_and_feeds_the_expert_ffn():
    """One torch.cuda.graph of moe_route_grouped (two launches), replayed with new x in the same buffer: the bits of the eager call.
    Its (ids, weights) then go into the expert launches as they are, on the smallest shape of tests/moe_ffn_cases.py (4 x 96 x 96 at
    blocksize 32: E = 4 experts in 2 groups of 2, one kept)."""
    bnb = _bnb()
    F = bnb.functional
    E, N, K, bs = min(FC.SHAPES, key=lambda s: s[0] * s[1] * s[2])
    assert (E, N, K, bs) == (4, 96, 96, 32)
    S, T = 2, 4
    W, xs = _router(E, K, torch.bfloat16, 73)
    sb = torch.tensor([0.0, 0.25, -0.25, 0.0], device=DEV)
    call = lambda x: bnb.moe_route_grouped(x, W, S, 2, 1, scale=2.5, select_bias=sb)
    eager = [call(x[:T].contiguous()) for x in xs]
    assert len({tuple(e[0].flatten().tolist()) for e in eager}) > 1
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
        assert bool((ids // 2 == (ids // 2)[:, :1]).all()), "one group kept: both experts of a row come from it"
    assert ids.dtype == torch.int32 and w.dtype == torch.float32 and ids.is_contiguous() and w.is_contiguous()
    gen = torch.Generator().manual_seed(81)
    Wgu = (torch.randn(E, N, K, generator=gen) / K ** 0.5).bfloat16().to(DEV)
    gu, gu_state = F.quantize_4bit(Wgu, blocksize=bs, compress_statistics=False, quant_type="nf4")
    h = bnb.matmul_4bit_experts(buf, gu, gu_state, ids, gated="chunked")
    assert h.shape == (T, S, N // 2) and bool(torch.isfinite(h).all())
    assert torch.equal(h, bnb.matmul_4bit_experts(buf, gu, gu_state, ids.to(torch.int64), gated="chunked"))
    y = bnb.matmul_4bit_experts(buf, gu, gu_state, ids, row_scale=w)
    assert y.shape == (T, S, N) and torch.equal(y, bnb.matmul_4bit_experts(buf, gu, gu_state, ids.to(torch.int64), row_scale=w.clone()))
    # that shape cannot form a whole block (I = 48 is no multiple of a blocksize): moe_ffn_4bit itself on the smallest one that can,
    # 8 x 512 x 1024 at blocksize 64 - 8 experts in 4 groups of 2, 2 kept
    E, N, K, bs = 8, 512, 1024, 64
    assert (E, N, K, bs) in FC.SHAPES
    x = torch.randn(5, K, generator=gen).bfloat16().to(DEV)
    Wr = (torch.randn(E, K, generator=gen) / K ** 0.5).bfloat16().to(DEV)
    ids, w = bnb.moe_route_grouped(x, Wr, 3, 4, 2, group_score="max", scoring="softmax")
    assert all(len(set((row // 2).tolist())) == 2 for row in ids.cpu())
    Wgu = (torch.randn(E, N, K, generator=gen) / K ** 0.5).bfloat16().to(DEV)
    Wdn = (torch.randn(E, K, N // 2, generator=gen) / (N // 2) ** 0.5).bfloat16().to(DEV)
    gu, gu_state = F.quantize_4bit(Wgu, blocksize=bs, compress_statistics=False, quant_type="nf4")
    dn, dn_state = F.quantize_4bit(Wdn, blocksize=bs, compress_statistics=False, quant_type="nf4")
    out = bnb.moe_ffn_4bit(x, gu, gu_state, dn, dn_state, ids, w)
    assert out.shape == (5, K) and out.dtype == x.dtype and bool(torch.isfinite(out).all()) and float(out.abs().max()) > 0
    assert torch.equal(out, bnb.moe_ffn_4bit(x, gu, gu_state, dn, dn_state, ids.to(torch.int64), w.clone()))
