"""CPU (-m "not gpu"): the preconditions of tests/test_gpu_decode_probe.py (tests/decode_probe_cases.py), for every case:

* the builders' preconditions: power-of-two scales that differ between neighbouring blocks, nested statistics that reconstruct the
  intended scales through the oracle's ``dequantize_blockwise`` bit for bit, and the rounding condition - decoding to T first, scaling
  first or staying in fp32 give one answer, a normal number of T - for every (code, scale, v) the case uses;
* the want equals the oracle CPU backend's ``gemm_4bit`` bit for bit on the same packed bytes (a subsample of the probe rows: the
  oracle is scalar C), and the whole weight equals the oracle's ``dequantize_4bit``; for the backward: the oracle's dequantized weight
  times the one-hot gradients; for the caller-supplied table (no oracle path): fp32 arithmetic on the gathered table entries;
* every one of the 256 byte values occurs, and under a uniform model every (copy, entry) cell of the family's table is read at least
  READS_FLOOR times;
* the probe bites: a CPU emulation of a kernel's table (copies x 256 entries, a copy per position) with one thing broken at a time - a
  code literal, the hi / lo order of the table build, one entry of one copy - is caught, and the report names the byte and the code.
"""
import pytest
import torch

import decode_probe_cases as P
from oracle import oracle as O

_id = lambda cs: f"{cs.family}-{cs.name}"


def _same(a, b):
    return not bool(P.mismatches(a, b).any())


def test_code_tables_are_the_oracles():
    for qt in ("nf4", "fp4"):
        mine, theirs = P.code_table(qt), O.get_4bit_code(qt)
        assert not bool(P.mismatches(mine, theirs).any()), qt                   # (bits; the sign of FP4's second zero is free)
    c = P.code_table("code16")
    assert c.dtype == torch.float32 and torch.unique(c).numel() == 16 and bool((c < 0).any()) and bool((c > 0).any())


def test_case_list_covers_what_each_family_is_asked_for():
    names = [_id(cs) for cs in P.ALL_CASES]
    assert len(set(names)) == len(names), "two cases share an id"
    fam = P.CASES
    assert set(fam) == set(P.COPIES)
    for f in ("stream", "sm", "rt", "kq", "pc", "tall"):
        assert all(cs.N == 1040 for cs in fam[f]), f
    assert {cs.K for cs in fam["stream"] + fam["sm"] + fam["experts"]} == {576}
    assert {cs.K for cs in fam["tall"]} == {512} and all(cs.K % 256 == 0 for cs in fam["pc"] + fam["rt"] + fam["kq"])
    for f in ("pc", "rt", "kq"):     # the single-slice form and one with two slices
        assert {cs.knob % 100 for cs in fam[f]} == {1, 2}, f
    assert {cs.knob // 100 for cs in fam["pc"]} == {11, 12, 13, 14}
    assert {cs.dtype for cs in fam["stream"]} == {P.BF, P.HF, P.F32} and {cs.quant for cs in fam["stream"]} == {"nf4", "fp4", "code16"}
    assert {(cs.blocksize, cs.nested) for cs in fam["stream"]} >= {(64, False), (64, True), (32, False), (128, True), (4096, False)}
    assert all(cs.rows == 16 for cs in fam["sm"]) and {(cs.blocksize, cs.nested) for cs in fam["sm"]} == {(64, False), (64, True), (1024, False)}
    assert {(cs.blocksize, cs.nested) for cs in fam["rt"]} >= {(32, False), (64, True), (1024, False)}
    assert all(cs.blocksize == 64 for cs in fam["kq"] if cs.nested) and any(cs.nested for cs in fam["kq"])
    assert {(cs.dtype, cs.quant) for cs in fam["tall"]} == {(d, q) for d in (P.BF, P.HF) for q in ("nf4", "fp4")}
    ex = [cs for cs in fam["experts"] if cs.fill == "random"]
    assert len({(cs.dtype, cs.quant, cs.blocksize, cs.nested) for cs in ex}) == 3 * 2 * 2 * 2 and all((cs.E, cs.N, cs.K) == (3, 272, 576) for cs in ex)
    gi = [cs for cs in fam["grad_input"] if cs.fill == "random"]
    assert len({(cs.dtype, cs.quant, cs.blocksize, cs.nested, cs.plan) for cs in gi}) == 2 * 2 * 3 * 2 and all((cs.N, cs.K) == (320, 640) for cs in gi)
    for f in fam:
        assert sum(cs.fill == "structured" for cs in fam[f]) == 1, f


def test_one_hot_rows_and_the_experts_probe():
    x, v = P.one_hot_rows(torch.tensor([5, 0, 5, 63, 2, 2, 2, 2, 7]), 64, torch.float16)
    assert v.tolist() == list(P.V_CYCLE) + [P.V_CYCLE[0]] and x[3, 63] == -0.5 and x[8, 7] == 1.0 and int((x != 0).sum()) == 9
    cs = P.CASES["experts"][0]
    x, ids, v = P.experts_probe(cs)
    assert x.shape == (576, 4, 576) and ids.shape == (576, 4) and ids.dtype == torch.int32
    assert set(ids.unique().tolist()) == {-1, 0, 1, 2, 3}
    for e in range(3):   # every expert at every k, once
        t, s = (ids == e).nonzero(as_tuple=True)
        assert torch.equal(t, torch.arange(576)) and bool((x[t, s, t] == v[t, s].to(x.dtype)).all())
    assert len({float(a) for a in v[0]}) == 4, "the slots of a token carry different values"


def test_comparison_rule():
    a = torch.tensor([0.0, -0.0, 1.0, 0.0, -0.0], dtype=torch.bfloat16)
    b = torch.tensor([-0.0, -0.0, 1.0078125, 2.0 ** -133, 0.0], dtype=torch.bfloat16)
    assert P.mismatches(b, a).tolist() == [False, False, True, True, False]    # either zero passes only where the want IS zero
    f = torch.tensor([1.0, -1.0]); g = torch.tensor([1.0, 1.0])
    assert P.mismatches(f, g).tolist() == [False, True]


@pytest.mark.parametrize("cs", P.ALL_CASES, ids=_id)
def test_case_preconditions_and_want_against_the_oracle(cs):
    fills = cs.fills if cs.fill == "random" else 1
    if cs.fill == "random":
        assert P.expected_reads_per_cell(cs) >= P.READS_FLOOR, P.expected_reads_per_cell(cs)
    for fi in range(fills):
        pr = P.build(cs, fi)
        R, K, N, bs = cs.weight_rows, cs.K, cs.N, cs.blocksize
        assert pr.bytes.shape == (R, K // 2) and torch.bincount(pr.bytes.reshape(-1).long(), minlength=256).min() >= 1
        if fi:
            assert not torch.equal(pr.bytes, P.build_bytes(cs, 0)), "a second fill repeats the first"
        checked = P.assert_rounding_precondition(pr.code16, pr.scale, cs.dtype)
        assert checked == 16 * torch.unique(pr.scale).numel() * 8 and torch.unique(pr.scale).numel() >= 4
        if cs.nested:
            rec = O.dequantize_blockwise(pr.absmax_8bit, pr.absmax, pr.absmax_code, 256, torch.float32) + pr.offset
            assert torch.equal(rec, pr.scale), "nested statistics do not reconstruct the intended scales"
            groups = pr.absmax.numel()
            assert groups == -(pr.scale.numel() // -256) and (groups < 2 or float(pr.absmax[0]) != float(pr.absmax[1]))
        wT = pr.W64.float().to(cs.dtype)
        if cs.quant == "code16":
            # no oracle path takes a caller's table: fp32 arithmetic on the gathered entries instead (exact: powers of two)
            s = pr.scale.repeat_interleave(bs)[:R * K].view(R, K)
            w32 = pr.code16[pr.nibbles.long()] * s
            ks = torch.arange(K)
            x, v = P.one_hot_rows(ks, K, cs.dtype)
            assert torch.equal(pr.want_forward(ks, v), (w32.t() * v.float()[:, None])) and torch.equal(w32.double(), pr.W64)
            continue
        deq = O.dequantize_4bit(pr.packed, pr.scale, bs, cs.quant, (R, K), cs.dtype)
        assert _same(deq, wT), "the constructed weight is not the oracle's dequantize_4bit"
        if cs.family == "grad_input":
            ns = torch.arange(N)
            g, v = P.one_hot_rows(ns, N, cs.dtype)
            want = pr.want_backward(ns, v)
            assert _same((g.double() @ deq.double()).float().to(cs.dtype), want)
            continue
        for e in range(cs.E):
            ks = P.host_sample(K)
            xf, vf = P.one_hot_rows(torch.arange(K), K, cs.dtype)
            x, v = xf[ks], vf[ks]
            want = pr.want_forward(ks, v, expert=e)
            rows = slice(e * N, (e + 1) * N)
            if cs.nested and cs.E == 1:
                y = O.gemm_4bit(x, pr.packed, (N, K), pr.absmax, bs, cs.quant, None, pr.absmax_8bit, pr.absmax_code, pr.offset)[0]
            else:   # (an expert's blocks start inside a group of 256: the reconstructed scales, checked above, as plain statistics)
                blocks = -((N * K) // -bs)
                assert cs.E == 1 or (N * K) % bs == 0
                y = O.gemm_4bit(x, pr.bytes[rows].reshape(-1, 1), (N, K), pr.scale[e * blocks:(e + 1) * blocks], bs, cs.quant)[0]
            assert y.dtype == cs.dtype and _same(y, want), str(P.first_mismatch(pr, y, want, ks, expert=torch.full((ks.numel(),), e)))
        if cs.family == "experts":
            x, ids, v = P.experts_probe(cs)
            want = P.experts_want(pr, ids, v)
            masked = (ids < 0) | (ids >= cs.E)
            assert not bool(want[masked].any()) and bool((want[~masked] != 0).any(dim=1).all())


# ------------------------------------------------------------------------------------------ the probe bites
def _emulate(pr, table, copies):
    """What a kernel with this decode table returns for the full forward probe: ``table`` [copies, 256, 2] fp32 - copy c of entry e holds
    (code[e >> 4], code[e & 15]) - read at copy ``(n + 3 j) mod copies`` for byte (n, j), scaled in fp32 and rounded to T."""
    cs = pr.case
    K, N = cs.K, cs.N
    ks = torch.arange(K)
    x, v = P.one_hot_rows(ks, K, cs.dtype)
    n = torch.arange(N)[None, :].expand(K, N)
    j = (ks // 2)[:, None].expand(K, N)
    byte = pr.bytes[n, j].long()
    val = table[(n + 3 * j) % copies, byte, (ks % 2)[:, None].expand(K, N)]
    s = pr.scale.repeat_interleave(cs.blocksize)[:N * K].view(N, K).t()
    return (val * s * v.float()[:, None]).to(cs.dtype), pr.want_forward(ks, v), ks


def _table(code, copies, swap=False):
    e = torch.arange(256)
    pair = torch.stack([code[e >> 4], code[e & 15]], dim=1)
    if swap:
        pair = pair.flip(1)
    return pair[None].repeat(copies, 1, 1)


@pytest.mark.parametrize("cs", [P.CASES["sm"][2], P.CASES["stream"][0], P.CASES["kq"][1]], ids=_id)
def test_probe_catches_a_broken_decode_table_in_a_cpu_emulation(cs):
    pr = P.build(cs)
    copies = P.COPIES[cs.family]
    code = pr.code16.clone()
    got, want, ks = _emulate(pr, _table(code, copies), copies)
    assert P.first_mismatch(pr, got, want, ks) is None, "the emulation of a correct table must pass"
    # one code literal: index 1 (FP4: +0.0052, the value a norm cannot see) returns 0
    broken = code.clone()
    broken[1] = 0.0
    got, want, ks = _emulate(pr, _table(broken, copies), copies)
    mm = P.first_mismatch(pr, got, want, ks)
    bad = P.mismatches(got, want)
    idx = pr.nibbles[: cs.N].t()
    assert mm is not None and mm.index == 1 and mm.got == 0.0 and mm.want != 0.0 and "code index=1" in str(mm)
    assert torch.equal(bad, idx == 1), "exactly the weights of code 1 differ"
    # the hi / lo order of the table build
    got, want, ks = _emulate(pr, _table(code, copies, swap=True), copies)
    mm = P.first_mismatch(pr, got, want, ks)
    assert mm is not None and f"byte=0x{mm.byte:02x}" in str(mm)
    other = (mm.byte & 15) if mm.nibble == "hi" else (mm.byte >> 4)
    assert float(code[other]) != mm.code, "the byte named holds two different codes"
    by = pr.bytes[: cs.N].long()
    differs = (code[by >> 4] != code[by & 15]).repeat_interleave(2, dim=1).t()
    assert torch.equal(P.mismatches(got, want), differs), "exactly the bytes whose two codes differ are reported"
    # one entry of one copy: the low half of entry 0xA7 in copy 5 holds its neighbour's value
    tb = _table(code, copies)
    tb[5, 0xA7, 1] = code[8 if cs.quant == "nf4" else 6]
    got, want, ks = _emulate(pr, tb, copies)
    mm = P.first_mismatch(pr, got, want, ks)
    n = torch.arange(cs.N)[:, None]
    j = torch.arange(cs.K // 2)[None, :]
    cell = (pr.bytes[: cs.N] == 0xA7) & ((n + 3 * j) % copies == 5)
    assert mm is not None and mm.byte == 0xA7 and mm.nibble == "lo" and mm.index == 7 and (mm.n + 3 * (mm.k // 2)) % copies == 5
    assert mm.count == int(cell.sum()) and mm.count >= 1, "every read of the broken cell is reported, nothing else"
