"""GPU: the fused optimizer update (csrc/optim8.hip) - bit for bit against the ledger of DESIGN.md §3.19 restated with one torch op
per rounding on the CPU (the project's pinned quantize_blockwise encodes the wanted states), the ledger itself against float64, and
the optimizer classes against direct calls."""
import math

import pytest
import torch

import bitsandbytes_amd as bnb
import bitsandbytes_amd.functional as F
from bitsandbytes_amd.optim import Adam8bit

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = (torch.float16, torch.bfloat16, torch.float32)
HYPER = {"adam": (0.9, 0.999), "momentum": (0.9, 0.0), "rmsprop": (0.99, 0.0), "adagrad": (0.0, 0.0), "lion": (0.9, 0.99)}
LR, EPS, GNORM_SCALE = 0.05, 1e-8, 0.75
QMAPS = (F.create_dynamic_map(signed=True), F.create_dynamic_map(signed=False))
CUS = 32


def ledger(name, g, p, s1, s2, step, wd, dt):
    """DESIGN.md §3.19, one torch op per rounding, in dtype dt (float32: the kernel's bits; float64: the formulas themselves).
    The scalars are computed in double and rounded to dt once. Returns the new (p, s1, s2) in dt."""
    b1, b2 = HYPER[name]
    S = lambda v: torch.tensor(v, dtype=dt)  # noqa: E731
    # CPU torch.sqrt of float32 is off by an ulp now and then (sqrt(4.7512688636779785) is); through float64 it is correctly
    # rounded - 53 bits are more than 2 * 24 + 2, so the second rounding cannot move the result
    sqrt = lambda x: torch.sqrt(x.double()).to(dt)  # noqa: E731
    g, p = g.to(dt) * S(GNORM_SCALE), p.to(dt)
    if name in ("adam", "lion") and wd > 0:
        p = p * S(1.0 - LR * wd)
    if name in ("momentum", "rmsprop", "adagrad") and wd > 0:
        g = g + p * S(wd)
    if name == "adam":
        s1 = s1 * S(b1) + g * S(1.0 - b1)
        s2 = s2 * S(b2) + (g * g) * S(1.0 - b2)
        d = sqrt(s2) / S(math.sqrt(1.0 - b2 ** step)) + S(EPS)
        p = p + (s1 / d) * S(-LR / (1.0 - b1 ** step))
    elif name == "lion":
        u = s1 * S(b1) + g * S(1.0 - b1)
        p = p + ((u > 0).to(dt) - (u < 0).to(dt)) * S(-LR)
        s1 = s1 * S(b2) + g * S(1.0 - b2)
    elif name == "momentum":
        s1 = g if step == 1 else s1 * S(b1) + g
        p = p + s1 * S(-LR)
    else:
        s1 = s1 * S(b1) + (g * g) * S(1.0 - b1) if name == "rmsprop" else s1 + g * g
        p = p + (g / (sqrt(s1) + S(EPS))) * S(-LR)
    return p, s1, s2


def dequant(codes, absmax, qmap, dt=torch.float32):
    return qmap.cpu().to(dt)[codes.cpu().long()] * absmax.cpu().to(dt).repeat_interleave(256)[: codes.numel()]


def inputs(name, dtype, n, step, offset=0, zero=False):
    """g, p (CPU), their device copies, and the fp32 start value of every state. offset 1: the device tensors are views that start
    one element past the allocation's alignment."""
    gen = torch.Generator().manual_seed(n + 7 * step)
    g = (torch.zeros(n + offset) if zero else torch.randn(n + offset, generator=gen)).to(dtype)
    p = torch.randn(n + offset, generator=gen).to(dtype)
    xs = [torch.randn(n + offset, generator=gen) for _ in range(2 if name == "adam" else 1)]
    # (state2, and state1 of rmsprop and adagrad, is a second moment: never negative, and sqrt() of it must not be NaN)
    xs = [(x * x if i or name in ("rmsprop", "adagrad") else x)[offset:] for i, x in enumerate(xs)]
    return g[offset:], p[offset:], g.to(DEV)[offset:], p.to(DEV)[offset:], xs


def run(name, dtype, n, step, wd, offset=0, zero=False):
    """One 8-bit launch on fresh inputs. Returns the inputs (CPU) and the updated device tensors."""
    two = name == "adam"
    g, p, gd, pd, xs = inputs(name, dtype, n, step, offset, zero)
    st = []
    for i, x in enumerate(xs):
        codes, qs = F.quantize_blockwise(x.to(DEV), code=QMAPS[i].to(DEV), blocksize=256)
        if zero:
            codes, qs.absmax = torch.zeros_like(codes), torch.zeros_like(qs.absmax)
        st.append((codes, qs.absmax, QMAPS[i].to(DEV)))
    before = [(c.clone(), a.clone()) for c, a, _ in st]
    assert offset == 0 or pd.data_ptr() % 8 != 0
    s2 = st[1] if two else (None, None, None)
    b1, b2 = HYPER[name]
    F.optimizer_update_8bit_blockwise(name, gd, pd, st[0][0], s2[0], b1, b2, 0.0, 0.0, EPS, step, LR, st[0][2], s2[2], st[0][1], s2[1], wd,
                                      GNORM_SCALE)
    return g, p, before, pd, st


def check_bits(name, dtype, n, step, wd, **kw):
    g, p, before, pd, st = run(name, dtype, n, step, wd, **kw)
    old = [dequant(c, a, q) for (c, a), q in zip(before, QMAPS)] + [None]
    want_p, *want_s = ledger(name, g, p, old[0], old[1], step, wd, torch.float32)
    what = f"{name} {dtype} n={n} step={step} wd={wd} {kw}"
    assert torch.equal(pd.cpu(), want_p.to(dtype)), f"p: {what}"
    for i, (codes, absmax, qmap) in enumerate(st):
        want_codes, qs = F.quantize_blockwise(want_s[i].to(DEV), code=qmap, blocksize=256)
        assert torch.equal(codes, want_codes), f"state{i + 1}: {what}"
        assert torch.equal(absmax, qs.absmax), f"absmax{i + 1}: {what}"
    return st


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("name", sorted(HYPER))
def test_update_matches_the_ledger_bit_for_bit(name, dtype):
    """n: one element; around one block; a partial block in a workgroup's last wavefront; the persistent loop (32 CUs)."""
    for n in (1, 255, 256, 257, 1027):
        for step, wd in ((1, 0.0), (7, 0.0), (1, 0.01), (7, 0.01)):
            check_bits(name, dtype, n, step, wd)
    bnb.lib.bnb_mi355x_set_cu_count(CUS)
    try:
        grid = bnb.lib.bnb_mi355x_optimizer_update_grid(1 << 30)   # the persistent grid's cap on 32 CUs; 1024 elements per pass each
        n = 2 * grid * 1024 + 257
        assert bnb.lib.bnb_mi355x_optimizer_update_grid(n) == grid and 2 * grid * 1024 < n < 1 << 19
        check_bits(name, dtype, n, 7, 0.01)
    finally:
        bnb.lib.bnb_mi355x_set_cu_count(0)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_unaligned_views_take_the_scalar_path(dtype):
    check_bits("adam", dtype, 1027, 7, 0.01, offset=1)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("name", sorted(HYPER))
def test_fp32_states_match_the_ledger_bit_for_bit(name, dtype):
    """optimizer_update_32bit (STATE = float): vector loads with a scalar tail (n = 257), then everything offset by one element."""
    b1, b2 = HYPER[name]
    for offset in (0, 1):
        g, p, gd, pd, xs = inputs(name, dtype, 257, 7, offset)
        sd = [torch.cat([x.new_zeros(offset), x]).to(DEV)[offset:] for x in xs] + [None]
        assert offset == 0 or sd[0].data_ptr() % 16 != 0
        F.optimizer_update_32bit(name, gd, pd, sd[0], b1, EPS, 7, LR, sd[1], b2, weight_decay=0.01, gnorm_scale=GNORM_SCALE)
        want_p, *want_s = ledger(name, g, p, xs[0], (xs + [None])[1], 7, 0.01, torch.float32)
        assert torch.equal(pd.cpu(), want_p.to(dtype)), f"p, offset {offset}"
        for i in range(len(xs)):
            assert torch.equal(sd[i].cpu(), want_s[i]), f"state{i + 1}, offset {offset}"


@pytest.mark.parametrize("name", sorted(HYPER))
def test_all_zero_block_gives_codes_zero_and_absmax_zero(name):
    for codes, absmax, _ in check_bits(name, torch.bfloat16, 513, 1, 0.0, zero=True):
        assert not codes.any() and not absmax.any()


def ulp(x, dtype):
    mant, emin = {torch.float32: (23, -126), torch.float16: (10, -14), torch.bfloat16: (7, -126)}[dtype]
    return torch.exp2((torch.frexp(x)[1] - 1).clamp(min=emin).double() - mant)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("name", sorted(HYPER))
def test_update_against_float64(name, dtype):
    """One step from the same inputs in float64 (scalars in double). Derivation of the bounds, u = 2^-24:
    p: the kernel rounds fp32 -> T once (half an ulp of T at the result) after at most 12 fp32 operations on the way to p, each
    with relative error u on a value no larger than |p0| + |delta|; 16 u (|p0| + |delta64|) covers them with first-order slack.
    state: the encoder returns the code nearest to the 16-bit bin value of s / absmax: half the widest code gap w at or next to
    that position, plus 2 / 65535 for the binning (bin width and the rounding of the bin index), times absmax; the fp32 update
    and the fp32 product code * absmax add at most 16 u |s64|. Every element is checked."""
    n, step, wd = 4096 + 3, 7, 0.01
    g, p, before, pd, st = run(name, dtype, n, step, wd)
    old = [dequant(c, a, q, torch.float64) for (c, a), q in zip(before, QMAPS)] + [None]
    p64, *s64 = ledger(name, g, p, old[0], old[1], step, wd, torch.float64)
    u16 = 16 * 2.0 ** -24
    bound_p = ulp(p64, dtype) / 2 + u16 * (p.double().abs() + (p64 - p.double()).abs())
    assert ((pd.cpu().double() - p64).abs() <= bound_p).all()
    for i, (codes, absmax, qmap) in enumerate(st):
        am = absmax.cpu().double().repeat_interleave(256)[:n]
        q64 = QMAPS[i].double()
        gaps = torch.cat([q64.new_zeros(1), q64[1:] - q64[:-1], q64.new_zeros(1)])   # gaps[k]: between code k - 1 and code k
        k = torch.searchsorted(q64, (s64[i] / am).clamp(-1, 1)).clamp(1, 255)        # code k - 1 <= position <= code k
        w = torch.stack([gaps[k - 1], gaps[k], gaps[k + 1]]).amax(0)
        got = dequant(codes, absmax, qmap, torch.float64)
        assert ((got - s64[i]).abs() <= am * (w / 2 + 2 / 65535) + u16 * s64[i].abs()).all(), f"state{i + 1}"


def test_adam8bit_class_matches_direct_calls_and_round_trips():
    torch.manual_seed(0)
    model = torch.nn.Linear(64, 64).to(DEV, torch.bfloat16)   # weight: 4096 elements, 8-bit; bias: 64, fp32 states
    late = torch.nn.Parameter(torch.ones(8, device=DEV))       # gets its first grad only after the state dict is loaded
    opt = Adam8bit([*model.parameters(), late], lr=LR, weight_decay=0.01)
    params = [p.detach().clone() for p in model.parameters()]
    maps = [m.to(DEV) for m in QMAPS]
    s8 = [torch.zeros(4096, dtype=torch.uint8, device=DEV) for _ in range(2)] + [torch.zeros(16, device=DEV) for _ in range(2)]
    s32 = [torch.zeros(64, device=DEV) for _ in range(2)]
    for step in (1, 2):
        grads = [torch.randn_like(p) for p in params]
        for p, g in zip(model.parameters(), grads):
            p.grad = g.clone()
        opt.step()
        F.optimizer_update_8bit_blockwise("adam", grads[0], params[0], s8[0], s8[1], 0.9, 0.999, 0.0, 0.0, 1e-8, step, LR, maps[0], maps[1],
                                          s8[2], s8[3], 0.01)
        F.optimizer_update_32bit("adam", grads[1], params[1], s32[0], 0.9, 1e-8, step, LR, s32[1], 0.999, weight_decay=0.01)
    w, b = (opt.state[p] for p in model.parameters())
    assert all(torch.equal(p, q) for p, q in zip(model.parameters(), params))
    assert set(w) == {"step", "state1", "state2", "qmap1", "qmap2", "absmax1", "absmax2"} and set(b) == {"step", "state1", "state2"}
    assert w["step"] == 2 and [w[k].dtype for k in ("state1", "state2", "qmap1", "absmax1")] == [torch.uint8] * 2 + [torch.float32] * 2
    for got, want in zip([w["state1"].view(-1), w["state2"].view(-1), w["absmax1"], w["absmax2"], b["state1"], b["state2"]], s8 + s32):
        assert got.dtype == want.dtype and torch.equal(got, want)
    assert torch.equal(w["qmap1"], maps[0]) and torch.equal(w["qmap2"], maps[1])
    opt2 = Adam8bit([*model.parameters(), late], lr=LR, weight_decay=0.01)
    opt2.load_state_dict(opt.state_dict())
    assert late not in opt.state and len(opt2.state[late]) == 0
    for p in model.parameters():
        assert opt2.state[p].keys() == opt.state[p].keys()
        for k, v in opt.state[p].items():
            v2 = opt2.state[p][k]
            assert v2 == v if k == "step" else (v2.dtype == v.dtype and torch.equal(v2, v)), k
    late.grad = torch.ones_like(late)       # a step after loading, with a parameter that had no saved state
    opt2.step()
    assert opt2.state[late]["step"] == 1 and opt2.state[model.weight]["step"] == 3 and not torch.equal(late, torch.ones_like(late))
    with pytest.raises(NotImplementedError):
        F.optimizer_update_32bit("adam", grads[1], params[1], s32[0], 0.9, 1e-8, 3, LR, s32[1], 0.999, max_unorm=1.0)
    with pytest.raises(NotImplementedError):
        F.optimizer_update_8bit_blockwise("ademamix", grads[0], params[0], s8[0], s8[1], 0.9, 0.999, 0.9999, 5.0, 1e-8, 3, LR, maps[0], maps[1],
                                          s8[2], s8[3])
