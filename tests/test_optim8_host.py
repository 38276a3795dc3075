"""CPU: the host side of the 8-bit optimizers - op schemas, fake kernels, the exported C entry points. No compute (no GPU here)."""
import ctypes as ct

import pytest
import torch

import bitsandbytes_amd as bnb

OPS = torch.ops.bitsandbytes

# the reference's schemas (bitsandbytes/_ops.py:409-455)
SCHEMAS = {
    "optimizer_update_32bit": "(str optimizer_name, Tensor(a0!) g, Tensor(a1!) p, Tensor(a2!) state1, Tensor(a3!)? state2, Tensor(a4!)? unorm_vec, float max_unorm, float param_norm, float beta1, float beta2, float beta3, float alpha, float eps, float weight_decay, int step, float lr, float gnorm_scale, bool skip_zeros=False) -> ()",
    "optimizer_update_8bit_blockwise": "(str optimizer_name, Tensor(a0!) g, Tensor(a1!) p, Tensor(a2!) state1, Tensor(a3!)? state2, float beta1, float beta2, float beta3, float alpha, float eps, int step, float lr, Tensor(a4!) qmap1, Tensor(a5!)? qmap2, Tensor(a6!) absmax1, Tensor(a7!)? absmax2, float weight_decay, float gnorm_scale, bool skip_zeros=False) -> ()",
}


@pytest.mark.parametrize("name", sorted(SCHEMAS))
def test_op_exists_with_the_reference_schema(name):
    want = torch._C.parse_schema(f"bitsandbytes::{name}{SCHEMAS[name]}")
    assert str(getattr(OPS, name).default._schema) == str(want)


def test_fake_kernels_reject_mismatched_dtypes():
    def meta(n, dtype):
        return torch.empty(n, dtype=dtype, device="meta")

    g, p, f32 = meta(512, torch.bfloat16), meta(512, torch.bfloat16), torch.float32
    codes, qmap, absmax = meta(512, torch.uint8), meta(256, f32), meta(2, f32)
    tail = (0.9, 0.999, 0.0, 0.0, 1e-8, 1, 1e-3)
    assert OPS.optimizer_update_8bit_blockwise.default("adam", g, p, codes, codes, *tail, qmap, qmap, absmax, absmax, 0.0, 1.0) is None
    assert OPS.optimizer_update_32bit.default("adam", g, p, meta(512, f32), meta(512, f32), None, 0.0, 0.0, *tail[:5], 0.0, 1, 1e-3, 1.0) is None
    for bad in (dict(g=meta(512, torch.float16)), dict(g=meta(256, torch.bfloat16)), dict(s1=meta(512, f32)), dict(s2=meta(512, f32)),
                dict(absmax=meta(2, torch.bfloat16)), dict(qmap=meta(256, torch.float16))):
        a = {"g": g, "s1": codes, "s2": codes, "qmap": qmap, "absmax": absmax, **bad}
        with pytest.raises(RuntimeError):
            OPS.optimizer_update_8bit_blockwise.default("adam", a["g"], p, a["s1"], a["s2"], *tail, a["qmap"], qmap, a["absmax"], absmax, 0.0, 1.0)
    with pytest.raises(RuntimeError):
        OPS.optimizer_update_32bit.default("adam", meta(512, torch.float16), p, meta(512, f32), None, None, 0.0, 0.0, *tail[:5], 0.0, 1, 1e-3, 1.0)


def test_c_entry_points_are_exported_and_refuse_without_launching():
    from bitsandbytes_amd.cextension import EXPORTED_SYMBOLS, OptimizerUpdateArgs

    for name in ("bnb_mi355x_optimizer_update_8bit_blockwise", "bnb_mi355x_optimizer_update_32bit"):
        assert name in EXPORTED_SYMBOLS and hasattr(bnb.lib, name)
    args = OptimizerUpdateArgs(struct_bytes=ct.sizeof(OptimizerUpdateArgs), optimizer=9, dtype=0, n=4)
    assert bnb.lib.bnb_mi355x_optimizer_update_8bit_blockwise(ct.byref(args)) == 2   # BNB_MI355X_OPTIM_REFUSED_OPTIMIZER
    args.optimizer, args.dtype = 0, 7
    assert bnb.lib.bnb_mi355x_optimizer_update_32bit(ct.byref(args)) == 3            # BNB_MI355X_OPTIM_REFUSED_DTYPE
    args.dtype = 0
    assert bnb.lib.bnb_mi355x_optimizer_update_32bit(ct.byref(args)) == 1            # BNB_MI355X_OPTIM_MALFORMED: NULL pointers
    args.struct_bytes -= 8
    assert bnb.lib.bnb_mi355x_optimizer_update_32bit(ct.byref(args)) == 1
    assert callable(bnb.functional.optimizer_update_8bit_blockwise) and callable(bnb.functional.optimizer_update_32bit)
    assert {"Adam8bit", "AdamW8bit", "Lion8bit", "SGD8bit", "RMSprop8bit", "Adagrad8bit"} <= set(bnb.optim.__all__)


def test_load_state_dict_takes_the_reference_nested_form_keeps_dtypes_and_runs_hooks():
    p, q = torch.nn.Parameter(torch.zeros(8, dtype=torch.bfloat16)), torch.nn.Parameter(torch.zeros(8, dtype=torch.bfloat16))
    opt = bnb.optim.Adam8bit([p, q])
    quant = {"state1": torch.arange(8, dtype=torch.uint8), "absmax1": torch.tensor([0.5]), "qmap1": torch.linspace(-1, 1, 256)}
    saved = {"state": {0: {"step": 3, "__bnb_optimizer_quant_state__": quant}}, "param_groups": opt.state_dict()["param_groups"]}
    seen = []
    opt.register_load_state_dict_pre_hook(lambda o, sd: seen.append("pre"))
    opt.register_load_state_dict_post_hook(lambda o: seen.append("post"))
    opt.load_state_dict(saved)
    assert seen == ["pre", "post"] and opt.state[p]["step"] == 3 and opt.state[q] == {}   # (q: no saved state, no KeyError)
    for k, v in quant.items():
        assert opt.state[p][k].dtype == v.dtype and torch.equal(opt.state[p][k], v)
