"""CPU: the AdamW state-precision modes as far as they need no device -- the third header / binding table / library agree, the argument
checks of both entries return before any launch, FlatAdamW's `state_precision` switch and its state-dict conversions, and the fixture
check of tests/test_adamw_modes_gpu.py: the references of tests/optim_ref.py alone meet every cap that file asserts on the device."""
import os
import re

import numpy as np
import pytest
import torch

import optim_ref as R
from util import ROOT, tiny_cfg


def test_optim_header_binding_and_library_agree():
    from navillm_amd import lib
    hdr = open(os.path.join(ROOT, "include", "navillm_hip_optim.h")).read()
    declared = set(re.findall(r"\b(nv_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(lib.OPTIM_SIGNATURES) == {"nv_adamw_master", "nv_adamw_sr"}
    assert not declared & set(lib.SIGNATURES) and not declared & set(lib.TOPP_SIGNATURES)
    assert len(lib.SIGNATURES) == 119 and len(lib.TOPP_SIGNATURES) == 2
    for name in declared:                              # argument counts of the declarations = those of the table
        args = re.search(name + r"\s*\(([^)]*)\)", hdr).group(1)
        assert len(args.split(",")) == len(lib.OPTIM_SIGNATURES[name][1]), name
    L = lib.load()                                     # binds all three tables: raises when the library does not export a name
    assert all(hasattr(L, n) for n in declared)


def test_argument_errors_return_before_any_launch():
    """null pointers, step < 1, negative n / elem0: -1; n == 0: 0.  No device is touched (the pointer values are never dereferenced)."""
    from navillm_amd import lib
    L = lib.load()
    one = 1 << 12
    h = (1e-5, 0.9, 0.999, 1e-8, 0.01)
    master = dict(p=one, g=one, master=one, m=one, v=one, n=16)
    sr = dict(p=one, g=one, m=one, v=one, n=16, elem0=0, seed=0)
    call_m = lambda a, step=1: L.nv_adamw_master(*a.values(), *h, step, None, 1, None)
    call_s = lambda a, step=1: L.nv_adamw_sr(*a.values(), *h, step, None, 1, None)
    for k in ("p", "g", "master", "m", "v"):
        assert call_m(dict(master, **{k: None})) == -1, k
    for k in ("p", "g", "m", "v"):
        assert call_s(dict(sr, **{k: None})) == -1, k
    for step in (0, -3):
        assert call_m(master, step) == -1 and call_s(sr, step) == -1
    assert call_m(dict(master, n=-1)) == -1 and call_s(dict(sr, n=-1)) == -1 and call_s(dict(sr, elem0=-8)) == -1
    assert call_m(dict(master, n=0)) == 0 and call_s(dict(sr, n=0)) == 0
    assert call_m(dict(master, n=0), 0) == -1          # (the argument check comes first)


class _ParamModel(torch.nn.Module):
    """FlatStore on the CPU + nn.Parameters that are views into it (what NavModel builds on the GPU)"""

    def __init__(self, cfg):
        super().__init__()
        from navillm_amd.flat import FlatStore
        from navillm_amd.params import param_specs
        self.cfg, self.store = cfg, FlatStore(cfg, "cpu")
        self._dp = None
        self.plist = torch.nn.ParameterList([torch.nn.Parameter(self.store.p(n)) for n, _, _ in param_specs(cfg)])


def test_state_precision_argument_and_environment(monkeypatch):
    from navillm_amd.optim import FlatAdamW, STATE_PRECISIONS
    cfg = tiny_cfg("bf16")
    monkeypatch.delenv("NAVILLM_ADAMW_STATE", raising=False)
    opt = FlatAdamW(_ParamModel(cfg), lr=1e-5)
    assert opt.state_precision == "bf16" and opt.sr_seed == 0 and opt.store.master is None
    assert opt.store.exp_avg["lm"].dtype == torch.bfloat16 and opt.store.exp_avg["f32"].dtype == torch.float32
    for bad in ("fp32", "BF16", "", "sr", 32):
        with pytest.raises(ValueError, match="state_precision"):
            FlatAdamW(_ParamModel(cfg), lr=1e-5, state_precision=bad)
    for mode in STATE_PRECISIONS:
        monkeypatch.setenv("NAVILLM_ADAMW_STATE", mode)
        assert FlatAdamW(_ParamModel(cfg), lr=1e-5).state_precision == mode               # the environment sets the default
        for explicit in STATE_PRECISIONS:
            assert FlatAdamW(_ParamModel(cfg), lr=1e-5, state_precision=explicit).state_precision == explicit      # the argument wins
    monkeypatch.setenv("NAVILLM_ADAMW_STATE", "float32")
    with pytest.raises(ValueError, match="NAVILLM_ADAMW_STATE"):
        FlatAdamW(_ParamModel(cfg), lr=1e-5)
    assert FlatAdamW(_ParamModel(cfg), lr=1e-5, state_precision="stochastic", sr_seed=7).sr_seed == 7
    # buffers per mode; an fp32 LM already has fp32 parameters and moments: nothing to add in any mode
    st = FlatAdamW(_ParamModel(cfg), lr=1e-5, state_precision="fp32_master").store
    assert st.exp_avg["lm"].dtype == st.exp_avg_sq["lm"].dtype == st.master["lm"].dtype == torch.float32
    assert st.master["lm"].shape == st.param["lm"].shape and not st.master["lm"].any() and set(st.master) == {"lm"}
    st = FlatAdamW(_ParamModel(cfg), lr=1e-5, state_precision="stochastic").store
    assert st.exp_avg["lm"].dtype == torch.bfloat16 and st.master is None
    st = FlatAdamW(_ParamModel(tiny_cfg("fp32")), lr=1e-5, state_precision="fp32_master").store
    assert st.exp_avg["lm"].dtype == torch.float32 and st.master is None
    # the release paths drop the master with the moments
    for release in ("release_grads", "release_decoder_layers_and_grads"):
        m = _ParamModel(cfg)
        FlatAdamW(m, lr=1e-5, state_precision="fp32_master")
        getattr(m.store, release)({})
        assert m.store.master is None and m.store.exp_avg is None and m.store.exp_avg_sq is None


def _filled(mode, seed, sr_seed=0):
    """an optimizer of `mode` on the CPU whose moments (and master) hold values that are NOT bf16 numbers where the buffer is fp32"""
    from navillm_amd.optim import FlatAdamW
    m = _ParamModel(tiny_cfg("bf16"))
    opt = FlatAdamW(m, lr=3e-5, state_precision=mode, sr_seed=sr_seed)
    gen = torch.Generator().manual_seed(seed)
    st = m.store
    st.param["lm"].copy_(torch.randn(st.total["lm"], generator=gen) * 0.02)
    for buf in (st.exp_avg, st.exp_avg_sq) + ((st.master,) if st.master is not None else ()):
        for t in buf.values():
            t.copy_(torch.rand(t.shape, generator=gen) * 1e-3 + 1e-6)
    st.touch_layers()
    opt.born, opt.step_count = {n: 0 for n in st.touched}, 4
    return opt


def test_state_dicts_convert_between_precisions():
    lm = lambda opt, key: getattr(opt.store, key)["lm"]
    src = {mode: _filled(mode, 1, sr_seed=5) for mode in ("bf16", "fp32_master", "stochastic")}
    sds = {mode: o.state_dict() for mode, o in src.items()}
    for mode, sd in sds.items():
        assert sd["state_precision"] == mode and sd["sr_seed"] == 5 and ("master" in sd) == (mode == "fp32_master")
        assert sd["exp_avg"]["lm"].data_ptr() != lm(src[mode], "exp_avg").data_ptr()
    assert sds["fp32_master"]["master"]["lm"].dtype == torch.float32 and sds["fp32_master"]["master"]["lm"].data_ptr() != src["fp32_master"].store.master["lm"].data_ptr()
    for a, sd in sds.items():
        for b in src:
            dst = _filled(b, 2)
            dst.load_state_dict(sd)
            assert dst.state_precision == b and dst.sr_seed == 5 and dst.step_count == 4 and dst.born == src[a].born
            want_dt = torch.float32 if b == "fp32_master" else torch.bfloat16
            for key in ("exp_avg", "exp_avg_sq"):
                got = lm(dst, key)
                assert got.dtype == want_dt
                # bf16 -> fp32: the exact upcast; fp32 -> bf16: round to nearest even; same precision: the same bits
                assert torch.equal(got, sd[key]["lm"].to(want_dt)), (a, b, key)
                assert torch.equal(getattr(dst.store, key)["f32"], sd[key]["f32"])
            if b == "fp32_master":
                # the saved master, or zeros = "adopt the parameter at the next step" (never the stale master of the loading optimizer)
                assert torch.equal(dst.store.master["lm"], sd["master"]["lm"]) if a == "fp32_master" else not dst.store.master["lm"].any()
            else:
                assert dst.store.master is None
    rounded = sds["fp32_master"]["exp_avg"]["lm"].to(torch.bfloat16)
    assert not torch.equal(rounded.float(), sds["fp32_master"]["exp_avg"]["lm"])             # (the RNE above was a real rounding)


def test_reference_format_state_in_every_mode():
    """the reference's torch.optim.AdamW entry loads into each mode (moments = the upcast values), and `reference_state_dict()` writes
    the LM moments in bf16 whatever the mode: the reference's parameters dictate the dtype"""
    ref_sd = _filled("bf16", 3).reference_state_dict()
    assert all(e["exp_avg"].dtype in (torch.bfloat16, torch.float32) for e in ref_sd["state"].values())
    for mode in ("bf16", "fp32_master", "stochastic"):
        dst = _filled(mode, 4)
        dst.load_state_dict(ref_sd)
        st = dst.store
        assert dst.step_count == 4 and dst.state_precision == mode
        assert st.exp_avg["lm"].dtype == (torch.float32 if mode == "fp32_master" else torch.bfloat16)
        from navillm_amd.optim import reference_param_orders
        order = reference_param_orders(st.cfg)[0]
        for k, ent in ref_sd["state"].items():
            for key, buf in (("exp_avg", st.exp_avg), ("exp_avg_sq", st.exp_avg_sq)):
                v = st._view(buf, order[k])
                assert torch.equal(v, ent[key].to(v.dtype)), (mode, order[k], key)
        if mode == "fp32_master":
            assert not st.master["lm"].any()
        out = dst.reference_state_dict()
        for k, ent in ref_sd["state"].items():
            assert out["state"][k]["exp_avg"].dtype == ent["exp_avg"].dtype and torch.equal(out["state"][k]["exp_avg"], ent["exp_avg"])
            assert torch.equal(out["state"][k]["exp_avg_sq"], ent["exp_avg_sq"])
    # fp32 moments that are not bf16 numbers leave as their RNE rounding
    src = _filled("fp32_master", 5)
    out = src.reference_state_dict()
    name = "lang_model.model.layers.0.self_attn.q_proj.weight"
    k = reference_param_orders(src.store.cfg)[0].index(name)
    want = src.store._view(src.store.exp_avg, name).to(torch.bfloat16)
    assert out["state"][k]["exp_avg"].dtype == torch.bfloat16 and torch.equal(out["state"][k]["exp_avg"], want)


# ---------------------------------------------------------------- the fixture check of tests/test_adamw_modes_gpu.py
def test_philox_emulation_known_answers():
    """Random123's known-answer vectors for philox4x32_10, and the counter layout of the header"""
    out = [int(x) for x in R.philox4x32_10(0, 0, 0, 0, 0, 0)]
    assert out == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    out = [int(x) for x in R.philox4x32_10(0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff)]
    assert out == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    e = np.arange(16, 32)
    r = R.sr_bits(9, 3, e, 2)
    w = [int(x) for x in R.philox4x32_10(2, 0, 3, 2, 9, 0)]                # group 2 = elements 16..23
    assert [int(x) for x in r[:8]] == [w[0] & 0xffff, w[0] >> 16, w[1] & 0xffff, w[1] >> 16, w[2] & 0xffff, w[2] >> 16, w[3] & 0xffff, w[3] >> 16]
    assert not np.array_equal(r[:8], r[8:]) and not np.array_equal(r, R.sr_bits(9, 3, e, 1)) and not np.array_equal(r, R.sr_bits(9, 4, e, 2))
    # the store: representable values unchanged whatever the bits; otherwise one of the two neighbours
    x = np.array([1.0, -0.5, 1.001953125, -1.001953125], dtype=np.float32)
    assert R.sr_store(x, [0xffff] * 4).tolist() == [1.0, -0.5, 1.0078125, -1.0078125]
    assert R.sr_store(x, [0] * 4).tolist() == [1.0, -0.5, 1.0, -1.0]


@pytest.mark.parametrize("nsteps", [1, 5])
def test_fixture_fp32_references_meet_the_exactness_cap(nsteps):
    """item 1 of the GPU file on the host: a correct fp32 evaluation (numpy, plain and with contracted multiply-adds) of the chosen
    inputs stays under 4 * err(torch fp32 AdamW) + 2^-24 * max|.| against the fp64 reference, for p, m and v at every size"""
    for n in R.SIZES:
        p, g = R.inputs(n)
        ref = R.adamw_run(p, g, nsteps, R.LR, coef=R.COEF)
        tor = R.torch_adamw(p, g, nsteps, R.LR, coef=R.COEF)
        for fma in (False, True):
            got = R.adamw_run(p, g, nsteps, R.LR, coef=R.COEF, dtype=np.float32, fma=fma)
            for name, a, t, r in zip("pmv", got, tor, ref):
                assert R.maxerr(a, r) <= R.fp32_cap(R.maxerr(t, r), r), (n, fma, name)
        assert R.maxerr(R.rne_bf16(p), p) == 0 and np.abs(ref[0] - p).max() > 0


def test_fixture_drift_references():
    """item 2: over 200 steps at lr 1e-5 with the constant gradient the fp64 reference displaces the mean weight by -2.0e-3 (1 %), an
    fp32 evaluation follows it within 1 %, and torch's own bf16 AdamW -- what the "bf16" mode reproduces -- delivers under 25 % of it"""
    D = R.DRIFT
    p, _ = R.inputs(4096, seed=1)
    g = R.rne_bf16(np.full(4096, D["g"], dtype=np.float32))
    ref = (R.adamw_run(p, g, D["steps"], D["lr"], D["wd"])[0] - p).mean()
    assert abs(ref / -2.0e-3 - 1) < 0.01, ref
    f32 = (R.adamw_run(p, g, D["steps"], D["lr"], D["wd"], dtype=np.float32, fma=True)[0].astype(np.float64) - p).mean()
    assert abs(f32 / ref - 1) < 0.01
    b16 = (R.torch_adamw(p, g, D["steps"], D["lr"], D["wd"], dtype=torch.bfloat16)[0] - p).mean()
    print(f"[drift] fp64 {ref:.4e}  fp32 {f32:.4e}  bf16 {b16:.4e} = {b16 / ref:.1%}")
    assert 0 < b16 / ref < 0.25


def test_fixture_stochastic_emulation_bracket_unbiasedness_and_drift():
    """items 4, 5 and 7 on the numpy emulation: the stored values bracket the fp64 reference within one bf16 spacing, the fractions
    rounded up are 0.25 and 0.5 within 6 sigma with the very Philox bits the device draws (seed 0, step 1), and 200 emulated steps
    drift within 5 % of the fp64 reference"""
    p, g = R.inputs(2051)
    one = R.sr_adamw_run(p, g, 1, R.LR, R.WD)
    ref = R.adamw_step(p, g, np.zeros(2051), np.zeros(2051), 1, R.LR, R.WD)
    for got, r in zip(one, ref):
        assert np.all(np.abs(got.astype(np.float64) - r) <= R.bf16_spacing(r) * (1 + 2.0 ** -10))
    n = 1 << 20
    for gsign, lo, hi, frac in ((-1.0, 1.0, 1.0078125, 0.25), (1.0, 0.99609375, 1.0, 0.5)):
        out = R.sr_adamw_run(np.ones(n, np.float32), np.full(n, gsign, np.float32), 1, 2.0 ** -9, 0.0)[0]
        assert set(np.unique(out).tolist()) == {lo, hi}
        six_sigma = 6 * np.sqrt(frac * (1 - frac) / n)
        assert abs((out == hi).mean() - frac) <= six_sigma, (gsign, (out == hi).mean())
    assert abs(6 * np.sqrt(0.25 * 0.75 / n) - 0.0026) < 1e-4
    D = R.DRIFT
    p, _ = R.inputs(65536, seed=2)
    g = R.rne_bf16(np.full(65536, D["g"], dtype=np.float32))
    ref = (R.adamw_run(p, g, D["steps"], D["lr"], D["wd"])[0] - p).mean()
    emu = (R.sr_adamw_run(p, g, D["steps"], D["lr"], D["wd"], fma=False)[0].astype(np.float64) - p).mean()
    print(f"[stochastic drift] fp64 {ref:.5e}  emulation {emu:.5e}  ({emu / ref - 1:+.3%})")
    assert abs(emu / ref - 1) < 0.05
