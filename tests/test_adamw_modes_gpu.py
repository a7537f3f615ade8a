"""GPU: nv_adamw_master and nv_adamw_sr (navillm_amd/csrc/adamw_hp.hip) against the fp64 AdamW of tests/optim_ref.py.

Every bound comes from the reference side: the fp32 cap is four times the error of torch's own fp32 AdamW on the CPU plus half an fp32
spacing (tests/test_adamw_modes_cpu.py checks that plain and contracted fp32 evaluations of the same inputs stay under it), the
stochastic bracket is one bf16 spacing plus four fp32 spacings of evaluation error, the unbiasedness window is 6 sigma of the binomial.
Sizes: 1, 7, 8, 9 (around one 8-element vector), 2051 (vector path + tail of 3), 8*256*3 + 5 (three blocks + tail) and a view that starts
one element into an aligned buffer (the scalar path for everything).  Each buffer sits between canaries."""
import numpy as np
import pytest
import torch

import optim_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 64
CASES = [(n, 0) for n in R.SIZES] + [(2051, 1)]                  # (n, offset of the view from a 128-byte aligned address)
CANARY = 3.0


class Buf:
    """a device array of n elements between two canaries, `off` elements past an aligned address"""

    def __init__(self, host, dtype, off=0):
        host = np.asarray(host, dtype=np.float32)
        self.full = torch.full((PAD + off + host.size + PAD,), CANARY, dtype=dtype, device=DEV)
        self.t = self.full[PAD + off:PAD + off + host.size]
        assert self.full.data_ptr() % 128 == 0
        self.t.copy_(torch.from_numpy(host.copy()).to(dtype))
        self.lo, self.hi = self.full[:PAD + off], self.full[PAD + off + host.size:]

    def intact(self):
        return bool((self.lo == CANARY).all()) and bool((self.hi == CANARY).all())

    def np(self):
        return self.t.detach().float().cpu().numpy()


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def clip_vec(coef):
    return torch.tensor([123.0, coef], dtype=torch.float32, device=DEV)


@pytest.fixture(scope="module")
def ops():
    from navillm_amd import ops
    return ops


# ---------------------------------------------------------------- 1. fp32_master exactness
@pytest.mark.parametrize("zero_grad", [False, True])
@pytest.mark.parametrize("nsteps", [1, 5])
@pytest.mark.parametrize("n,off", CASES)
def test_master_exactness(ops, n, off, nsteps, zero_grad):
    """after each step p == RNE_bf16(master) bit for bit and g is zero when asked; after the last, err(x) = max|x - fp64 reference| obeys
    err(device) <= 4 * err(torch fp32 AdamW on the CPU) + 2^-24 * max|x| for x = master, m, v.  The master starts as zeros: the first
    step adopts the weights (self-healing).  Measured ratios err(device) / err(torch): printed, recorded in DESIGN.md."""
    p0, g0 = R.inputs(n)
    p, g = Buf(p0, torch.bfloat16, off), Buf(g0, torch.bfloat16, off)
    w, m, v = (Buf(np.zeros(n), torch.float32, off) for _ in range(3))
    clip = clip_vec(R.COEF)
    for k in range(1, nsteps + 1):
        g.t.copy_(R.t_bf16(g0))
        ops.adamw_master_(p.t, g.t, w.t, m.t, v.t, k, R.LR, wd=R.WD, clip=clip, zero_grad=zero_grad)
        assert torch.equal(bits(p.t), bits(w.t.to(torch.bfloat16))), f"step {k}: p is not RNE_bf16(master)"
        assert torch.equal(g.t, torch.zeros_like(g.t) if zero_grad else R.t_bf16(g0).to(DEV)), f"step {k}: gradient"
    assert all(b.intact() for b in (p, g, w, m, v)), "a write outside the arrays"
    ref = R.adamw_run(p0, g0, nsteps, R.LR, coef=R.COEF)
    tor = R.torch_adamw(p0, g0, nsteps, R.LR, coef=R.COEF)
    for name, got, t, r in zip(("master", "m", "v"), (w.np(), m.np(), v.np()), tor, ref):
        e_dev, e_tor = R.maxerr(got, r), R.maxerr(t, r)
        print(f"[master n={n} off={off} steps={nsteps}] {name}: err device {e_dev:.3e}  torch fp32 {e_tor:.3e}  ratio {e_dev / max(e_tor, 1e-300):.2f}"
              f"  cap {R.fp32_cap(e_tor, r):.3e}")
        assert e_dev <= R.fp32_cap(e_tor, r), (name, e_dev, e_tor)


# ---------------------------------------------------------------- 2. the point of the feature
def test_master_trains_where_bf16_state_stalls(ops):
    """200 steps at lr 1e-5 with the constant gradient 1e-3 on 4096 N(0, 0.02) weights: "fp32_master" displaces the mean weight to within
    1 % of the fp64 reference's -2.0e-3; the reference-exact bf16 kernel on the same inputs delivers under 25 % of it (torch's own bf16
    AdamW on the CPU: 13.5 %, tests/test_adamw_modes_cpu.py)."""
    D = R.DRIFT
    n = 4096
    p0, _ = R.inputs(n, seed=1)
    g0 = R.rne_bf16(np.full(n, D["g"], dtype=np.float32))
    ref = (R.adamw_run(p0, g0, D["steps"], D["lr"], D["wd"])[0] - p0).mean()
    assert abs(ref / -2.0e-3 - 1) < 0.01
    p, g = Buf(p0, torch.bfloat16), Buf(g0, torch.bfloat16)
    w, m, v = (Buf(np.zeros(n), torch.float32) for _ in range(3))
    q, mq, vq = Buf(p0, torch.bfloat16), Buf(np.zeros(n), torch.bfloat16), Buf(np.zeros(n), torch.bfloat16)
    for k in range(1, D["steps"] + 1):
        ops.adamw_master_(p.t, g.t, w.t, m.t, v.t, k, D["lr"], wd=D["wd"])
        ops.adamw_(q.t, g.t, mq.t, vq.t, k, D["lr"], wd=D["wd"])
    master = (w.np().astype(np.float64) - p0).mean()
    seen = (p.np().astype(np.float64) - p0).mean()                 # (printed only: every weight moved by the same amount off its grid point,
                                                                   # so the bf16 roundings of the masters share one residual per binade)
    bf16 = (q.np().astype(np.float64) - p0).mean()
    print(f"[drift] fp64 {ref:.5e}  fp32_master {master:.5e} ({master / ref - 1:+.3%}; bf16 view {seen / ref - 1:+.3%})  bf16 kernel {bf16:.5e} = {bf16 / ref:.1%}")
    assert abs(master / ref - 1) < 0.01
    assert 0 <= bf16 / ref < 0.25
    assert all(b.intact() for b in (p, g, w, m, v, q, mq, vq))


# ---------------------------------------------------------------- 3. self-healing master
def test_master_self_healing(ops):
    """p overwritten between two steps: the second step's result is the fp64 update started from the NEW p (with the first step's
    moments); untouched elements continue from their fp32 master, sub-bf16 bits included.  Cap: the form of item 1 with the numpy fp32
    evaluation of the same step as the yardstick (bit-identical to torch's CPU result where both exist, tests/test_adamw_modes_cpu.py)."""
    n = 2051
    p0, g0 = R.inputs(n)
    p, g = Buf(p0, torch.bfloat16), Buf(g0, torch.bfloat16)
    w, m, v = (Buf(np.zeros(n), torch.float32) for _ in range(3))
    lr = 1e-3                                                      # (a step large enough that the master leaves the bf16 grid everywhere)
    ops.adamw_master_(p.t, g.t, w.t, m.t, v.t, 1, lr, wd=R.WD)
    w1, m1, v1 = w.np(), m.np(), v.np()
    assert (w1 != R.rne_bf16(w1)).mean() > 0.9                     # the masters carry bits below bf16
    hit = np.zeros(n, dtype=bool)
    hit[::3] = True
    hit[-1] = True                                                 # (one in the scalar tail)
    new = R.inputs(n, seed=7)[0]
    idx = torch.from_numpy(np.flatnonzero(hit)).to(DEV)
    p.t[idx] = R.t_bf16(new[hit]).to(DEV)                          # an external write: no hook, no call into the optimizer
    ops.adamw_master_(p.t, g.t, w.t, m.t, v.t, 2, lr, wd=R.WD)
    adopted = hit & (new != R.rne_bf16(w1))                         # (a new value that IS the master's rounding changes nothing)
    assert adopted.sum() > 0.99 * hit.sum()
    start = np.where(adopted, new, w1)
    ref = R.adamw_step(start, g0, m1, v1, 2, lr, R.WD)
    f32 = R.adamw_step(start, g0, m1, v1, 2, lr, R.WD, dtype=np.float32, fma=True)
    for name, got, a, r in zip(("master", "m", "v"), (w.np(), m.np(), v.np()), f32, ref):
        assert R.maxerr(got, r) <= R.fp32_cap(R.maxerr(a, r), r), name
    # had the untouched elements restarted from their bf16 parameter, they would be off by the sub-bf16 part: orders above the cap
    lost = np.abs(R.adamw_step(R.rne_bf16(w1), g0, m1, v1, 2, lr, R.WD)[0] - ref[0])[~hit]
    assert np.median(lost) > 100 * R.fp32_cap(R.maxerr(f32[0], ref[0]), ref[0])
    assert torch.equal(bits(p.t), bits(w.t.to(torch.bfloat16))) and all(b.intact() for b in (p, g, w, m, v))


# ---------------------------------------------------------------- 4. stochastic bracket
def bracket_ok(stored, ref):
    """one bf16 spacing (the store picks one of the two neighbours of the fp32 result) + 4 fp32 spacings of evaluation error"""
    tol = R.bf16_spacing(np.maximum(np.abs(ref), np.abs(stored))) + 2.0 ** -21 * np.abs(ref)
    return np.abs(stored.astype(np.float64) - ref) <= tol


@pytest.mark.parametrize("zero_grad", [False, True])
@pytest.mark.parametrize("n,off", CASES)
def test_stochastic_bracket(ops, n, off, zero_grad):
    """five steps; every stored p, m, v lies within one bf16 spacing of the fp64 update of THAT step (started from the state the device
    stored at the step before), and the stores actually round both ways"""
    p0, g0 = R.inputs(n)
    p, g = Buf(p0, torch.bfloat16, off), Buf(g0, torch.bfloat16, off)
    m, v = Buf(np.zeros(n), torch.bfloat16, off), Buf(np.zeros(n), torch.bfloat16, off)
    clip = clip_vec(R.COEF)
    up = tot = 0
    for k in range(1, 6):
        before = (p.np(), m.np(), v.np())
        g.t.copy_(R.t_bf16(g0))
        ops.adamw_sr_(p.t, g.t, m.t, v.t, k, R.LR, wd=R.WD, clip=clip, zero_grad=zero_grad, elem0=off, seed=11)
        ref = R.adamw_step(before[0], g0, before[1], before[2], k, R.LR, R.WD, coef=R.COEF)
        for name, got, r in zip("pmv", (p.np(), m.np(), v.np()), ref):
            ok = bracket_ok(got, r)
            assert ok.all(), (k, name, int((~ok).sum()))
            up += int((np.abs(got) > np.abs(r)).sum())
            tot += got.size
        assert torch.equal(g.t, torch.zeros_like(g.t) if zero_grad else R.t_bf16(g0).to(DEV))
    assert all(b.intact() for b in (p, g, m, v))
    if n >= 2051:
        assert 0.3 < up / tot < 0.7, up / tot                        # away from zero about half the time (RNE would do so too; truncation not)


@pytest.mark.parametrize("n,off", CASES)
def test_stochastic_store_keeps_representable_values(ops, n, off):
    """g = 0, zero moments, wd = 0: every fp32 result is the bf16 input itself (p * 1 - s * 0 / eps, 0, 0) and is stored exactly,
    whatever the random bits"""
    p0, _ = R.inputs(n)
    p, g = Buf(p0, torch.bfloat16, off), Buf(np.zeros(n), torch.bfloat16, off)
    m, v = Buf(np.zeros(n), torch.bfloat16, off), Buf(np.zeros(n), torch.bfloat16, off)
    for seed in (0, 1, 2 ** 40 + 5):
        ops.adamw_sr_(p.t, g.t, m.t, v.t, 3, 1e-3, wd=0.0, elem0=off, seed=seed)
    assert torch.equal(bits(p.t), bits(R.t_bf16(p0).to(DEV))) and not m.t.any() and not v.t.any()
    assert all(b.intact() for b in (p, g, m, v))


# ---------------------------------------------------------------- 5. stochastic unbiasedness
@pytest.mark.parametrize("gsign,lo,hi,frac", [(-1.0, 1.0, 1.0078125, 0.25), (1.0, 0.99609375, 1.0, 0.5)])
def test_stochastic_unbiasedness_and_counter_layout(ops, gsign, lo, hi, frac):
    """2^20 elements p = 1, g = -/+1, wd 0, step 1, lr = 2^-9: the first AdamW step moves by lr (1 - 1e-8) -- a quarter of the spacing
    2^-7 above 1.0, half of the spacing 2^-8 below it.  Every result is one of the two neighbours, and the fraction stored as the upper
    one is 0.25 (0.5) within 6 sigma of the binomial: +-0.0026 (+-0.0029).
    The same run pins the documented counter layout: m = fp32(0.1) * -/+1 and v = fp32(0.001) are exact, so their stored bits must equal
    the numpy emulation's everywhere; p's fp32 value may differ from the emulation's by a few fp32 spacings (contraction), so p must
    agree wherever the random bits are not within 64 of the rounding threshold."""
    n = 1 << 20
    ones = np.ones(n, np.float32)
    p, g = Buf(ones, torch.bfloat16), Buf(gsign * ones, torch.bfloat16)
    m, v = Buf(np.zeros(n), torch.bfloat16), Buf(np.zeros(n), torch.bfloat16)
    lr = 2.0 ** -9
    ops.adamw_sr_(p.t, g.t, m.t, v.t, 1, lr, wd=0.0, elem0=0, seed=0)
    out = p.np()
    assert set(np.unique(out).tolist()) == {lo, hi}
    got = float((out == hi).mean())
    six_sigma = 6 * np.sqrt(frac * (1 - frac) / n)
    print(f"[unbiased g={gsign:+.0f}] fraction stored as {hi}: {got:.5f} (expected {frac} +- {six_sigma:.4f})")
    assert abs(got - frac) <= six_sigma
    pf, mf, vf = R.adamw_step(ones, gsign * ones, np.zeros(n, np.float32), np.zeros(n, np.float32), 1, lr, 0.0, dtype=np.float32, fma=True)
    e = np.arange(n)
    assert np.array_equal(m.np(), R.sr_store(mf, R.sr_bits(0, 1, e, 1))), "m: the counter layout of include/navillm_hip_optim.h"
    assert np.array_equal(v.np(), R.sr_store(vf, R.sr_bits(0, 1, e, 2))), "v: the counter layout of include/navillm_hip_optim.h"
    r = R.sr_bits(0, 1, e, 0).astype(np.int64)
    low = int(pf.view(np.uint32)[0] & 0xFFFF)
    clear = np.abs(r + low - 65536) > 64
    assert clear.mean() > 0.99 and np.array_equal(out[clear], R.sr_store(pf, r)[clear]), "p: the counter layout"
    assert all(b.intact() for b in (p, g, m, v))


# ---------------------------------------------------------------- 6. stochastic determinism
def test_stochastic_determinism_and_launch_cuts(ops):
    n = 8 * 256 * 3 + 5
    p0, g0 = R.inputs(n)

    def run(seed, step, cuts=(), elem0=0):
        p, g = Buf(p0, torch.bfloat16), Buf(g0, torch.bfloat16)
        m, v = Buf(np.zeros(n), torch.bfloat16), Buf(np.zeros(n), torch.bfloat16)
        edges = [0, *cuts, n]
        for a, b in zip(edges[:-1], edges[1:]):
            ops.adamw_sr_(p.t[a:b], g.t[a:b], m.t[a:b], v.t[a:b], step, R.LR, wd=R.WD, elem0=elem0 + a, seed=seed, zero_grad=True)
        assert all(x.intact() for x in (p, g, m, v)) and not g.t.any()
        return torch.cat([bits(p.t), bits(m.t), bits(v.t)])

    base = run(5, 2)
    assert torch.equal(base, run(5, 2)), "the same (seed, step) must give the same bits"
    assert not torch.equal(base, run(6, 2)) and not torch.equal(base, run(5 + 2 ** 32, 2)), "another seed (either key word) must differ"
    assert not torch.equal(base, run(5, 3)), "another step must differ"
    # one launch == two launches at elem0 = 0 and elem0 = k: k = 1000 (the second piece on the vector path), k = 1003 (not a multiple of
    # 8: the second piece on the scalar path), and three pieces
    for cuts in ((1000,), (1003,), (1, 2049)):
        assert torch.equal(base, run(5, 2, cuts)), cuts
    # the bits belong to the GLOBAL index: the same buffer as a piece that starts elsewhere draws other bits
    assert not torch.equal(base, run(5, 2, elem0=8)) and not torch.equal(base, run(5, 2, elem0=2 ** 35))
    assert torch.equal(run(5, 2, elem0=2 ** 35 + 3), run(5, 2, (1000,), elem0=2 ** 35 + 3))      # (high counter word, scalar path)


# ---------------------------------------------------------------- 7. stochastic drift
def test_stochastic_drift_follows_the_reference(ops):
    """the 200 steps of item 2 on 65536 weights: the mean displacement is within 5 % of the fp64 reference's (rounding noise of the mean
    ~2e-6 against a drift of 2e-3; the bias from a noisy v is second order, ~1e-4 relative; the numpy emulation lands at -0.02 %)"""
    D = R.DRIFT
    n = 65536
    p0, _ = R.inputs(n, seed=2)
    g0 = R.rne_bf16(np.full(n, D["g"], dtype=np.float32))
    ref = (R.adamw_run(p0, g0, D["steps"], D["lr"], D["wd"])[0] - p0).mean()
    p, g = Buf(p0, torch.bfloat16), Buf(g0, torch.bfloat16)
    m, v = Buf(np.zeros(n), torch.bfloat16), Buf(np.zeros(n), torch.bfloat16)
    for k in range(1, D["steps"] + 1):
        ops.adamw_sr_(p.t, g.t, m.t, v.t, k, D["lr"], wd=D["wd"], seed=0)
    got = (p.np().astype(np.float64) - p0).mean()
    print(f"[stochastic drift] fp64 {ref:.5e}  device {got:.5e} ({got / ref - 1:+.3%})")
    assert abs(got / ref - 1) < 0.05
    assert all(b.intact() for b in (p, g, m, v))
