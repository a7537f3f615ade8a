"""Host references for the AdamW state-precision modes (navillm_amd/csrc/adamw_hp.hip, include/navillm_hip_optim.h): the update in
numpy fp64 (the reference of every bound), the same in numpy fp32 (what a correct fp32 kernel computes, with or without contracted
multiply-adds), torch's own fp32 AdamW on the CPU (the yardstick of the fp32 error), Philox4x32-10 with the header's counter layout
and the stochastic bf16 store.  Shared by tests/test_adamw_modes_cpu.py (which checks that the references themselves meet the caps
the GPU tests assert) and tests/test_adamw_modes_gpu.py; the inputs of both come from `inputs()`."""
import functools
import math

import numpy as np
import torch

BETAS, EPS = (0.9, 0.999), 1e-8
SIZES = (1, 7, 8, 9, 2051, 8 * 256 * 3 + 5)
COEF = float(np.float32(0.37))                    # the clip vector's coefficient as the device reads it (fp32)
WD = 0.01
LR = 1e-5                                         # the reference's setting (tools/parser.py:39): where the feature matters
DRIFT = dict(lr=1e-5, g=1e-3, steps=200, wd=0.01)  # "the point of the feature": constant gradient, N(0, 0.02) weights
M32 = np.uint64(0xFFFFFFFF)


# ---------------------------------------------------------------- bf16 <-> fp32 on the host
def bf16_bits(x):
    """fp32 array -> bf16 bit patterns (uint16), round to nearest even (finite inputs)"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return (((u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)) & np.uint64(0xFFFF)).astype(np.uint16)


def bits_to_f32(b):
    return (np.asarray(b).astype(np.uint32) << np.uint32(16)).view(np.float32)


def rne_bf16(x):
    return bits_to_f32(bf16_bits(x))


def bf16_spacing(x):
    """distance between neighbouring bf16 numbers at the magnitude of x (normal range)"""
    a = np.abs(np.asarray(x, dtype=np.float64))
    return 2.0 ** (np.floor(np.log2(np.maximum(a, 2.0 ** -126))) - 7)


def t_bf16(a):
    """numpy array of bf16-representable fp32 values -> torch bf16 tensor"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16)


def np_f32(t):
    return t.detach().float().cpu().numpy()


# ---------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def inputs(n, seed=0):
    """(p, g): bf16-representable fp32 arrays, N(0, 0.02) weights and N(0, 1e-3) gradients"""
    r = np.random.RandomState(1000 + seed)
    p = rne_bf16((r.randn(n) * 0.02).astype(np.float32))
    g = rne_bf16((r.randn(n) * 1e-3).astype(np.float32))
    p.setflags(write=False)
    g.setflags(write=False)
    return p, g


# ---------------------------------------------------------------- the update
def scalars(step, lr, wd, betas=BETAS, eps=EPS):
    """the hyper-parameter scalars in double, as the launchers prepare them"""
    b1, b2 = betas
    return dict(decay=1.0 - lr * wd, w1=1.0 - b1, b2=b2, w2=1.0 - b2, eps=eps, step_size=lr / (1.0 - b1 ** step),
                sqrt_bc2=math.sqrt(1.0 - b2 ** step))


def adamw_step(p, g, m, v, step, lr, wd=WD, coef=1.0, dtype=np.float64, fma=False):
    """one element-wise update by the header's formula -> (p, m, v).  dtype=float64: the reference.  dtype=float32: every scalar rounded
    to fp32 once and every operation rounded to fp32 (numpy); fma=True evaluates a*b+c with one rounding where a compiler may contract."""
    T = dtype
    s = {k: T(x) for k, x in scalars(step, lr, wd).items()}
    p, g, m, v = (np.asarray(a).astype(T) for a in (p, g, m, v))
    wide = lambda x: np.asarray(x).astype(np.float64)
    if fma:
        muladd = lambda a, b, c: (wide(a) * wide(b) + wide(c)).astype(T)
    else:
        muladd = lambda a, b, c: a * b + c
    g = g * T(coef)
    p = p * s["decay"]
    m = muladd(s["w1"], g - m, m)
    v = muladd(s["w2"] * g, g, s["b2"] * v)
    den = np.sqrt(v) / s["sqrt_bc2"] + s["eps"]
    p = p - s["step_size"] * m / den
    assert p.dtype == T and m.dtype == T and v.dtype == T
    return p, m, v


def adamw_run(p, g, nsteps, lr, wd=WD, coef=1.0, dtype=np.float64, fma=False, m=None, v=None, step0=0):
    """nsteps updates with the same gradient from zero (or the given) moments -> (p, m, v)"""
    m = np.zeros_like(p, dtype=dtype) if m is None else m
    v = np.zeros_like(p, dtype=dtype) if v is None else v
    p = np.asarray(p).astype(dtype)
    for k in range(nsteps):
        p, m, v = adamw_step(p, g, m, v, step0 + k + 1, lr, wd, coef, dtype, fma)
    return p, m, v


def torch_adamw(p, g, nsteps, lr, wd=WD, coef=1.0, dtype=torch.float32):
    """torch.optim.AdamW on the CPU with parameter (and so moments) of `dtype`; the gradient is float(g) * coef rounded to `dtype`
    -> (p, m, v) as fp64 numpy"""
    w = torch.nn.Parameter(torch.from_numpy(np.array(p, dtype=np.float32)).to(dtype))       # (a copy: the step is in place)
    opt = torch.optim.AdamW([w], lr=lr, betas=BETAS, eps=EPS, weight_decay=wd)
    grad = (torch.from_numpy(np.array(g, dtype=np.float32)) * torch.tensor(coef, dtype=torch.float32)).to(dtype)
    for _ in range(nsteps):
        w.grad = grad.clone()
        opt.step()
    st = opt.state[w]
    return tuple(t.detach().double().numpy() for t in (w, st["exp_avg"], st["exp_avg_sq"]))


def maxerr(a, ref):
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(ref, dtype=np.float64)))) if np.size(ref) else 0.0


def fp32_cap(err_torch, ref):
    """the cap of an fp32 result's error: four times torch's own fp32 error (another, equally valid evaluation order) plus half a
    spacing of fp32 at the largest magnitude"""
    return 4.0 * err_torch + 2.0 ** -24 * float(np.max(np.abs(ref)))


# ---------------------------------------------------------------- Philox4x32-10 and the stochastic store
def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """vectorised over uint64 arrays holding 32-bit words -> four arrays of 32-bit words"""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & M32 for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = np.uint64(k0) & M32, np.uint64(k1) & M32
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ k0) & M32, p1 & M32, ((p0 >> np.uint64(32)) ^ c3 ^ k1) & M32, p0 & M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def sr_bits(seed, step, elem, array):
    """the 16 random bits of global element `elem` (array of indices) of array 0: p, 1: m, 2: v (include/navillm_hip_optim.h)"""
    e = np.asarray(elem, dtype=np.uint64)
    grp, inv = np.unique(e >> np.uint64(3), return_inverse=True)          # one Philox block per group of 8 elements
    out = philox4x32_10(grp & M32, grp >> np.uint64(32), np.uint64(step), np.uint64(array), np.uint64(seed) & M32, np.uint64(seed) >> np.uint64(32))
    word = ((e & np.uint64(7)) >> np.uint64(1)).astype(np.int64)
    w = np.stack(out)[word, inv.reshape(e.shape)]
    return (w >> (np.uint64(16) * (e & np.uint64(1)))) & np.uint64(0xFFFF)


def sr_store(x, r):
    """finite fp32 values + 16 random bits each -> the stored bf16 values (as fp32)"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return bits_to_f32(((u + np.asarray(r, dtype=np.uint64)) >> np.uint64(16)) & np.uint64(0xFFFF))


def sr_adamw_run(p, g, nsteps, lr, wd, seed=0, elem0=0, fma=True):
    """emulation of `nsteps` stochastic-mode updates (fp32 arithmetic from the stored bf16 state) -> (p, m, v)"""
    p = np.asarray(p, dtype=np.float32)
    m, v = np.zeros_like(p), np.zeros_like(p)
    e = elem0 + np.arange(p.size)
    for k in range(1, nsteps + 1):
        pf, mf, vf = adamw_step(p, g, m, v, k, lr, wd, 1.0, np.float32, fma)
        p, m, v = (sr_store(x, sr_bits(seed, k, e, a)) for a, x in enumerate((pf, mf, vf)))
    return p, m, v
