"""GPU: every C-ABI entry point of navillm_amd/csrc/enc_f32.hip (the fp32 scene encoder and navigation fusion) against references
that share no code with the kernels (tests/enc_ref.py, checked on the CPU by test_enc_ref_cpu.py).  The raw entries are called
through ops._L() / ops._st(): leading dimensions, base pointers, workspaces and null arguments are the test's.

Two rules hold for every case.  (1) Every output is a refkit.Guarded fp32 view (guard rows, a padded ld where the entry takes one):
nothing outside the documented write set may change a bit; every const input, pad columns included, is snapshotted (ReadOnly) and
compared bit for bit afterwards.  Pad columns of inputs hold NaN, so a read past the logical extent poisons the result.  (2) No
bound holds a number measured on a kernel: a check is bit equality on data that makes the arithmetic exact, or a bound derived
below from the kernel's order of operations with refkit's constants: e = 2^-24 per fp32 rounding, gamma(n) = n e / (1 - n e) for
n roundings in a row, REL_MATH (the stated 4-ulp cap) per expf / erff / rsqrtf / division, TINY where a result may be subnormal,
SECOND = 1.01 for products of two such errors.  Fused multiply-adds only remove roundings, so every bound covers both contractions.

GEMM.  Exact: integers in [-8, 8], bias and C0 below 2^10 -> every partial sum is an integer < 2^24 in any order and split: the
result equals the int64 reference bit for bit, for all enc_ref.GEMM_CASES.  Bounded (randn): v_mfma_f32_16x16x4_f32 is an fma chain,
so a product passes through at most K roundings on its way through the accumulator; the split adds at most ksplit (the reduce
kernel's chain), bias and accumulate 2:  |C - C64| <= SECOND gamma(K + ksplit + 2) (sum_k |a||b| + |bias| + |C0|) + TINY.

LayerNorm forward.  A row sum is ceil(d/256) adds per thread, 6 wave levels, 4 block partials: n_s = ceil(d/256) + 10 roundings.
    mean_k = fl(S / d):        Em = SECOND (gamma(n_s) sum|x| / d + REL_MATH |mean|) + TINY
    t = fl(x - mean_k):        |t - c| <= D = Em + e (|c| + Em),  c = x - mean
    var_k = fl(fl(sum t^2)/d): Ev = SECOND ((gamma(n_s + 1) sum (|c| + D)^2 + sum (2 |c| D + D^2)) / d + REL_MATH var) + TINY
    w = var + eps:             Ew = Ev + e (w + Ev);   the test requires Ew < w (it is, except where the data are degenerate)
    rstd_k = rsqrtf(w_k):      Er = SECOND (Ew / 2 (w - Ew)^-3/2 + REL_MATH rstd) + TINY          (|d/dw w^-1/2| is decreasing)
    y = fl(fl(fl(t r_k) w) + b):  E1 = D (r + Er) + |c| Er + e (|c| + D)(r + Er)
                               Ey = SECOND (|w| E1 + 2 e (|c r w| + |w| E1) + e |b|) + TINY
  and y against ((x - mean_k) rstd_k w + b) in fp64 from the kernel's OWN mean_k, rstd_k: the four roundings of that expression
  only,  SECOND (gamma(4) |c' r_k w| + e |b|) + TINY -- free of the math-function cap; catches a wrong row, column or parameter.
LayerNorm backward (mean, rstd are inputs: their given values are used).  xh = fl(fl(x - mu) rs) (2 roundings), dxh = fl(dy w) (1):
    S1 = sum dxh / d:          E1 = SECOND (gamma(n_s + 1) sum|dxh| / d + REL_MATH |S1|) + TINY
    S2 = sum dxh xh / d:       E2 = SECOND (gamma(n_s + 4) sum|dxh xh| / d + REL_MATH |S2|) + TINY
    dx = fl(rs fl(fl(dxh - s1) - fl(xh s2))): at most 5 roundings on any term:
                               Edx = SECOND |rs| (E1 + |xh| E2 + gamma(6) (|dxh| + |S1| + |xh S2|)) + TINY
    gw = sum_m fl(dy xh) (3 roundings per term), gb = sum_m dy: M terms summed in any tree round at most M - 1 times, + accumulate:
                               Egw = SECOND gamma(M + 5) (sum_m |dy xh| + |gw0|) + TINY,  Egb = SECOND gamma(M + 2) (sum_m |dy| + |gb0|) + TINY
  Exact: integer dy, x - mean in {-1, 0, 1}, rstd = 1: gw, gb are order-free integers, bit for bit.

Attention core (one block per (b, head); lens[b] = 0 is outside the contract: every score of the row is -inf and the kernel yields
NaN -- not tested).  q' = fl(q rsqrtf(hd)), score = hd products and adds:
    Es = SECOND (gamma(hd + 1) + REL_MATH + e) sum_e |q k| / sqrt(hd)
  softmax is shift invariant, so take the kernel's own maximum as the shift: the argument of expf is off by at most
    delta = Es + max_c Es + e ((smax - s) + 4 max_c Es),     rho = SECOND (expm1(delta) + REL_MATH)    relative, per probability
  the row sum is ceil(N/64) lane adds and 6 wave levels (n_w = ceil(N/64) + 6), the reciprocal one REL_MATH, the product one e:
    EP = SECOND (rho + max_c rho + gamma(n_w + 1) + REL_MATH) P + TINY               (a padded key is exactly 0)
  out = sum_j fl(P_j m_j) v_j, m = keep fl(1 / (1 - p)) (REL_MATH + 2 e when p > 0), N roundings:
    Eout = SECOND sum_j |v_j| m_j (EP_j + P_j (gamma(N) + [p > 0] (REL_MATH + 2 e))) + TINY
  backward, for the GIVEN P (an input):  dp = fl(fl(dO . v) m), dot = sum_c dp P, dS = fl(P fl(dp - dot)):
    Edp = SECOND (gamma(hd + 2) + [p > 0] (REL_MATH + 2 e)) m sum_e |dO v|
    Edot = SECOND (sum_c Edp P + gamma(n_w + 1) sum_c |dp| P),     EdS = SECOND P (Edp + Edot + gamma(2) (|dp| + |dot|))
    dq = fl(rsqrtf(hd) sum_j dS k):  Edq = SECOND (sum_j EdS |k| + (gamma(N + 1) + REL_MATH) sum_j |dS k|) / sqrt(hd) + TINY;  dk alike
    dv = sum_j fl(P m) dO:           Edv = SECOND (gamma(N) + [p > 0] (REL_MATH + 3 e)) sum_j P m |dO| + TINY
  Exact: q = 0 -> every score 0, expf(0) = 1, P = 1 / len exact for len a power of two; V holds one integer per key in the column
  (key mod hd) of its head, for one window of hd keys at a time: out = V / len bit for bit, 0 for padded keys.  With dropout the
  same operands make `out != 0` the kept set: it must equal enc_ref.mha_keep on the valid keys.

GELU (order: fl(fl(0.5 v) fl(1 + erff(fl(v c)))), c = fl(1/sqrt 2); u = |v| / sqrt 2):
    Eerf = (2 / sqrt pi) exp(-u^2) gamma(2) u + REL_MATH |erf|            (argument error 2 e u through erf', then the 4-ulp cap)
    Ey = SECOND (|v| / 2 (Eerf + e (1 + erf)) + e |y|) + TINY             absolute in |v|: 1 + erff cancels for v << 0
  backward: cdf = fl(0.5 fl(1 + erff)), pdf = fl(c2 expf(fl(fl(-0.5 v) v))), dx = fl(dy fl(cdf + fl(v pdf))):
    Ecdf = (Eerf + e (1 + erf)) / 2,   Epdf = SECOND pdf (expm1(e v^2 / 2) + REL_MATH + 2 e) + TINY
    Edx = SECOND (|dy| (Ecdf + |v| Epdf + e |v pdf| + e (cdf + |v| pdf)) + e |dx|) + TINY (1 + |dy| (1 + |v|))

Dropout: the kept set equals enc_ref.dropout_keep element for element; kept values are fl(x fl(1 / (1 - p))): bitwise where
1 / (1 - p) is exact (p = 0, 0.5), else within REL_MATH (the division) + e; dropped values are +0.
add / mul / rowscale / gather_add are single roundings: bit equality with float64 -> float32.  colsum, index_sum and the numerators
of masked_mean on integer data: bit equality; masked_mean with a power-of-two count bitwise, else within REL_MATH.  An all-zero
mask row is outside the contract (the kernel divides by zero) and is not tested."""
import math

import numpy as np
import pytest
import torch

import enc_ref as R
from refkit import (F32, F64, I32, E, REL_MATH, TINY, SECOND, NV_ERR_ARG, NV_ERR_SHAPE, Guarded, ReadOnly, gamma, gen, randn, dev, bits_equal,
                    check_bound)
from test_rowops_ref_gpu import L, st, run

pytestmark = pytest.mark.gpu

NAN = float("nan")
CAP = 2048 * 256                                  # grid_for(): 2048 blocks of 256 threads; above it the elementwise kernels stride


def ptr(t):
    return None if t is None else t.data_ptr()


def padded(t, ld, off=0):
    """t [rows, cols] (any device) -> (flat NaN-filled fp32 device buffer, its view [rows, cols] with row stride ld that starts `off`
    elements after the 16-byte aligned base, the address of the view: data_ptr() of an EMPTY view is null)"""
    rows, cols = t.shape
    assert ld >= cols
    buf = torch.full((off + max(rows, 1) * max(ld, 1) + 8,), NAN, dtype=F32, device=dev())
    assert buf.data_ptr() % 16 == 0
    view = torch.as_strided(buf, (rows, cols), (ld, 1), off)
    view.copy_(t.to(F32))
    return buf, view, buf.data_ptr() + 4 * off


def g1(n, init=None):
    """a guarded vector"""
    return Guarded(1, n, dtype=F32, init=None if init is None else init.reshape(1, n))


def assert_bits(got, want, what):
    if not bits_equal(got, want.to(got.device)):
        bad = (got.contiguous().view(torch.int32) != want.to(got.device).contiguous().view(torch.int32))
        i = bad.flatten().nonzero()[0].item()
        raise AssertionError(f"{what}: {int(bad.sum())} of {want.numel()} elements differ bitwise; first at flat index {i}: got "
                             f"{got.flatten()[i].item():.9g} want {want.flatten()[i].item():.9g}")


# ================================================================================================ GEMM
def gemm_launch(c, A, B, bias, C0):
    """one call of nv_gemm_f32_ws on CPU operands in storage orientation -> (Guarded C, plan)"""
    _, _, lda, _, _, ldb, ldc = R.gemm_dims(c)
    plan = R.gemm_case_plan(c)
    Abuf, _, a_addr = padded(A, lda, c.a_off)
    Bbuf, _, b_addr = padded(B, ldb, c.b_off)
    assert a_addr % 16 == (4 * c.a_off) % 16 and b_addr % 16 == (4 * c.b_off) % 16
    biasd = None if bias is None else bias.to(F32).to(dev())
    out = Guarded(max(c.M, 1), max(c.N, 1), dtype=F32, ld=max(c.N, 1) + c.pc, init=C0.to(F32) if c.M and c.N else None)
    ws = None
    if c.ws:
        nbytes = L().nv_gemm_f32_workspace_bytes(c.M, c.N)
        assert nbytes == 8 * c.M * c.N * 4
        ws = g1(max(nbytes // 4, 1))
    ro = ReadOnly(**{k: t for k, t in dict(A=Abuf, B=Bbuf, bias=biasd).items() if t is not None})
    null = c.null
    rc = L().nv_gemm_f32_ws(c.layout, None if null == "A" else a_addr, None if null == "B" else b_addr,
                            None if null == "C" else out.view.data_ptr(), ptr(biasd), c.M, c.N, c.K, lda, ldb, out.geom[1][0], c.acc,
                            None if ws is None else ws.view.data_ptr(), st())
    run(rc, c.name, c.expect)
    written = c.expect == 0 and plan["kernel"] in ("vec", "generic")
    out.check(c.name, (slice(None), slice(None)) if written else (slice(0, 0), slice(0, 0)))
    if ws is not None:
        ws.check(c.name + " workspace", (slice(None), slice(0, plan["ws_floats"] if written else 0)))
    ro.check(c.name)
    return out, plan


@pytest.mark.parametrize("name", [c.name for c in R.GEMM_CASES])
def test_gemm_exact(name):
    c = R.GEMM_BY_NAME[name]
    A, B, bias, C0 = R.gemm_int_operands(c)
    out, plan = gemm_launch(c, A, B, bias, C0)
    if c.expect != 0 or plan["kernel"] == "none":
        return
    want, mag = R.gemm_reference(c, A, B, bias, C0)
    assert int(mag.max()) < R.EXACT_LIMIT
    assert torch.isfinite(out.view).all(), f"{name}: non-finite output (a read of the NaN padding)"
    assert_bits(out.view, want.to(F32), name)


@pytest.mark.parametrize("name", R.GEMM_BOUNDED)
def test_gemm_bounded(name):
    c = R.GEMM_BY_NAME[name]
    a_rows, a_cols, _, b_rows, b_cols, _, _ = R.gemm_dims(c)
    g = R.cpu_gen(R.name_key(name), 2)
    A, B = torch.randn(a_rows, a_cols, generator=g), torch.randn(b_rows, b_cols, generator=g)
    bias = torch.randn(c.N, generator=g) if c.bias else None
    C0 = torch.randn(c.M, c.N, generator=g)
    out, plan = gemm_launch(c, A, B, bias, C0)
    want, mag = R.gemm_reference(c, A.to(F64), B.to(F64), None if bias is None else bias.to(F64), C0.to(F64))
    bound = SECOND * gamma(c.K + plan["ksplit"] + 2) * mag + TINY
    check_bound(out.view.cpu(), want, bound, f"gemm_f32 {plan['kernel']}{' split' if plan['ksplit'] > 1 else ''}", name)


# ================================================================================================ LayerNorm
def ln_nsum(d):
    return (d + 255) // 256 + 10


def ln_fwd_bounds(x, w, b, eps):
    """fp64 device tensors -> (y, mean, rstd, Ey, Em, Er) as derived in the file header"""
    M, d = x.shape
    ns = ln_nsum(d)
    y, mean, rstd = R.layernorm_fwd_ref(x, w, b, eps)
    Em = SECOND * (gamma(ns) * x.abs().sum(1) / d + REL_MATH * mean.abs()) + TINY
    c = (x - mean[:, None]).abs()
    D = Em[:, None] + E * (c + Em[:, None])
    var = (c ** 2).mean(1)
    Ev = SECOND * ((gamma(ns + 1) * ((c + D) ** 2).sum(1) + (2 * c * D + D * D).sum(1)) / d + REL_MATH * var) + TINY
    wv = var + eps
    Ew = Ev + E * (wv + Ev)
    assert bool((Ew < wv).all()), "degenerate data: the variance is not resolved against eps (no finite bound on rstd)"
    Er = SECOND * (0.5 * Ew * (wv - Ew) ** -1.5 + REL_MATH * rstd) + TINY
    r, er = rstd[:, None], Er[:, None]
    E1 = D * (r + er) + c * er + E * (c + D) * (r + er)
    Ey = SECOND * (w.abs()[None] * E1 + 2 * E * (c * r * w.abs()[None] + w.abs()[None] * E1) + E * b.abs()[None]) + TINY
    return y, mean, rstd, Ey, Em, Er


LN_FWD = [(1, 1, 1e-5), (1, 1, 1e-12), (77, 7, 1e-12), (1, 255, 1e-5), (129, 256, 1e-12), (77, 257, 1e-5), (2, 768, 1e-12), (288, 1024, 1e-5),
          (129, 1, 1e-5), (288, 255, 1e-12), (1, 1024, 1e-12)]


@pytest.mark.parametrize("M,d,eps", LN_FWD)
def test_layernorm_forward(M, d, eps):
    what = f"layernorm_fwd M={M} d={d} eps={eps}"
    g = gen(M, d, 1)
    # d = 1: the variance is 0 and rstd = eps^-1/2 exactly as long as mean_k = x; small |x| keeps D^2 below eps = 1e-12
    x = randn(g, M, d, scale=0.25 if d == 1 else 1.0, dtype=F32) + (0.0 if d == 1 else 0.5)
    w, b = randn(g, d, dtype=F32) + 1.0, randn(g, d, dtype=F32)
    eps32 = float(np.float32(eps))
    y, mean, rstd = Guarded(M, d, dtype=F32), g1(M), g1(M)
    ro = ReadOnly(x=x, w=w, b=b)
    run(L().nv_layernorm_fwd_f32(ptr(x), ptr(w), ptr(b), ptr(y.view), ptr(mean.view), ptr(rstd.view), M, d, eps32, st()), what)
    for o in (y, mean, rstd):
        o.check(what, (slice(None), slice(None)))
    ro.check(what)
    x64, w64, b64 = x.to(F64), w.to(F64), b.to(F64)
    yr, mr, rr, Ey, Em, Er = ln_fwd_bounds(x64, w64, b64, eps32)
    check_bound(mean.view[0], mr, Em, "layernorm_fwd mean", what)
    check_bound(rstd.view[0], rr, Er, "layernorm_fwd rstd", what)
    check_bound(y.view, yr, Ey, "layernorm_fwd y", what)
    mk, rk = mean.view[0].to(F64)[:, None], rstd.view[0].to(F64)[:, None]
    prod = (x64 - mk) * rk * w64[None]
    check_bound(y.view, prod + b64[None], SECOND * (gamma(4) * prod.abs() + E * b64.abs()[None]) + TINY, "layernorm_fwd y from own mean/rstd", what)
    # null mean / rstd outputs: y alone, bit-identical
    y2 = Guarded(M, d, dtype=F32)
    run(L().nv_layernorm_fwd_f32(ptr(x), ptr(w), ptr(b), ptr(y2.view), None, None, M, d, eps32, st()), what + " null stats")
    y2.check(what, (slice(None), slice(None)))
    assert_bits(y2.view, y.view, what + " null stats")


def ln_bwd_run(dy, x, w, mean, rstd, gw0, gb0, acc, what):
    M, d = x.shape
    dx, gw, gb = Guarded(M, d, dtype=F32), g1(d, gw0), g1(d, gb0)
    nbytes = L().nv_layernorm_bwd_workspace_bytes(d)
    assert nbytes == 2 * 128 * d * 4
    ws = g1(nbytes // 4)
    ro = ReadOnly(dy=dy, x=x, w=w, mean=mean, rstd=rstd)
    run(L().nv_layernorm_bwd_f32(ptr(dy), ptr(x), ptr(w), ptr(mean), ptr(rstd), ptr(dx.view), ptr(gw.view), ptr(gb.view), ptr(ws.view), M, d, acc,
                                 st()), what)
    for o in (dx, gw, gb):
        o.check(what, (slice(None), slice(None)))
    written = torch.zeros(1, 2 * 128 * d, dtype=torch.bool, device=dev())                 # P = min(M, 128) partial rows of dg and of db
    P = min(M, 128)
    written[0, :P * d] = True
    written[0, 128 * d:128 * d + P * d] = True
    ws.check(what + " workspace", written)
    ro.check(what)
    return dx.view, gw.view[0], gb.view[0]


LN_BWD = [(1, 1, 0), (1, 257, 1), (127, 7, 0), (128, 255, 1), (129, 256, 0), (288, 257, 1), (288, 1024, 0), (129, 768, 1), (5, 1024, 1)]


@pytest.mark.parametrize("M,d,acc", LN_BWD)
def test_layernorm_backward(M, d, acc):
    what = f"layernorm_bwd M={M} d={d} acc={acc}"
    g = gen(M, d, acc, 2)
    x, dy, w = randn(g, M, d, dtype=F32) + 0.5, randn(g, M, d, dtype=F32), randn(g, d, dtype=F32) + 1.0
    x64 = x.to(F64)
    eps = 1e-5 if acc else 1e-12
    _, m64, r64 = R.layernorm_fwd_ref(x64, w.to(F64), torch.zeros(d, dtype=F64, device=dev()), eps)
    if d == 1:
        r64 = torch.full_like(r64, 3.0)                      # rstd is an input: any value will do, eps^-1/2 would only scale dx = 0
    mean, rstd = m64.to(F32), r64.to(F32)
    gw0, gb0 = randn(g, d, dtype=F32), randn(g, d, dtype=F32)
    dx, gw, gb = ln_bwd_run(dy, x, w, mean, rstd, gw0, gb0, acc, what)
    dy64, w64, mu, rs = dy.to(F64), w.to(F64), mean.to(F64), rstd.to(F64)
    dxr, gwr, gbr = R.layernorm_bwd_ref(dy64, x64, w64, mu, rs)
    g0w, g0b = (gw0.to(F64), gb0.to(F64)) if acc else (torch.zeros_like(gwr), torch.zeros_like(gbr))
    ns = ln_nsum(d)
    xh = ((x64 - mu[:, None]) * rs[:, None]).abs()
    dxh = (dy64 * w64[None])
    S1, S2 = dxh.mean(1, keepdim=True), (dxh * (x64 - mu[:, None]) * rs[:, None]).mean(1, keepdim=True)
    E1 = SECOND * (gamma(ns + 1) * dxh.abs().sum(1, keepdim=True) / d + REL_MATH * S1.abs()) + TINY
    E2 = SECOND * (gamma(ns + 4) * (dxh.abs() * xh).sum(1, keepdim=True) / d + REL_MATH * S2.abs()) + TINY
    Edx = SECOND * rs.abs()[:, None] * (E1 + xh * E2 + gamma(6) * (dxh.abs() + S1.abs() + xh * S2.abs())) + TINY
    check_bound(dx, dxr, Edx, "layernorm_bwd dx", what)
    check_bound(gw, gwr + g0w, SECOND * gamma(M + 5) * ((dy64.abs() * xh).sum(0) + g0w.abs()) + TINY, "layernorm_bwd gw", what)
    check_bound(gb, gbr + g0b, SECOND * gamma(M + 2) * (dy64.abs().sum(0) + g0b.abs()) + TINY, "layernorm_bwd gb", what)


@pytest.mark.parametrize("M,d,acc", [(288, 257, 1), (129, 64, 0), (128, 300, 1), (1, 5, 0)])
def test_layernorm_backward_exact_parameter_gradients(M, d, acc):
    """integer dy, x - mean in {-1, 0, 1}, rstd = 1: dy xh and every partial sum are integers below 2^24"""
    what = f"layernorm_bwd exact M={M} d={d} acc={acc}"
    g = R.cpu_gen(M, d, acc)
    xi, dyi = R.rand_ints(g, -1, 1, M, d), R.rand_ints(g, -8, 8, M, d)
    mu = R.rand_ints(g, -3, 3, M)
    g0w, g0b = R.rand_ints(g, -1000, 1000, d), R.rand_ints(g, -1000, 1000, d)
    todev = lambda t: t.to(F32).to(dev())
    _, gw, gb = ln_bwd_run(todev(dyi), todev(xi + mu[:, None]), randn(gen(M, d), d, dtype=F32), todev(mu), torch.ones(M, dtype=F32, device=dev()),
                           todev(g0w), todev(g0b), acc, what)
    assert_bits(gw, ((dyi * xi).sum(0) + (g0w if acc else 0)).to(F32), what + " gw")
    assert_bits(gb, (dyi.sum(0) + (g0b if acc else 0)).to(F32), what + " gb")


# ================================================================================================ colsum
COLSUM = ([(P, 65, 3, P % 2) for P in (0, 1, 3, 4, 5, 28, 29, 32, 33, 36, 64, 65, 288)] +
          [(0, 1, 0, 1), (1, 1, 0, 0), (5, 1, 2, 1), (29, 63, 0, 0), (33, 64, 0, 1), (36, 64, 5, 0), (65, 300, 0, 1), (288, 300, 4, 0), (61, 63, 1, 1),
           (60, 300, 2, 1), (93, 65, 0, 0)])


@pytest.mark.parametrize("P,d,pad,acc", COLSUM)
def test_colsum_exact(P, d, pad, acc):
    what = f"colsum P={P} d={d} ld={d + pad} acc={acc}"
    g = R.cpu_gen(P, d, pad, acc)
    xi, o0 = R.rand_ints(g, -1000, 1000, P, d), R.rand_ints(g, -1000, 1000, d)
    xbuf, _, x_addr = padded(xi, d + pad)
    out = g1(d, o0.to(F32))
    ro = ReadOnly(x=xbuf)
    run(L().nv_colsum_f32(x_addr, ptr(out.view), P, d, d + pad, acc, st()), what)
    out.check(what, (slice(None), slice(None)))
    ro.check(what)
    assert_bits(out.view[0], (xi.sum(0) + (o0 if acc else 0)).to(F32), what)


# ================================================================================================ attention core
MHA_SHAPES = [(2, 8, 4, 32), (3, 36, 2, 64), (2, 70, 2, 16), (1, 130, 1, 8)]


def mha_lens(B, N, pow2=False):
    """N, a value in the middle, 1 (powers of two for the exact cases)"""
    if pow2:
        top = 1 << (N.bit_length() - 1)
        return torch.tensor([top, max(1, top // 4), 1][:B], dtype=I32, device=dev())
    return torch.tensor([N, max(1, (N * 5) // 9), 1][:B], dtype=I32, device=dev())


def mha_forward(qkv, lens, B, N, heads, hd, keep=None, p=0.0, seed=0, offset=0, what="", plain=False):
    h = heads * hd
    out, P = Guarded(B * N, h, dtype=F32), Guarded(B * heads * N, N, dtype=F32)
    ro = ReadOnly(**{k: t for k, t in dict(qkv=qkv, lens=lens, keep=keep).items() if t is not None})
    if plain:
        rc = L().nv_mha_fwd_f32(ptr(qkv), ptr(lens), ptr(out.view), ptr(P.view), B, N, heads, hd, st())
    else:
        rc = L().nv_mha_fwd_drop_f32(ptr(qkv), ptr(lens), ptr(out.view), ptr(P.view), ptr(keep), p, seed, offset, B, N, heads, hd, st())
    run(rc, what)
    out.check(what, (slice(None), slice(None)))
    P.check(what, (slice(None), slice(None)))
    ro.check(what)
    return out.view, P.view.reshape(B, heads, N, N)


def mha_backward(qkv, P, dout, B, N, heads, hd, keep=None, p=0.0, seed=0, offset=0, what="", plain=False):
    dqkv = Guarded(B * N, 3 * heads * hd, dtype=F32)
    ro = ReadOnly(**{k: t for k, t in dict(qkv=qkv, P=P, dout=dout, keep=keep).items() if t is not None})
    if plain:
        rc = L().nv_mha_bwd_f32(ptr(qkv), ptr(P), ptr(dout), ptr(dqkv.view), B, N, heads, hd, st())
    else:
        rc = L().nv_mha_bwd_drop_f32(ptr(qkv), ptr(P), ptr(dout), ptr(dqkv.view), ptr(keep), p, seed, offset, B, N, heads, hd, st())
    run(rc, what)
    dqkv.check(what, (slice(None), slice(None)))
    ro.check(what)
    return dqkv.view


def heads_first(t, B, N, heads, hd):
    """[B*N, h] -> [B, heads, N, hd]"""
    return t.reshape(B, N, heads, hd).permute(0, 2, 1, 3)


def mha_fwd_bounds(qkv64, lens, B, N, heads, hd, keep64, p):
    out, P = R.mha_fwd_ref(qkv64, lens, B, N, heads, hd, keep64, p)
    q, k, v = R.split_qkv(qkv64, B, N, heads, hd)
    rs = 1.0 / math.sqrt(hd)
    s = (q @ k.transpose(-1, -2)) * rs
    Es = SECOND * (gamma(hd + 1) + REL_MATH + E) * (q.abs() @ k.abs().transpose(-1, -2)) * rs
    valid = (torch.arange(N, device=dev())[None, :] < lens[:, None])[:, None, None, :].expand(B, heads, N, N)
    smax = s.masked_fill(~valid, -float("inf")).max(-1, keepdim=True).values
    Esm = Es.masked_fill(~valid, 0.0).max(-1, keepdim=True).values
    delta = Es + Esm + E * ((smax - s).clamp(min=0) + 4 * Esm)
    rho = (SECOND * (torch.expm1(delta) + REL_MATH)).masked_fill(~valid, 0.0)
    nw = (N + 63) // 64 + 6
    EP = SECOND * (rho + rho.max(-1, keepdim=True).values + gamma(nw + 1) + REL_MATH) * P + TINY
    m = torch.ones_like(P) if p == 0.0 else keep64 / (1.0 - p)
    relm = (REL_MATH + 2 * E) if p > 0 else 0.0
    Eout = SECOND * ((m * (EP + P * (gamma(N) + relm))) @ v.abs()) + TINY
    return out, P, Eout.permute(0, 2, 1, 3).reshape(B * N, heads * hd), EP


def mha_bwd_bounds(qkv64, P, dout64, B, N, heads, hd, keep64, p):
    want = R.mha_bwd_ref(qkv64, P, dout64, B, N, heads, hd, keep64, p)
    q, k, v = R.split_qkv(qkv64, B, N, heads, hd)
    dO = heads_first(dout64, B, N, heads, hd)
    rs = 1.0 / math.sqrt(hd)
    m = torch.ones_like(P) if p == 0.0 else keep64 / (1.0 - p)
    relm = (REL_MATH + 2 * E) if p > 0 else 0.0
    nw = (N + 63) // 64 + 6
    dp = (dO @ v.transpose(-1, -2)) * m
    Edp = SECOND * (gamma(hd + 2) + relm) * (dO.abs() @ v.abs().transpose(-1, -2)) * m
    dot = (dp * P).sum(-1, keepdim=True)
    Edot = SECOND * ((Edp * P).sum(-1, keepdim=True) + gamma(nw + 1) * (dp.abs() * P).sum(-1, keepdim=True))
    dS = P * (dp - dot)
    EdS = SECOND * P * (Edp + Edot + gamma(2) * (dp.abs() + dot.abs()))
    Edq = SECOND * rs * (EdS @ k.abs() + (gamma(N + 1) + REL_MATH) * (dS.abs() @ k.abs())) + TINY
    Edk = SECOND * rs * (EdS.transpose(-1, -2) @ q.abs() + (gamma(N + 1) + REL_MATH) * (dS.abs().transpose(-1, -2) @ q.abs())) + TINY
    Edv = SECOND * (gamma(N) + relm + E) * ((P * m).transpose(-1, -2) @ dO.abs()) + TINY
    bound = torch.stack([Edq, Edk, Edv], dim=0).permute(1, 3, 0, 2, 4).reshape(B * N, 3 * heads * hd)
    return want, bound


def onehot_qkv(B, N, heads, hd, window):
    """q = 0, k arbitrary, v[key j of head hh, column j mod hd] = 1 + (j + 3 hh) mod 7 for the keys of `window` (hd keys), else 0"""
    h = heads * hd
    g = R.cpu_gen(B, N, heads, hd)
    qkv = torch.zeros(B, N, 3, heads, hd)
    qkv[:, :, 1] = torch.randn(B, N, heads, hd, generator=g)
    val = torch.zeros(heads, N)
    for j in range(window * hd, min(N, (window + 1) * hd)):
        for hh in range(heads):
            val[hh, j] = 1 + (j + 3 * hh) % 7
            qkv[:, j, 2, hh, j % hd] = val[hh, j]
    return qkv.reshape(B * N, 3 * h).to(dev()), val.to(dev())


@pytest.mark.parametrize("B,N,heads,hd", MHA_SHAPES)
def test_mha_forward_exact_structure(B, N, heads, hd):
    what = f"mha_fwd exact B={B} N={N} heads={heads} hd={hd}"
    lens = mha_lens(B, N, pow2=True)
    valid = torch.arange(N, device=dev())[None, :] < lens[:, None]                          # [B, N]
    P_want = (valid.to(F32) / lens.to(F32)[:, None])[:, None, None, :].expand(B, heads, N, N)
    for window in range((N + hd - 1) // hd):
        qkv, val = onehot_qkv(B, N, heads, hd, window)
        out, P = mha_forward(qkv, lens, B, N, heads, hd, what=f"{what} window {window}", plain=True)
        assert_bits(P, P_want, f"{what} window {window} P")
        want = torch.zeros(B, heads, N, hd, device=dev())
        for j in range(window * hd, min(N, (window + 1) * hd)):
            want[:, :, :, j % hd] = (val[None, :, j] * P_want[:, :, 0, j])[:, :, None]
        assert_bits(out, want.permute(0, 2, 1, 3).reshape(B * N, heads * hd), f"{what} window {window} out")


def mha_random(B, N, heads, hd, key):
    g = gen(B, N, heads, hd, key)
    h = heads * hd
    return randn(g, B * N, 3 * h, scale=0.5, dtype=F32), randn(g, B * N, h, scale=0.5, dtype=F32)


@pytest.mark.parametrize("B,N,heads,hd", MHA_SHAPES)
def test_mha_forward_backward_bounded(B, N, heads, hd):
    what = f"mha B={B} N={N} heads={heads} hd={hd}"
    qkv, dout = mha_random(B, N, heads, hd, 1)
    lens = mha_lens(B, N)
    out, P = mha_forward(qkv, lens, B, N, heads, hd, what=what + " fwd", plain=True)
    qkv64 = qkv.to(F64)
    o_ref, P_ref, Eout, EP = mha_fwd_bounds(qkv64, lens, B, N, heads, hd, None, 0.0)
    check_bound(P, P_ref, EP, "mha_fwd P", what)
    check_bound(out, o_ref, Eout, "mha_fwd out", what)
    pad = torch.arange(N, device=dev())[None, :] >= lens[:, None]
    assert bool((P.view(torch.int32)[pad[:, None, None, :].expand(B, heads, N, N)] == 0).all()), f"{what}: P of a padded key is not +0"
    # backward for a given P: the reference probabilities, rounded to fp32
    Pin = P_ref.to(F32).contiguous()
    dqkv = mha_backward(qkv, Pin, dout, B, N, heads, hd, what=what + " bwd", plain=True)
    want, bound = mha_bwd_bounds(qkv64, Pin.to(F64), dout.to(F64), B, N, heads, hd, None, 0.0)
    check_bound(dqkv, want, bound, "mha_bwd dqkv", what)
    kv = dqkv.reshape(B, N, 3, heads * hd)[:, :, 1:]
    assert bool((kv[pad] == 0).all()), f"{what}: a k / v gradient row of a padded key is not +-0"


DROP = [(2, 8, 4, 32, 0.1, 7), (2, 8, 4, 32, 0.5, (1 << 32) - 300), (2, 70, 2, 16, 0.5, 12345), (2, 70, 2, 16, 0.1, (1 << 32) - 9000),
        (1, 130, 1, 8, 0.5, (1 << 33) - 5000)]


@pytest.mark.parametrize("B,N,heads,hd,p,offset", DROP)
def test_mha_dropout_kept_set_is_philox(B, N, heads, hd, p, offset):
    what = f"mha_fwd drop B={B} N={N} heads={heads} hd={hd} p={p} offset={offset}"
    seed = 0x1234567 * 0x89ABCDEF + N
    total = B * heads * N * N
    assert offset == 7 or offset == 12345 or (offset >> 32) != ((offset + total - 1) >> 32), "the counter must cross a multiple of 2^32"
    lens = mha_lens(B, N, pow2=True)
    keep = torch.from_numpy(R.mha_keep(seed, offset, B, heads, N, p)).to(dev())
    valid = (torch.arange(N, device=dev())[None, :] < lens[:, None])[:, None, None, :].expand(B, heads, N, N)
    got = torch.zeros(B, heads, N, N, dtype=torch.bool, device=dev())
    for window in range((N + hd - 1) // hd):
        qkv, _ = onehot_qkv(B, N, heads, hd, window)
        out, _ = mha_forward(qkv, lens, B, N, heads, hd, p=p, seed=seed, offset=offset, what=f"{what} window {window}")
        o = heads_first(out, B, N, heads, hd)
        for j in range(window * hd, min(N, (window + 1) * hd)):
            got[:, :, :, j] = o[:, :, :, j % hd] != 0
    diff = (got != keep) & valid
    assert not bool(diff.any()), f"{what}: {int(diff.sum())} of {int(valid.sum())} keep flags differ from Philox; first at {diff.nonzero()[0].tolist()}"
    assert not bool((got & ~valid).any()), f"{what}: a padded key contributes"
    rate = keep[valid].float().mean().item()
    assert abs(rate - (1 - p)) < 0.05, rate


@pytest.mark.parametrize("B,N,heads,hd,p,offset", [(2, 8, 4, 32, 0.1, (1 << 32) - 300), (3, 36, 2, 64, 0.5, 99), (2, 70, 2, 16, 0.1, (1 << 32) - 9000),
                                                   (1, 130, 1, 8, 0.5, 3)])
def test_mha_dropout_injected_mask_identical_and_bounded(B, N, heads, hd, p, offset):
    what = f"mha drop B={B} N={N} heads={heads} hd={hd} p={p} offset={offset}"
    seed = 0xDEADBEEFCAFE + hd
    p32 = float(np.float32(p))
    qkv, dout = mha_random(B, N, heads, hd, 2)
    lens = mha_lens(B, N)
    keep = torch.from_numpy(R.mha_keep(seed, offset, B, heads, N, p)).to(dev()).to(F32).contiguous()
    out_p, P_p = mha_forward(qkv, lens, B, N, heads, hd, p=p32, seed=seed, offset=offset, what=what + " philox fwd")
    out_k, P_k = mha_forward(qkv, lens, B, N, heads, hd, keep=keep, p=p32, seed=seed + 1, offset=offset + 1, what=what + " injected fwd")
    assert_bits(out_k, out_p, what + ": forward with the host mask injected vs the in-kernel Philox draw")
    assert_bits(P_k, P_p, what + " P")
    qkv64, keep64 = qkv.to(F64), keep.to(F64)
    o_ref, P_ref, Eout, EP = mha_fwd_bounds(qkv64, lens, B, N, heads, hd, keep64, p32)
    check_bound(P_k, P_ref, EP, "mha_fwd P", what)
    check_bound(out_k, o_ref, Eout, "mha_fwd_drop out", what)
    Pin = P_ref.to(F32).contiguous()
    d_p = mha_backward(qkv, Pin, dout, B, N, heads, hd, p=p32, seed=seed, offset=offset, what=what + " philox bwd")
    d_k = mha_backward(qkv, Pin, dout, B, N, heads, hd, keep=keep, p=p32, seed=seed + 1, offset=offset + 1, what=what + " injected bwd")
    assert_bits(d_k, d_p, what + ": backward with the host mask injected vs the in-kernel Philox draw")
    want, bound = mha_bwd_bounds(qkv64, Pin.to(F64), dout.to(F64), B, N, heads, hd, keep64, p32)
    check_bound(d_k, want, bound, "mha_bwd_drop dqkv", what)


def test_mha_refusals_leave_the_outputs_untouched():
    B, N, heads, hd = 1, 8, 2, 8
    qkv, dout = mha_random(B, N, heads, hd, 3)
    lens = mha_lens(B, N)
    h = heads * hd
    out, P, dq = Guarded(B * N, h, dtype=F32), Guarded(B * heads * N, N, dtype=F32), Guarded(B * N, 3 * h, dtype=F32)
    Pin = torch.full((B * heads * N, N), 1.0 / N, dtype=F32, device=dev())
    o, pp, q, l_, d_ = ptr(out.view), ptr(P.view), ptr(qkv), ptr(lens), ptr(dout)
    for p in (-0.1, 1.0, 1.5, NAN):
        run(L().nv_mha_fwd_drop_f32(q, l_, o, pp, None, p, 1, 2, B, N, heads, hd, st()), f"mha_fwd p={p}", NV_ERR_ARG)
        run(L().nv_mha_bwd_drop_f32(q, ptr(Pin), d_, ptr(dq.view), None, p, 1, 2, B, N, heads, hd, st()), f"mha_bwd p={p}", NV_ERR_ARG)
    for args in ((None, l_, o, pp), (q, None, o, pp), (q, l_, None, pp), (q, l_, o, None)):
        run(L().nv_mha_fwd_drop_f32(*args, None, 0.1, 1, 2, B, N, heads, hd, st()), "mha_fwd null", NV_ERR_ARG)
        run(L().nv_mha_fwd_f32(*args, B, N, heads, hd, st()), "mha_fwd null", NV_ERR_ARG)
    for args in ((None, ptr(Pin), d_, ptr(dq.view)), (q, None, d_, ptr(dq.view)), (q, ptr(Pin), None, ptr(dq.view)), (q, ptr(Pin), d_, None)):
        run(L().nv_mha_bwd_drop_f32(*args, None, 0.1, 1, 2, B, N, heads, hd, st()), "mha_bwd null", NV_ERR_ARG)
        run(L().nv_mha_bwd_f32(*args, B, N, heads, hd, st()), "mha_bwd null", NV_ERR_ARG)
    for o_ in (out, P, dq):
        o_.check("mha refusals", (slice(0, 0), slice(0, 0)))
    # LDS: forward (3 N (hd + 1) + N^2) 4 bytes, backward (4 N (hd + 1) + 2 N^2) 4 bytes, limit 160 KiB
    for N2, hd2, fwd_ok in ((200, 8, False), (150, 8, True)):
        assert ((3 * N2 * (hd2 + 1) + N2 * N2) * 4 <= 160 * 1024) == fwd_ok and (4 * N2 * (hd2 + 1) + 2 * N2 * N2) * 4 > 160 * 1024
        qkv2, dout2 = mha_random(1, N2, 1, hd2, 4)
        lens2 = mha_lens(1, N2)
        out2, P2, dq2 = Guarded(N2, hd2, dtype=F32), Guarded(N2, N2, dtype=F32), Guarded(N2, 3 * hd2, dtype=F32)
        Pin2 = torch.full((N2, N2), 1.0 / N2, dtype=F32, device=dev())
        if not fwd_ok:
            run(L().nv_mha_fwd_f32(ptr(qkv2), ptr(lens2), ptr(out2.view), ptr(P2.view), 1, N2, 1, hd2, st()), f"mha_fwd N={N2}", NV_ERR_SHAPE)
        run(L().nv_mha_bwd_f32(ptr(qkv2), ptr(Pin2), ptr(dout2), ptr(dq2.view), 1, N2, 1, hd2, st()), f"mha_bwd N={N2}", NV_ERR_SHAPE)
        for o_ in (out2, P2, dq2):
            o_.check(f"mha LDS refusal N={N2}", (slice(0, 0), slice(0, 0)))


# ================================================================================================ dropout
# 4 * 524288 + 5 elements: 524290 groups, above the 524288 of the capped grid; p = 0.5 (an exact 1 / (1 - p)) at one size
DROPOUT = ([(n, p, o) for n in (1, 3, 4, 1001, 4 * 524288 + 5) for p in (0.0, 0.1, 0.4) for o in (0, 12345, (1 << 32) - 2)] +
           [(1001, 0.5, o) for o in (0, 12345, (1 << 32) - 2)])


@pytest.mark.parametrize("n,p,offset", DROPOUT)
def test_dropout_mask_is_philox(n, p, offset):
    what = f"dropout n={n} p={p} offset={offset}"
    seed = 0xA5A5A5A55A5A5A5A ^ n
    x = 1.0 + randn(gen(n, 3), n, dtype=F32).abs()                       # non-zero: the kept set can be read off the output
    out = g1(n)
    ro = ReadOnly(x=x)
    p32 = np.float32(p)
    run(L().nv_dropout_f32(ptr(x), ptr(out.view), n, float(p32), seed, offset, st()), what)
    out.check(what, (slice(None), slice(None)))
    ro.check(what)
    keep = torch.from_numpy(R.dropout_keep(seed, offset, n, p)).to(dev())
    got = out.view[0]
    diff = (got != 0) != keep
    assert not bool(diff.any()), f"{what}: {int(diff.sum())} keep flags differ from Philox; first at element {int(diff.nonzero()[0])}"
    assert bool((got.view(torch.int32)[~keep] == 0).all()), f"{what}: a dropped element is not +0"
    if p == 0.0:
        assert bool(keep.all())
    scale64 = 1.0 / (1.0 - float(p32))
    if p in (0.0, 0.5):
        assert_bits(got[keep], (x.to(F64) * scale64).to(F32)[keep], what + " kept values")
    else:
        want = x.to(F64) * scale64
        check_bound(got[keep], want[keep], (SECOND * (REL_MATH + 2 * E) * want.abs() + TINY)[keep], "dropout kept values", what)


def test_dropout_refusals():
    x, out = torch.ones(8, dtype=F32, device=dev()), g1(8)
    for p in (-0.5, 1.0, NAN):
        run(L().nv_dropout_f32(ptr(x), ptr(out.view), 8, p, 1, 2, st()), f"dropout p={p}", NV_ERR_ARG)
    run(L().nv_dropout_f32(None, ptr(out.view), 8, 0.1, 1, 2, st()), "dropout null x", NV_ERR_ARG)
    run(L().nv_dropout_f32(ptr(x), None, 8, 0.1, 1, 2, st()), "dropout null out", NV_ERR_ARG)
    run(L().nv_dropout_f32(ptr(x), ptr(out.view), 0, 0.1, 1, 2, st()), "dropout n=0")
    out.check("dropout refusals", (slice(0, 0), slice(0, 0)))


# ================================================================================================ GELU
def gelu_grid(n):
    """+-0, subnormals, +-2^k up to 32, dense points in [-6, 6]; filled up to n with uniform points of [-6, 6]"""
    pow2 = 2.0 ** torch.arange(-30, 6, dtype=F64)
    special = torch.tensor([0.0, -0.0, 1e-40, -1e-40, 2.0 ** -149, -2.0 ** -149, 2.0 ** -127, -2.0 ** -127, 2.0 ** -126], dtype=F64)
    v = torch.cat([special, pow2, -pow2, torch.linspace(-6, 6, 4801, dtype=F64)])
    if n > v.numel():
        v = torch.cat([v, torch.rand(n - v.numel(), generator=R.cpu_gen(n), dtype=F64) * 12 - 6])
    v = v.to(F32)
    assert torch.isfinite(v).all() and v.abs().max() == 32 and v.numel() == max(n, v.numel())
    return v.to(dev())


def gelu_err_erf(v64):
    u = v64.abs() / math.sqrt(2.0)
    erf = torch.erf(v64 / math.sqrt(2.0))
    return (2.0 / math.sqrt(math.pi)) * torch.exp(-u * u) * gamma(2) * u + REL_MATH * erf.abs(), erf


@pytest.mark.parametrize("n", [0, CAP + 259], ids=["grid", "above-cap"])
def test_gelu_forward_backward(n):
    v = gelu_grid(n)
    n = v.numel()
    what = f"gelu n={n}"
    dy = randn(gen(n, 5), n, dtype=F32)
    y, dx = g1(n), g1(n)
    ro = ReadOnly(v=v, dy=dy)
    run(L().nv_gelu_fwd_f32(ptr(v), ptr(y.view), n, st()), what + " fwd")
    run(L().nv_gelu_bwd_f32(ptr(v), ptr(dy), ptr(dx.view), n, st()), what + " bwd")
    y.check(what, (slice(None), slice(None)))
    dx.check(what, (slice(None), slice(None)))
    ro.check(what)
    v64, dy64 = v.to(F64), dy.to(F64)
    Eerf, erf = gelu_err_erf(v64)
    yr = R.gelu_fwd_ref(v64)
    check_bound(y.view[0], yr, SECOND * (0.5 * v64.abs() * (Eerf + E * (1 + erf)) + E * yr.abs()) + TINY, "gelu_fwd", what)
    dxr, cdf, pdf = R.gelu_bwd_ref(v64, dy64)
    Ecdf = 0.5 * (Eerf + E * (1 + erf))
    Epdf = SECOND * pdf * (torch.expm1(E * v64 * v64 / 2) + REL_MATH + 2 * E) + TINY
    Edx = (SECOND * (dy64.abs() * (Ecdf + v64.abs() * Epdf + E * v64.abs() * pdf + E * (cdf + v64.abs() * pdf)) + E * dxr.abs()) +
           TINY * (1 + dy64.abs() * (1 + v64.abs())))
    check_bound(dx.view[0], dxr, Edx, "gelu_bwd", what)


# ================================================================================================ single-rounding ops
@pytest.mark.parametrize("rows,d", [(3, 7), (2053, 257)])
def test_add_mul_rowscale_exact(rows, d):
    """one correctly rounded operation each: the float64 result (exact for a product, and for a sum of values of comparable size)
    rounded once.  2053 x 257 = 527,621 elements: above the 524,288 of the capped grid"""
    n = rows * d
    assert (n > CAP) == (rows > 3)
    g = gen(rows, d, 6)
    a, b, brow, s = randn(g, n, dtype=F32), randn(g, n, dtype=F32), randn(g, d, dtype=F32), randn(g, rows, dtype=F32)
    ro = ReadOnly(a=a, b=b, brow=brow, s=s)
    a64 = a.to(F64)
    for what, call, want in (
            ("add", lambda o: L().nv_add_f32(ptr(a), ptr(b), o, n, d, 0, st()), a64 + b.to(F64)),
            ("add row-broadcast", lambda o: L().nv_add_f32(ptr(a), ptr(brow), o, n, d, 1, st()), (a64.reshape(rows, d) + brow.to(F64)[None]).reshape(n)),
            ("mul", lambda o: L().nv_mul_f32(ptr(a), ptr(b), o, n, st()), a64 * b.to(F64)),
            ("rowscale", lambda o: L().nv_rowscale_f32(ptr(a), ptr(s), o, rows, d, st()), (a64.reshape(rows, d) * s.to(F64)[:, None]).reshape(n))):
        out = g1(n)
        run(call(ptr(out.view)), f"{what} rows={rows} d={d}")
        out.check(what, (slice(None), slice(None)))
        assert_bits(out.view[0], want.to(F32), f"{what} rows={rows} d={d}")
    ro.check("add / mul / rowscale")


@pytest.mark.parametrize("rows,d,S,with_base", [(9, 5, 4, True), (9, 5, 4, False), (2053, 257, 37, True), (700, 600, 3, False)])
def test_gather_add_exact(rows, d, S, with_base):
    what = f"gather_add rows={rows} d={d} S={S} base={with_base}"
    g = gen(rows, d, S, 7)
    src = randn(g, S, d, dtype=F32)
    base = randn(g, rows, d, dtype=F32) if with_base else None
    idx = (torch.arange(rows, device=dev()) * 7 % (S + 2) - 2).clamp(min=-1).to(I32)            # -1 (several times) and repeated indices
    assert int((idx < 0).sum()) >= 2 and int(idx.max()) == S - 1 and idx.unique().numel() < rows
    out = Guarded(rows, d, dtype=F32)
    ro = ReadOnly(**{k: t for k, t in dict(src=src, base=base, idx=idx).items() if t is not None})
    run(L().nv_gather_add_f32(ptr(src), ptr(idx), ptr(base), ptr(out.view), rows, d, st()), what)
    out.check(what, (slice(None), slice(None)))
    ro.check(what)
    want = torch.where((idx >= 0)[:, None], src.to(F64)[idx.clamp(min=0).long()], torch.zeros(rows, d, dtype=F64, device=dev()))
    if with_base:
        want = want + base.to(F64)
    assert_bits(out.view, want.to(F32), what)


@pytest.mark.parametrize("n,Rr,d,acc", [(11, 4, 5, 0), (40, 6, 255, 1), (40, 3, 256, 0), (23, 5, 257, 1), (300, 7, 600, 0), (0, 2, 9, 1)])
def test_index_sum_exact(n, Rr, d, acc):
    what = f"index_sum n={n} R={Rr} d={d} acc={acc}"
    g = R.cpu_gen(n, Rr, d, acc)
    srci, d0 = R.rand_ints(g, -1000, 1000, n, d), R.rand_ints(g, -1000, 1000, Rr, d)
    idx = R.rand_ints(g, 0, Rr - 2, n)                            # the value R - 1 never occurs: a zero row
    idx[idx == 1] = -1                                            # nor does 1; -1 matches no row
    src = torch.cat([srci, torch.zeros(1, d, dtype=torch.int64)]).to(F32).to(dev())[:n + 1]          # never empty: n = 0 needs a pointer
    idxd = torch.cat([idx, torch.zeros(1, dtype=torch.int64)]).to(I32).to(dev())
    out = Guarded(Rr, d, dtype=F32, init=d0.to(F32))
    ro = ReadOnly(src=src, idx=idxd)
    run(L().nv_index_sum_f32(ptr(src), ptr(idxd), ptr(out.view), n, Rr, d, acc, st()), what)
    out.check(what, (slice(None), slice(None)))
    ro.check(what)
    want = torch.zeros(Rr, d, dtype=torch.int64)
    for r in range(Rr):
        want[r] = srci[idx == r].sum(0)
    assert int(want[Rr - 1].abs().sum()) == 0 and int(want[1].abs().sum()) == 0
    assert_bits(out.view, (want + (d0 if acc else 0)).to(F32), what)


@pytest.mark.parametrize("B,N,d", [(3, 8, 5), (4, 17, 255), (3, 16, 256), (5, 9, 257), (3, 33, 600)])
def test_masked_mean(B, N, d):
    """integer x: the numerator is exact; rows with a power-of-two count (a single kept row included) have an exact quotient"""
    what = f"masked_mean B={B} N={N} d={d}"
    g = R.cpu_gen(B, N, d)
    xi = R.rand_ints(g, -1000, 1000, B, N, d)
    mask = torch.zeros(B, N, dtype=torch.int64)
    counts = [1, 4, 3, N, 8][:B]                                  # one kept row; powers of two; 3 and (for odd N) N are not
    for b, cnt in enumerate(counts):
        mask[b, torch.randperm(N, generator=g)[:cnt]] = 1
    assert len({tuple(r.tolist()) for r in mask}) == B            # every batch row has its own mask
    x, m = xi.to(F32).to(dev()), mask.to(F32).to(dev())
    out = Guarded(B, d, dtype=F32)
    ro = ReadOnly(x=x, mask=m)
    run(L().nv_masked_mean_f32(ptr(x), ptr(m), ptr(out.view), B, N, d, st()), what)
    out.check(what, (slice(None), slice(None)))
    ro.check(what)
    num = (xi * mask[:, :, None]).sum(1)
    want = num.to(F64) / torch.tensor(counts, dtype=F64)[:, None]
    for b, cnt in enumerate(counts):
        if cnt & (cnt - 1) == 0:
            assert_bits(out.view[b], want[b].to(F32), f"{what} row {b} (count {cnt})")
    check_bound(out.view.cpu(), want, SECOND * REL_MATH * want.abs() + TINY, "masked_mean quotient", what)


def test_small_ops_refusals_and_empty_calls():
    x, out = torch.ones(16, dtype=F32, device=dev()), g1(16)
    idx = torch.zeros(4, dtype=I32, device=dev())
    o, xp, ip = ptr(out.view), ptr(x), ptr(idx)
    for what, rc in (("gelu_fwd", L().nv_gelu_fwd_f32(None, o, 4, st())), ("gelu_bwd", L().nv_gelu_bwd_f32(xp, None, o, 4, st())),
                     ("add", L().nv_add_f32(xp, None, o, 4, 4, 0, st())), ("mul", L().nv_mul_f32(None, xp, o, 4, st())),
                     ("rowscale", L().nv_rowscale_f32(xp, None, o, 2, 2, st())), ("gather_add", L().nv_gather_add_f32(xp, None, None, o, 2, 2, st())),
                     ("index_sum", L().nv_index_sum_f32(xp, None, o, 2, 2, 2, 0, st())), ("masked_mean", L().nv_masked_mean_f32(xp, None, o, 1, 2, 2, st())),
                     ("colsum", L().nv_colsum_f32(None, o, 2, 2, 2, 0, st())),
                     ("layernorm_fwd", L().nv_layernorm_fwd_f32(xp, xp, None, o, None, None, 2, 2, 1e-5, st())),
                     ("layernorm_bwd", L().nv_layernorm_bwd_f32(xp, xp, xp, xp, xp, o, o, o, None, 2, 2, 0, st()))):
        run(rc, what + " null argument", NV_ERR_ARG)
    for what, rc in (("gelu_fwd", L().nv_gelu_fwd_f32(xp, o, 0, st())), ("add", L().nv_add_f32(xp, xp, o, 0, 4, 0, st())),
                     ("rowscale", L().nv_rowscale_f32(xp, xp, o, 0, 2, st())), ("gather_add", L().nv_gather_add_f32(xp, ip, None, o, 0, 2, st())),
                     ("index_sum", L().nv_index_sum_f32(xp, ip, o, 2, 0, 2, 0, st())), ("masked_mean", L().nv_masked_mean_f32(xp, xp, o, 0, 2, 2, st())),
                     ("layernorm_fwd", L().nv_layernorm_fwd_f32(xp, xp, xp, o, None, None, 0, 2, 1e-5, st()))):
        run(rc, what + " empty")
    out.check("refusals and empty calls", (slice(0, 0), slice(0, 0)))
