"""GPU: every kernel of csrc/head_loss_optim.hip against an fp64 reference (heads, action CE, LM CE, sum of squares / clip
coefficient) or, for AdamW, against the oracle's `adamw_step_` at sizes where the grid strides.

Bounds are derived, never measured (x = the fp64 value; u, e, REL_MATH, TINY, SECOND, gamma as in refkit's docstring).

Heads (the RANDOM form of test_gemm_ref_gpu.py).  A sum of K products accumulated in fp32 in any order is within
Ek = (K + 1) e sum |a| |b| of its fp64 value.
    y  = bf16(acc + bias)            : the bias joins the sum as one more term (K = d + 1):  |y - x| <= Ek + u (|x| + Ek)
    dx = bf16(sum_n dy W)            : K = N
    gW = bf16(gW0 + bf16(sum_b dy x)): K = B;  Ei = Ek + u (|S| + Ek);  |gW - (gW0 + S)| <= Ei + (u + e) SECOND (|gW0| + |S| + Ei)
    gb likewise with the terms dy[b, n].

Cross entropy (action: one wave of 64 lanes per row; LM: 256 threads per row, special columns count as -inf).  mx = max l is exact.
s = sum exp(l_j - mx): the difference is one fp32 rounding, which moves the exponent by e |l_j - mx|; expf adds REL_MATH; a term
passes through at most D roundings of the sum (D = ceil(G / 64) + 6 for the wave, ceil(V / 256) + 10 for the block), all terms >= 0:
    ds := SECOND sum_j exp(l_j - mx) (REL_MATH + e |l_j - mx| + gamma(D)) / s          (relative error of s; s >= 1)
    lse = fl(mx + logf(s)) : dlse := SECOND (ds + REL_MATH |log s|) + e (|mx| + |log s|)
    loss = fl(lse - l_t)   : |loss - x| <= dlse + e (|mx| + |log s| + |l_t|)
    p_j = expf(fl(l_j - lse)) : dp := SECOND p_j (REL_MATH + dlse + e |l_j - lse|) + TINY   (a probability below 2^-126 may vanish)
    g = fl(gs * fl(p_j - [j = t])) : dg := |gs| (dp + e |p_j - [j = t]|) + e |g| ;  dlogits = bf16(g): |got - g| <= dg + u (|g| + dg) + TINY
gs is the fp32 value of gscale, times the fp32 value of gscale_dev rounded once to fp32 where that is given.  Ignored rows (a
negative target; for the action loss also t >= G, which the kernel treats as ignored) give loss 0 and an all-zero gradient row.

sum of squares / clip coefficient.  Every thread adds its terms in turn, a block reduces them (6 + 4 levels), the final kernel adds
ceil(P / 256) partials per thread and reduces again (6 + 4).  With T the largest number of terms one thread adds in the first kernel
(+1 for the rounding of an fp32 square; a bf16 square is exact) the sum of squares is within gamma(D), D = T + 1 + 10 + ceil(P / 256)
+ 10, of its fp64 value, and the norm within SECOND (gamma(D) / 2 + REL_MATH) ||g|| (sqrtf).  The coefficient is then one fp32 add
and one fp32 division of the kernel's own norm: asserted exactly.

AdamW at striding sizes: bit-compared with the oracle on the CPU fed the device's own fp32 coefficient, with the allowance of
test_clip_and_adamw_vs_reference_fixture_g8 (fewer than 0.1 % of the elements differ, each by at most one bf16 spacing; fp32: rtol 1e-6, atol 1e-9), from moments Adam can reach -- the test's docstring derives why that allowance is sound there.

Outputs are views inside sentinel-filled buffers (refkit.Guarded); everything outside the documented write set must be bitwise
unchanged, const inputs are compared bitwise before and after, all pointers are 16-byte aligned."""
import math

import pytest
import torch

from refkit import (BF, F32, F64, I32, I64, E, U, REL_MATH, TINY, SECOND, PATTERN, NV_ERR_ARG, Guarded, ReadOnly, gamma, gen, randn,
                    randint, dev, bits_equal, check_bound)

pytestmark = pytest.mark.gpu
NEG_INF = float("-inf")


def L():
    from navillm_amd import ops
    return ops._L()


def st():
    from navillm_amd import ops
    return ops._st()


def run(rc, what, expect=0):
    assert rc == expect, f"{what} returned {rc}, expected {expect}"
    torch.cuda.synchronize()


def accum_bound(S, Sa, K, R):
    """bf16(R + bf16(sum)) : the bound of the module docstring"""
    Ek = (K + 1) * E * Sa
    Ei = Ek + U * (S.abs() + Ek)
    return Ei + (U + E) * SECOND * (R.abs() + S.abs() + Ei)


# ============================================================================================== heads
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("N", [1, 3, 100])
@pytest.mark.parametrize("d", [8, 512, 1000, 5120])
def test_bounded_head_fwd_bwd(d, N, B):
    """d = 8 leaves 63 lanes idle, 512 is exactly one pass of the lane loop, 1000 a partly filled second pass (and the `c >= d` cut
    of both backward kernels), 5120 ten passes; N = 1 and 3 leave waves without an output (N % 4 != 0)."""
    g = gen(21, d, N, B)
    x, W, bias, dy = randn(g, B, d), randn(g, N, d, scale=0.5), randn(g, 1, N), randn(g, B, N)
    gW0, gb0 = randn(g, N, d), randn(g, 1, N)
    what = f"head d={d} N={N} B={B}"
    y = Guarded(B, N)
    ro = ReadOnly(x=x, W=W, bias=bias, dy=dy)
    run(L().nv_head_fwd_bf16(x.data_ptr(), W.data_ptr(), bias.data_ptr(), y.view.data_ptr(), B, d, N, st()), what + " fwd")
    x64, W64, b64, dy64 = x.to(F64), W.to(F64), bias.to(F64), dy.to(F64)
    want = x64 @ W64.t() + b64
    Ek = (d + 2) * E * (x64.abs() @ W64.abs().t() + b64.abs())
    check_bound(y.view, want, Ek + U * (want.abs() + Ek), "head_fwd", what)
    y.check(what + " fwd")

    dx, gW, gb = Guarded(B, d), Guarded(N, d, init=gW0, fill=PATTERN[BF]), Guarded(1, N, init=gb0, fill=PATTERN[BF])
    run(L().nv_head_bwd_bf16(dy.data_ptr(), x.data_ptr(), W.data_ptr(), dx.view.data_ptr(), gW.view.data_ptr(), gb.view.data_ptr(), B, d,
                             N, st()), what + " bwd")
    want = dy64 @ W64
    Ek = (N + 1) * E * (dy64.abs() @ W64.abs())
    check_bound(dx.view, want, Ek + U * (want.abs() + Ek), "head_bwd dx", what)
    S, Sa = dy64.t() @ x64, dy64.abs().t() @ x64.abs()
    check_bound(gW.view, gW0.to(F64) + S, accum_bound(S, Sa, B, gW0.to(F64)), "head_bwd gW", what)
    S, Sa = dy64.sum(0, keepdim=True), dy64.abs().sum(0, keepdim=True)
    check_bound(gb.view, gb0.to(F64) + S, accum_bound(S, Sa, B, gb0.to(F64)), "head_bwd gb", what)
    for t in (dx, gW, gb):
        t.check(what + " bwd")
    ro.check(what)


def test_head_fwd_refuses_d_not_multiple_of_8():
    g = gen(22)
    x, W, bias = randn(g, 2, 16), randn(g, 3, 16), randn(g, 1, 3)
    y = Guarded(2, 3)
    run(L().nv_head_fwd_bf16(x.data_ptr(), W.data_ptr(), bias.data_ptr(), y.view.data_ptr(), 2, 12, 3, st()), "nv_head_fwd_bf16 d=12",
        NV_ERR_ARG)
    y.check("head_fwd refusal", torch.zeros(2, 3, dtype=torch.bool, device=dev()))


# ============================================================================================== cross entropy: shared reference
def ce_rows(g, n_rows, C, live_cols):
    """[n_rows, C] bf16 logits by row family (row % 6) and the family names.  live_cols: the columns a target may point at.
       0 normal | 1 -inf slots (never the target's) | 2 base + 60 | 3 base - 60 | 4 base | 5 peaked (every other exp underflows)
    base holds multiples of 0.5 in [-4, 4], so base + 60 and base - 60 are bf16 numbers: rows 2, 3 and 4 have the same loss and the
    same gradient in the reference."""
    base = randint(g, -8, 9, 1, C, dtype=F64) / 2
    lg = randn(g, n_rows, C, scale=2.0).to(F64)
    tgt = live_cols[randint(g, 0, live_cols.numel(), n_rows).long()].clone()
    tgt[(torch.arange(n_rows, device=dev()) % 6 >= 2) & (torch.arange(n_rows, device=dev()) % 6 <= 4)] = live_cols[0]
    for r in range(n_rows):
        f = r % 6
        if f == 1 and C >= 3:
            holes = torch.rand(C, generator=g, device=dev()) < 0.3
            holes[tgt[r]] = False
            lg[r, holes] = NEG_INF
        elif f in (2, 3, 4):
            lg[r] = base[0] + (60.0, -60.0, 0.0)[f - 2]
        elif f == 5:
            lg[r, tgt[r]] = 200.0
    return lg.to(BF), tgt


def ce_reference(l64, tgt, live, gs, D):
    """fp64 loss / gradient of the live rows and their bounds; l64 has -inf in masked columns; tgt: int64 column per row"""
    mx = l64.max(1, keepdim=True).values
    ex = torch.exp(l64 - mx)
    s = ex.sum(1, keepdim=True)
    logs = torch.log(s)
    diff = torch.where(torch.isfinite(l64), (l64 - mx).abs(), torch.zeros_like(l64))
    ds = SECOND * (ex * (REL_MATH + E * diff + gamma(D))).sum(1, keepdim=True) / s
    dlse = SECOND * (ds + REL_MATH * logs.abs()) + E * (mx.abs() + logs.abs())
    lse = mx + logs
    lt = l64.gather(1, tgt[:, None])
    loss = (lse - lt)[:, 0]
    dloss = (dlse + E * (mx.abs() + logs.abs() + lt.abs()))[:, 0]
    p = torch.exp(l64 - lse)
    dl = torch.where(torch.isfinite(l64), (l64 - lse).abs(), torch.zeros_like(l64))
    dp = SECOND * p * (REL_MATH + dlse + E * dl) + TINY
    oh = torch.zeros_like(l64).scatter_(1, tgt[:, None], 1.0)
    grad = gs * (p - oh)
    dg = abs(gs) * (dp + E * (p - oh).abs()) + E * grad.abs()
    dgrad = dg + U * (grad.abs() + dg) + TINY
    z = torch.zeros_like(loss)
    return (torch.where(live, loss, z), torch.where(live, dloss, z), torch.where(live[:, None], grad, torch.zeros_like(grad)),
            torch.where(live[:, None], dgrad, torch.zeros_like(grad)))


# ============================================================================================== action CE
@pytest.mark.parametrize("mode", ["grad", "gscale_dev", "loss_only"])
@pytest.mark.parametrize("G", [1, 9, 64, 65, 100, 130])
def test_bounded_action_ce(G, mode):
    """G = 64 / 65 sit on the lane-stride loop (j += 64), 100 is the model's size, 130 needs a third pass.  Rows 0..5 are the six
    families of ce_rows, row 6 has target -100 and row 7 target G: the kernel treats t >= G as ignored (loss 0, zero gradient) rather
    than reading past the row.  Every live row must be finite although some slots are -inf.  `gscale_dev`: the gradient scale is
    gscale * gscale_dev[0], one fp32 product.  `loss_only`: a null dlogits pointer, only loss_rows is written."""
    g = gen(23, G, len(mode))
    B = 8
    lg, tgt = ce_rows(g, B, G, torch.arange(G, device=dev()))
    tgt = tgt.to(I64)
    tgt[6], tgt[7] = -100, G
    live = (tgt >= 0) & (tgt < G)
    gscale = 0.37
    gd = torch.tensor([1.7], dtype=F32, device=dev()) if mode == "gscale_dev" else None
    gs32 = torch.tensor(gscale, dtype=F32, device=dev())
    gs = (gs32.to(F64) * gd[0].to(F64)).to(F32).item() if gd is not None else gs32.item()
    loss = Guarded(1, B, dtype=F32)
    dl = Guarded(B, G)
    ro = ReadOnly(logits=lg, targets=tgt, **({"gscale_dev": gd} if gd is not None else {}))
    what = f"action_ce G={G} {mode}"
    run(L().nv_action_ce_bf16(lg.data_ptr(), tgt.data_ptr(), loss.view.data_ptr(), None if mode == "loss_only" else dl.view.data_ptr(), B, G,
                              gscale, gd.data_ptr() if gd is not None else None, st()), what)
    want, dwant, grad, dgrad = ce_reference(lg.to(F64), tgt.clamp(0, G - 1), live, gs, math.ceil(G / 64) + 6)
    if G >= 3:
        assert abs(want[2].item() - want[4].item()) < 1e-12 and abs(want[3].item() - want[4].item()) < 1e-12, "shift invariance"
    check_bound(loss.view[0], want, dwant, "action_ce loss", what)
    assert bool((loss.view[0][~live] == 0).all())
    loss.check(what)
    if mode == "loss_only":
        dl.check(what, torch.zeros(B, G, dtype=torch.bool, device=dev()))
    else:
        check_bound(dl.view, grad, dgrad, "action_ce dlogits", what)
        assert bool((dl.view[~live] == 0).all()), "ignored rows must have an all-zero gradient"
        dl.check(what)
    ro.check(what)


# ============================================================================================== LM CE
def lm_case(V, ldl, M, sp, key):
    g = gen(24, V, M, len(sp), key)
    nspecial = 0 if sp == "none" else 5
    special0 = {"none": V // 3, "mid": max(V // 2 - 2, 1), "end": V - 5}[sp]
    cols = torch.arange(V, device=dev())
    is_sp = (cols >= special0) & (cols < special0 + nspecial)
    lg, tgt = ce_rows(g, M, V, cols[~is_sp])
    if nspecial:
        lg[:, special0 + 2] = 300.0                                  # a special column holds every row's largest raw logit
    labels = tgt.to(I32)
    if M > 1:
        labels[M - 2] = -100
    buf = Guarded(M, V, ld=ldl, init=lg, fill=PATTERN[BF])
    return buf, lg, labels, special0, nspecial, is_sp


LM_SHAPES = [(7, 8, 1), (7, 8, 13), (256, 264, 1), (256, 264, 13), (257, 264, 1), (257, 264, 13), (406, 408, 1), (406, 408, 13),
             (32005, 32008, 3)]


@pytest.mark.parametrize("sp", ["none", "mid", "end"])
@pytest.mark.parametrize("V,ldl,M", LM_SHAPES, ids=lambda v: str(v))
def test_bounded_lm_ce(V, ldl, M, sp):
    """V = 256 / 257 sit on the thread-stride loop (j += 256).  nspecial = 0, or five special ids in the middle or at the very end of
    [0, V), one of which holds the row's largest raw logit (300): it must not reach max, loss or gradient -- the reference masks the
    specials to -inf.  Rows are the families of ce_rows (normal, -inf slots, +60 / -60 / unshifted, peaked) plus one ignored row.
    Exact parts: ignored rows become +0 bit patterns in [0, V), special columns of live rows are +0, columns [V, ldl) stay."""
    buf, lg, labels, special0, nspecial, is_sp = lm_case(V, ldl, M, sp, 0)
    loss = Guarded(1, M, dtype=F32)
    ro = ReadOnly(labels=labels)
    gscale = 1.0 / 3.0
    what = f"lm_ce V={V} ldl={ldl} M={M} specials={sp}"
    run(L().nv_lm_ce_bf16(buf.view.data_ptr(), labels.data_ptr(), loss.view.data_ptr(), M, V, ldl, special0, nspecial, gscale, 1, st()), what)
    live = labels >= 0
    l64 = lg.to(F64).masked_fill(is_sp[None], NEG_INF)
    gs = torch.tensor(gscale, dtype=F32).item()
    want, dwant, grad, dgrad = ce_reference(l64, labels.clamp(min=0).long(), live, gs, math.ceil(V / 256) + 10)
    check_bound(loss.view[0], want, dwant, "lm_ce loss", what)
    check_bound(buf.view, grad, dgrad, "lm_ce dlogits", what)
    bits = buf.view.view(torch.int16)
    assert bool((bits[~live] == 0).all()), "ignored rows must be +0 bit patterns"
    assert bool((loss.view[0][~live] == 0).all())
    if nspecial:
        assert bool((bits[live][:, is_sp] == 0).all()), "special columns of live rows must be +0 bit patterns"
    buf.check(what)                                                      # columns [V, ldl) and the guard rows
    loss.check(what)
    ro.check(what)


@pytest.mark.parametrize("sp", ["none", "end"])
@pytest.mark.parametrize("V,ldl,M", [(257, 264, 13), (32005, 32008, 3)], ids=lambda v: str(v))
def test_lm_ce_without_grad_leaves_logits(V, ldl, M, sp):
    """write_grad = 0: the loss is the same, the whole logits buffer is bitwise unchanged (ignored rows included)"""
    buf, lg, labels, special0, nspecial, is_sp = lm_case(V, ldl, M, sp, 1)
    loss = Guarded(1, M, dtype=F32)
    what = f"lm_ce write_grad=0 V={V} M={M} specials={sp}"
    run(L().nv_lm_ce_bf16(buf.view.data_ptr(), labels.data_ptr(), loss.view.data_ptr(), M, V, ldl, special0, nspecial, 1.0, 0, st()), what)
    live = labels >= 0
    l64 = lg.to(F64).masked_fill(is_sp[None], NEG_INF)
    want, dwant, _, _ = ce_reference(l64, labels.clamp(min=0).long(), live, 1.0, math.ceil(V / 256) + 10)
    check_bound(loss.view[0], want, dwant, "lm_ce loss", what)
    buf.check(what, torch.zeros(M, V, dtype=torch.bool, device=dev()))
    loss.check(what)


# ============================================================================================== sumsq / clip_coef
def norm_depth(sizes):
    """D of the module docstring for a list of (n, is_bf16)"""
    T = parts = 0
    for n, is_bf in sizes:
        items = (n + 7) // 8 if is_bf else n
        blocks = min(max((items + 255) // 256, 1), 2048)
        per_thread = math.ceil(items / (blocks * 256))
        T = max(T, (8 * per_thread + 1) if is_bf else per_thread)      # + 1: the scalar tail of a bf16 tensor
        parts += blocks
    return T + 1 + 10 + math.ceil(parts / 256) + 10


@pytest.mark.parametrize("zero", [False, True], ids=["normal", "all-zero"])
def test_bounded_clip_coef_striding(zero):
    """a bf16 tensor of 8 * 524,288 + 8 * 100 + 5 elements (the vector loop strides and the scalar loop reads a ragged tail), an fp32
    tensor of 524,288 + 777 (strides) and a bf16 tensor of 3 elements (tail only).  The norm against fp64 within the derived bound,
    the coefficient exactly from the kernel's own norm; an all-zero list gives norm 0 and coefficient 1."""
    from navillm_amd import ops
    g = gen(25, int(zero))
    sizes = [(8 * 524288 + 8 * 100 + 5, True), (524288 + 777, False), (3, True)]
    gs = []
    for n, is_bf in sizes:
        dt = BF if is_bf else F32
        gs.append(Guarded(1, n, dtype=dt, init=torch.zeros(1, n, dtype=dt, device=dev()) if zero else randn(g, 1, n, dtype=dt), fill=PATTERN[dt]))
    max_norm = 40.0
    out = Guarded(1, 2, dtype=F32)
    coef = ops.clip_coef([t.view[0] for t in gs], max_norm, out2=out.view[0])
    torch.cuda.synchronize()
    tot64 = math.sqrt(sum((t.view.to(F64) ** 2).sum().item() for t in gs))
    D = norm_depth(sizes)
    bound = SECOND * (gamma(D) / 2 + REL_MATH) * tot64
    tot = coef[0].item()
    ratio = abs(tot - tot64) / bound if bound > 0 else (0.0 if tot == 0 else float("inf"))
    print(f"REF_RATIO clip_coef norm | {'all-zero' if zero else 'normal'}: norm {tot!r} fp64 {tot64!r} depth {D} err/bound {ratio:.4f}")
    assert ratio <= 1.0
    t32 = coef[0:1].to(F64)
    c = (torch.tensor([max_norm], dtype=F64, device=dev()) / (t32 + torch.tensor(1e-6, dtype=F32).to(F64)).to(F32).to(F64)).to(F32)
    want = torch.minimum(c, torch.ones_like(c))
    assert bits_equal(coef[1:2], want), (coef[1].item(), want.item())
    if zero:
        assert tot == 0.0 and coef[1].item() == 1.0
    else:
        assert coef[1].item() < 1.0
    out.check("clip_coef")
    for t in gs:
        t.check("clip_coef reads the gradients only", torch.zeros(t.view.shape, dtype=torch.bool, device=dev()))


# ============================================================================================== AdamW at striding sizes
@pytest.mark.parametrize("zero_grad", [False, True], ids=["keep_grad", "zero_grad"])
@pytest.mark.parametrize("dtype,n", [(BF, 8 * 1048576 + 8 * 50 + 3), (F32, 1048576 + 999)], ids=["bf16", "fp32"])
def test_adamw_striding_vs_oracle(dtype, n, zero_grad):
    """more than 4096 x 256 work items: the vector loop strides (bf16: and the scalar tail runs after it).  One step with a clip
    tensor, compared with the oracle's adamw_step_ on the CPU fed the device's own fp32 coefficient.

    The moments are a state Adam can be in: v0 = m0^2 + r^2, so |m0| <= sqrt(v0) (in bf16: up to one rounding of v0).  Adam keeps
    m^2 / v bounded (Cauchy-Schwarz over the two moving averages), which is what bounds the update by a small multiple of lr; the
    fp32 allowance of test_clip_and_adamw_vs_reference_fixture_g8 (rtol 1e-6, atol 1e-9, relative to the RESULT) is only sound
    there.  With |m0| <= sqrt(v0):  m1^2 = (0.9 m0 + 0.1 g)^2 <= (0.81 / 0.999 + 0.01 / 0.001) v1 = 10.9 v1, and at step 3
    den >= sqrt(v1) / sqrt(1 - 0.999^3) = 18.2 sqrt(v1), so |m1 / den| <= 0.19 and the update |step_size m1 / den| <= 3.7e-3 * 0.19
    = 7e-4.  The device may fuse a multiply into the following add and the CPU may not, so in fp32 m1 and v1 may each differ by
    up to 2 e-spacings (e = 2^-24 relative per rounding), the denominator by 1 (sqrt halves v1's) + 3 roundings of its own, the
    quotient and the product with step_size by one each: below 16 e relative of the update = 16 * 6e-8 * 7e-4 = 7e-10 < atol.  The
    final rounding of p can then land on the neighbouring fp32 value: 2 e |p| = 1.2e-7 |p| < rtol |p|.  m1 itself: the two forms of
    m0 + 0.1 (g - m0) differ by one rounding of the product, e * 0.1 |g - m0| <= 6e-9 * 0.2 = 1.2e-9 absolute at the very most (six
    sigma of both) plus one flip of the final rounding, again inside atol + rtol |m1|; v1 is a sum of non-negative terms, two or three
    roundings apart, 4 e relative at most.  A state with v0 far below m0^2 makes updates of the size of p itself, where p - update
    cancels and no bound relative to the result can hold."""
    from navillm_amd import ops
    from util import load_oracle
    O = load_oracle()
    g = gen(26, n, int(zero_grad))
    p0, g0 = randn(g, 1, n, scale=0.05, dtype=dtype), randn(g, 1, n, scale=0.02, dtype=dtype)
    m0 = randn(g, 1, n, scale=0.01, dtype=dtype)
    v0 = (m0.to(F32) ** 2 + randn(g, 1, n, scale=0.01, dtype=F32) ** 2).to(dtype)
    fill = PATTERN[dtype]
    P, G, Mo, Vo = (Guarded(1, n, dtype=dtype, init=t, fill=fill) for t in (p0, g0, m0, v0))
    coef = ops.clip_coef([G.view[0]], 1.0)
    torch.cuda.synchronize()
    assert coef[1].item() < 1.0
    lr, step = 1e-3, 3
    ops.adamw_(P.view[0], G.view[0], Mo.view[0], Vo.view[0], step, lr, clip=coef, zero_grad=zero_grad)
    torch.cuda.synchronize()
    c32 = coef[1].cpu()
    ep, em, ev = p0[0].cpu().clone(), m0[0].cpu().clone(), v0[0].cpu().clone()
    O.adamw_step_(ep, (g0[0].cpu().float() * c32).to(dtype), em, ev, step, lr=lr)
    for name, got, ref, prev in (("p", P.view[0], ep, p0[0]), ("m", Mo.view[0], em, m0[0]), ("v", Vo.view[0], ev, v0[0])):
        got, ref, prev = got.float().cpu(), ref.float(), prev.float().cpu()
        de = (got - ref).abs()
        if dtype == BF:
            spacing = torch.exp2(torch.floor(torch.log2(torch.maximum(ref.abs(), prev.abs()).clamp_min(1e-30))) - 7)
            frac = (de > 0).float().mean().item()
            print(f"[adamw striding {name} zero_grad={zero_grad}] {frac:.4%} of the elements differ (max {(de / spacing).max().item():.2f} spacings)")
            assert frac < 1e-3 and bool((de <= spacing).all()), name
        else:
            assert torch.allclose(got, ref, rtol=1e-6, atol=1e-9), (name, de.max().item())
    if zero_grad:
        assert not bool(G.view.view(torch.int16 if dtype == BF else torch.int32).any()), "the gradient must be all +0 afterwards"
        G.check("adamw zero_grad")
    else:
        G.check("adamw keeps the gradient", torch.zeros(1, n, dtype=torch.bool, device=dev()))
    for t in (P, Mo, Vo):
        t.check("adamw")
