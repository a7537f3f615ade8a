"""GPU: every kernel of csrc/lm_rowops.hip against an fp64 reference that rounds only where the kernel's header comment rounds.

EXACT cases (torch.equal on the bits).  embed_vis, vis_grad, the five RoPE entry points, gather / scatter, scale / scale_dev, the
K/V-gradient accumulator and embed_grad perform at most one correctly rounded fp32 operation between two bf16 roundings, and the
fp64 value of that operation is exact on the data used here, so float64 -> float32 -> bfloat16 (refkit.bf) reproduces them whatever
the data.  embed_grad sums up to 300 rows in fp32: it is made exact with integer data (dE in {-3..3}, the table gradient even
integers up to 510), so that the sum does not depend on its order; the case asserts that it contains a sum above 256 and a tie.

BOUNDED cases (derived, never measured; x = the fp64 value, u, e, REL_MATH, TINY, SECOND as in refkit's docstring):

RMSNorm forward.  Every thread adds its 8 * ceil(d / 2048) squares in turn (a square of a bf16 value is exact in fp32), a 64-lane
butterfly adds 6 levels, the four wave sums are added to a zero: a term passes through at most D = 8 ceil(d/2048) + 10 roundings,
all terms are >= 0, so the sum is within gamma(D) = D e / (1 - D e) of its fp64 value.  The divide by d costs REL_MATH, the add of
eps one e; rsqrtf halves the relative error of its argument and adds REL_MATH of its own:
    |rstd - x| <= SECOND (gamma(D) / 2 + (REL_MATH + e) / 2 + REL_MATH) x =: rho x.
y = bf16(w * bf16(x * rstd)): t = fl(x * rstd) is within (rho + e) of its fp64 value and everything after it (bf16 rounding, an
exact product with w, bf16 rounding) is monotone in t, so y lies between that chain at t (1 - rho - e) and at t (1 + rho + e).

RMSNorm backward (rstd is an fp32 INPUT here, so X = x * rstd etc. use its exact value).  Dh = bf16(dy * w) is reproduced exactly
(one rounding of an exact product).  mean = (1/d) sum Dh X is accumulated like the forward sum, from terms that each carry two more
roundings (xh = fl(x rs), the product): |mean^ - mean| <= dm := SECOND (gamma(D + 2) A / d + REL_MATH |mean|), A = sum |Dh| |X|.
o = fl(rs * fl(Dh - fl(xh * mean^))), O its fp64 value:
    |o - O| <= Eo := SECOND (rs (|X| dm + 3 e |X| |mean| + e |Dh|) + e |O|)
    dx = bf16(o):                      |dx - O|        <= Eo + u (|O| + Eo) =: E1
    dx = bf16(resid + bf16(o)):        |dx - (r + O)|  <= E1 + (u + e) SECOND (|r| + |O| + E1)
gw = bf16(gw0 + bf16(S)), S = sum_m dy * bf16(x rs) whose terms are reproduced exactly; an fp32 sum of M terms in any order is within
Es = (M + 1) e sum |dy xhat| of S:  |gw - (gw0 + S)| <= Ei + (u + e) SECOND (|gw0| + |S| + Ei),  Ei = Es + u (|S| + Es).

SwiGLU.  sg = 1 / (1 + expf(-g)) carries REL_MATH from expf (weighted by e^-g / (1 + e^-g) <= 1), e from the add and REL_MATH from
the divide: rho_s = SECOND (2 REL_MATH + e); the same for silu = g / (1 + expf(-g)) of the forward.  expf(-g) overflows fp32 for
g < -88.72; no bf16 value lies between -88.5 and -89, so the reference knows on which side every input is, and sets the quotient to
(-)0 exactly where the kernel gets x / inf.  Forward: h = bf16(bf16(silu) * u) is monotone in silu: interval check at silu (1 -+
rho_s).  Backward: du = bf16(dh * bf16(fl(g * sg))), interval at q = g sg -+ (|g| (rho_s sg + TINY) + e |q|) -- TINY because sg is
a subnormal fp32 number for g < -87.3; dg = bf16(bf16(dh u) * sp), sp = sg (1 + g (1 - sg)) evaluated left to right in fp32:
    a = 1 - sg : da = rho_s sg + TINY + e |a| ;  b = g a : db = |g| da + e |b| ;  t = 1 + b : dt = db + e |t|
    sp = sg t  : dsp = SECOND (sg dt + |t| (rho_s sg + TINY) + e |sp|) ;  w = P sp : dw = |P| dsp + e (|w| + |P| dsp)
and dg lies between bf16(w - dw) and bf16(w + dw).  The interval is a point wherever no rounding boundary falls inside it.

Every output is a view inside a sentinel-filled buffer (refkit.Guarded) and everything outside the documented write set must be
bitwise unchanged; every const input is compared bitwise before and after.  All pointers are 16-byte aligned."""
import math

import pytest
import torch

from refkit import (BF, F32, F64, I32, E, U, REL_MATH, TINY, SECOND, PATTERN, NV_ERR_ARG, NV_ERR_SHAPE, Guarded, ReadOnly, bf, f32r,
                    gamma, gen, randn, randint, randperm, dev, bits_equal, check_bound, check_interval, bf_round_int)

pytestmark = pytest.mark.gpu


def L():
    from navillm_amd import ops
    return ops._L()


def st():
    from navillm_amd import ops
    return ops._st()


def run(rc, what, expect=0):
    assert rc == expect, f"{what} returned {rc}, expected {expect}"
    torch.cuda.synchronize()


def row_mask(rows_total, width, rows):
    m = torch.zeros(rows_total, width, dtype=torch.bool, device=dev())
    m[rows.long()] = True
    return m


# ============================================================================================== embed_vis / vis_grad
def vis_layout(g, M):
    """vis_idx[m] >= 0 on the first row, the last row and a run of adjacent rows, -1 elsewhere; the indices are a permutation"""
    rows = sorted({0, M - 1} | {r for r in (3, 4, 5) if r < M} | {r for r in range(1000, M, 2)})
    vis_idx = torch.full((M,), -1, dtype=I32, device=dev())
    vis_idx[torch.tensor(rows, device=dev())] = randperm(g, len(rows))
    return vis_idx, len(rows)


@pytest.mark.parametrize("M,d", [(1, 8), (1, 256), (1, 4096), (40, 8), (40, 256), (40, 4096), (1030, 4096)],
                         ids=lambda v: str(v))
def test_exact_embed_vis(M, d):
    """out = table[ids] or bf16(f32(table[ids]) + vis[vis_idx]) (single rounding).  (1030, 4096) is 527,360 vectors: the grid strides
    and the rows reached by the second pass include visual ones."""
    g = gen(1, M, d)
    V = 53
    table, ids = randn(g, V, d), randint(g, 0, V, M)
    vis_idx, nv = vis_layout(g, M)
    vis = randn(g, nv, d, dtype=F32)
    out = Guarded(M, d)
    ro = ReadOnly(table=table, ids=ids, vis_idx=vis_idx, vis=vis)
    run(L().nv_embed_vis_bf16(table.data_ptr(), ids.data_ptr(), vis_idx.data_ptr(), vis.data_ptr(), out.view.data_ptr(), M, d, st()),
        "nv_embed_vis_bf16")
    t64 = table[ids.long()].to(F64)
    add = torch.where((vis_idx >= 0)[:, None], vis[vis_idx.clamp(min=0).long()].to(F64), torch.zeros_like(t64))
    want = bf(t64 + add)
    assert bits_equal(out.view, want), f"embed_vis {M}x{d}: {int((out.view != want).sum())} elements differ"
    out.check("embed_vis")
    ro.check("embed_vis")


def test_exact_embed_vis_no_visual_rows_null_vis():
    """zero visual rows: vis may be a null pointer (ops.embed_vis passes one); the output is the plain gather"""
    M, d = 40, 256
    g = gen(2, M, d)
    table, ids = randn(g, 31, d), randint(g, 0, 31, M)
    vis_idx = torch.full((M,), -1, dtype=I32, device=dev())
    out = Guarded(M, d)
    run(L().nv_embed_vis_bf16(table.data_ptr(), ids.data_ptr(), vis_idx.data_ptr(), None, out.view.data_ptr(), M, d, st()),
        "nv_embed_vis_bf16")
    assert bits_equal(out.view, table[ids.long()])
    out.check("embed_vis (no visual rows)")


@pytest.mark.parametrize("M,d", [(1, 8), (1, 256), (1, 4096), (40, 8), (40, 256), (40, 4096), (1030, 4096)], ids=lambda v: str(v))
def test_exact_vis_grad(M, d):
    """dvis[i] = f32(dE[vis_rows[i]]); at M = 1030 every row is listed (in permuted order): 527,360 vectors, the grid strides"""
    g = gen(3, M, d)
    dE = randn(g, M, d)
    if M == 1030:
        rows = randperm(g, M)
    else:
        vis_idx, _ = vis_layout(g, M)
        rows = torch.nonzero(vis_idx >= 0).flatten().to(I32)
        rows = rows[randperm(g, rows.numel()).long()]
    n = rows.numel()
    out = Guarded(n, d, dtype=F32)
    ro = ReadOnly(dE=dE, rows=rows)
    run(L().nv_vis_grad_f32(dE.data_ptr(), rows.data_ptr(), out.view.data_ptr(), n, d, st()), "nv_vis_grad_f32")
    assert bits_equal(out.view, dE[rows.long()].to(F32))
    out.check("vis_grad")
    ro.check("vis_grad")


# ============================================================================================== embed_grad
@pytest.mark.parametrize("d", [8, 2048, 4096])
def test_exact_embed_grad(d):
    """gtable[uniq[u]] = bf16(g0 + bf16(sum over segment u of dE[tok])) with segments of 1, 2 and 300 tokens; at d = 4096 the column
    loop (c += 2048) runs twice.  dE holds integers in {-3..3} (a third of the columns only positive, a third only negative ones, so
    that the long segment passes 256), g0 even integers up to 510: every fp32 sum is exact in any order."""
    g = gen(4, d)
    lens = [1, 300, 2]
    T, V = sum(lens), 11
    col = torch.arange(d, device=dev()) % 3
    dE = randint(g, -3, 4, T + 5, d, dtype=torch.int64)
    dE = torch.where(col == 0, dE.abs().clamp(min=1), torch.where(col == 1, -dE.abs().clamp(min=1), dE)).to(BF)
    tok = randperm(g, T + 5)[:T].contiguous()
    uniq = randperm(g, V)[:3].contiguous()
    seg = torch.tensor([0, 1, 301, 303], dtype=I32, device=dev())
    g0 = (2 * randint(g, -255, 256, V, d, dtype=torch.int64)).to(BF)
    gt = Guarded(V, d, init=g0, fill=PATTERN[BF])
    ro = ReadOnly(dE=dE, tok=tok, uniq=uniq, seg=seg)
    run(L().nv_embed_grad_bf16(dE.data_ptr(), uniq.data_ptr(), seg.data_ptr(), tok.data_ptr(), gt.view.data_ptr(), 3, d, st()),
        "nv_embed_grad_bf16")
    want = g0.clone()
    ties = big = 0
    bounds, urows = seg.tolist(), uniq.tolist()
    for u in range(3):
        s = dE[tok[bounds[u]:bounds[u + 1]].long()].to(F64).sum(0)
        si = s.to(torch.int64)
        inner_i, tie_i, big_i = bf_round_int(si)
        assert torch.equal(bf(s).to(F64), inner_i.to(F64)), "reference rounding disagrees with integer arithmetic"
        pre = inner_i + g0[urows[u]].to(torch.int64)
        want_i, tie_o, _ = bf_round_int(pre)
        want[urows[u]] = bf(pre.to(F64))
        assert torch.equal(want[urows[u]].to(F64), want_i.to(F64))
        ties += int(tie_i.sum()) + int(tie_o.sum())
        big += int(big_i.sum())
    assert ties > 0 and big > 0, f"case has no tie / no segment sum above 256 (ties {ties}, big {big})"
    assert bits_equal(gt.view, want), f"embed_grad d={d}: {int((gt.view != want).sum())} elements differ"
    gt.check("embed_grad", row_mask(V, d, uniq))
    ro.check("embed_grad")


# ============================================================================================== RoPE
MAXS = 37


def rope_tables(g, hd, kind):
    """[MAXS, hd] bf16 cos and sin.  `hf`: as HF builds them, the two halves of a row identical.  `indep`: the second half holds
    unrelated numbers -- the kernels read only the first hd/2 entries of a row, so both must give the reference's result."""
    half = hd // 2
    inv = 1.0 / (10000.0 ** (torch.arange(0, half, device=dev(), dtype=F64) / half))
    ang = torch.arange(MAXS, device=dev(), dtype=F64)[:, None] * inv[None]
    c, s = ang.cos().to(BF), ang.sin().to(BF)
    if kind == "hf":
        return torch.cat([c, c], 1).contiguous(), torch.cat([s, s], 1).contiguous()
    return torch.cat([c, randn(g, MAXS, half)], 1).contiguous(), torch.cat([s, randn(g, MAXS, half)], 1).contiguous()


def rope_reference(x, cos_t, sin_t, pos, H, hd, sign):
    """bf16( bf16(x1 c) + bf16(-+ x2 s) ) | bf16( bf16(x2 c) + bf16(+- x1 s) ) on the q and k heads; x: [M, 3 H hd] bf16"""
    M, half = x.shape[0], hd // 2
    qk = x[:, :2 * H * hd].to(F64).reshape(M, 2 * H, 2, half)
    c = cos_t[pos.long(), :half].to(F64)[:, None, :]
    s = sin_t[pos.long(), :half].to(F64)[:, None, :]
    x1, x2 = qk[:, :, 0], qk[:, :, 1]
    o1 = bf(bf(x1 * c).to(F64) + bf(-sign * x2 * s).to(F64))
    o2 = bf(bf(x2 * c).to(F64) + bf(sign * x1 * s).to(F64))
    out = x.clone()
    out[:, :2 * H * hd] = torch.stack([o1, o2], 2).reshape(M, 2 * H * hd)
    return out


def positions(g, M):
    pos = randint(g, 0, MAXS, M)
    for i, v in enumerate((0, MAXS - 1, 11, 11)):
        if i < M:
            pos[i] = v
    return pos


def rope_inplace_case(hd, H, pad, M, kinds=("hf", "indep")):
    S = 7
    assert M % S != 0
    for kind in kinds:
        for entry in ("fwd", "bwd", "rows", "rows_t"):
            g = gen(5, hd, H, pad, M, len(kind), len(entry))
            cos_t, sin_t = rope_tables(g, hd, kind)
            W = 3 * H * hd
            x = randn(g, M, W)
            buf = Guarded(M, W, ld=W + pad, init=x, fill=PATTERN[BF])
            pos = positions(g, M) if entry.startswith("rows") else (torch.arange(M, device=dev()) % S).to(I32)
            ro = ReadOnly(cos=cos_t, sin=sin_t, pos=pos)
            p = (buf.view.data_ptr(), cos_t.data_ptr(), sin_t.data_ptr())
            what = f"rope {entry} hd={hd} H={H} ld={W + pad} M={M} tables={kind}"
            if entry in ("fwd", "bwd"):
                run(L().nv_rope_bf16(*p, M, S, H, hd, W + pad, 1 if entry == "bwd" else 0, st()), what)
            elif entry == "rows":
                run(L().nv_rope_rows_bf16(*p, pos.data_ptr(), M, H, hd, W + pad, st()), what)
            else:
                run(L().nv_rope_rows_t_bf16(*p, pos.data_ptr(), M, H, hd, W + pad, st()), what)
            want = rope_reference(x, cos_t, sin_t, pos, H, hd, -1.0 if entry in ("bwd", "rows_t") else 1.0)
            assert bits_equal(buf.view, want), f"{what}: {int((buf.view != want).sum())} elements differ"
            buf.check(what, (slice(None), slice(0, 2 * H * hd)))         # the v columns and the pad columns stay
            ro.check(what)


@pytest.mark.parametrize("pad", [0, 8], ids=["ld=3Hhd", "ld=3Hhd+8"])
@pytest.mark.parametrize("H", [1, 3, 32])
@pytest.mark.parametrize("hd", [16, 64, 128])
def test_exact_rope_inplace(hd, H, pad):
    """nv_rope_bf16 forward and backward (position m % S, M = 13, S = 7), nv_rope_rows_bf16 and nv_rope_rows_t_bf16 (random positions
    with 0, MAXS - 1 and a repeated one), with HF tables and with tables whose second halves are independent"""
    rope_inplace_case(hd, H, pad, 13)


@pytest.mark.parametrize("H,hd", [(32, 128), (64, 64)], ids=["hd128", "hd64"])
def test_exact_rope_inplace_striding(H, hd):
    """M = 1030: 527,360 work items, more than the 2048 x 256 threads of the capped grid"""
    assert 1030 * 2 * H * hd // 16 > 524288
    rope_inplace_case(hd, H, 8, 1030, kinds=("indep",))


def rope_scatter_case(hd, H, M):
    g = gen(6, hd, H, M)
    cos_t, sin_t = rope_tables(g, hd, "indep")
    W, R = 3 * H * hd, M + 7
    src = randn(g, M, W)
    pos = positions(g, M)
    rows = randperm(g, R)[:M].contiguous()
    dst = Guarded(R, W)
    ro = ReadOnly(src=src, cos=cos_t, sin=sin_t, pos=pos, rows=rows)
    what = f"rope_scatter hd={hd} H={H} M={M}"
    run(L().nv_rope_scatter_rows_bf16(src.data_ptr(), cos_t.data_ptr(), sin_t.data_ptr(), pos.data_ptr(), rows.data_ptr(),
                                      dst.view.data_ptr(), M, H, hd, W, st()), what)
    want = rope_reference(src, cos_t, sin_t, pos, H, hd, 1.0)
    assert bits_equal(dst.view[rows.long()], want), f"{what}: {int((dst.view[rows.long()] != want).sum())} elements differ"
    dst.check(what, row_mask(R, W, rows))
    ro.check(what)                                                       # src in particular


@pytest.mark.parametrize("H", [1, 3, 32])
@pytest.mark.parametrize("hd", [16, 64, 128])
def test_exact_rope_scatter(hd, H):
    """dst[rows[m]] = [rope(q) | rope(k) | v] of src row m at pos[m]; rows is a random subset of dst's rows, src stays untouched"""
    rope_scatter_case(hd, H, 13)


def test_exact_rope_scatter_striding():
    """M = 520, H = 32, hd = 128: 266,240 rotation items + 266,240 copy items = 532,480 > 524,288, so the grid strides and the
    `i < n_rope` boundary lies in the middle of the first pass"""
    rope_scatter_case(128, 32, 520)


def test_rope_refusals():
    """head_dim 24 (not a multiple of 16) is NV_ERR_ARG at every entry point, and so is ld != 3 H hd at rope_scatter; nothing is
    written"""
    g = gen(7)
    M, H = 4, 2
    for hd, ld_extra in ((24, 0), (32, 8)):
        W = 3 * H * hd
        cos_t, sin_t = randn(g, MAXS, hd), randn(g, MAXS, hd)
        x = Guarded(M, W, ld=W + ld_extra, init=randn(g, M, W), fill=PATTERN[BF])
        dst = Guarded(M, W, ld=W + ld_extra)
        pos, rows = positions(g, M), randperm(g, M)
        p = (x.view.data_ptr(), cos_t.data_ptr(), sin_t.data_ptr())
        if hd == 24:
            run(L().nv_rope_bf16(*p, M, 3, H, hd, W, 0, st()), "nv_rope_bf16 hd=24", NV_ERR_ARG)
            run(L().nv_rope_bf16(*p, M, 3, H, hd, W, 1, st()), "nv_rope_bf16 backward hd=24", NV_ERR_ARG)
            run(L().nv_rope_rows_bf16(*p, pos.data_ptr(), M, H, hd, W, st()), "nv_rope_rows_bf16 hd=24", NV_ERR_ARG)
            run(L().nv_rope_rows_t_bf16(*p, pos.data_ptr(), M, H, hd, W, st()), "nv_rope_rows_t_bf16 hd=24", NV_ERR_ARG)
        run(L().nv_rope_scatter_rows_bf16(*p, pos.data_ptr(), rows.data_ptr(), dst.view.data_ptr(), M, H, hd, W + ld_extra, st()),
            f"nv_rope_scatter_rows_bf16 hd={hd} ld={W + ld_extra}", NV_ERR_ARG)
        x.check("rope refusal", torch.zeros(M, W, dtype=torch.bool, device=dev()))
        dst.check("rope_scatter refusal", torch.zeros(M, W, dtype=torch.bool, device=dev()))


# ============================================================================================== gather / scatter
@pytest.mark.parametrize("n,d", [(1, 8), (1, 4096), (37, 8), (37, 4096), (1030, 4096)], ids=lambda v: str(v))
def test_exact_gather_scatter_rows(n, d):
    """gather with repeated rows, scatter with unique rows (its contract); (1030, 4096) is 527,360 vectors: the grid strides"""
    g = gen(8, n, d)
    R = 23
    src = randn(g, R, d)
    rows = randint(g, 0, R, n)
    if n > 1:
        rows[1] = rows[0]
    out = Guarded(n, d)
    ro = ReadOnly(src=src, rows=rows)
    run(L().nv_gather_rows_bf16(src.data_ptr(), rows.data_ptr(), out.view.data_ptr(), n, d, st()), "nv_gather_rows_bf16")
    assert bits_equal(out.view, src[rows.long()])
    out.check("gather_rows")
    ro.check("gather_rows")

    R = n + 9
    src = randn(g, n, d)
    rows = randperm(g, R)[:n].contiguous()
    dst = Guarded(R, d)
    ro = ReadOnly(src=src, rows=rows)
    run(L().nv_scatter_rows_bf16(src.data_ptr(), rows.data_ptr(), dst.view.data_ptr(), n, d, st()), "nv_scatter_rows_bf16")
    assert bits_equal(dst.view[rows.long()], src)
    dst.check("scatter_rows", row_mask(R, d, rows))
    ro.check("scatter_rows")


# ============================================================================================== scale
@pytest.mark.parametrize("scale", [1.0, 0.125, 1.0 / 3.0, -2.5], ids=["1", "1/8", "1/3", "-2.5"])
@pytest.mark.parametrize("n", [8, 8 * 1000, 8 * 524288 + 8 * 300])
def test_exact_scale(n, scale):
    """nv_scale_bf16 out of place and in place (ops.scale_bf16_), nv_scale_dev_bf16 plain and accumulating
    (out = bf16(out + bf16(x * s))).  The kernel multiplies by the fp32 value of the scale: the reference uses exactly that value.
    The largest n is 524,588 vectors: the grid strides."""
    from navillm_amd import ops
    g = gen(9, n, int(scale * 1000))
    x = randn(g, 1, n)
    s32 = torch.tensor([scale], dtype=F32, device=dev())
    want = bf(x.to(F64) * s32.to(F64))
    out = Guarded(1, n)
    ro = ReadOnly(x=x, s=s32)
    run(L().nv_scale_bf16(x.data_ptr(), out.view.data_ptr(), n, scale, st()), "nv_scale_bf16")
    assert bits_equal(out.view, want), "scale_bf16"
    out.check("scale_bf16")
    inp = Guarded(1, n, init=x, fill=PATTERN[BF])
    ops.scale_bf16_(inp.view, scale)
    torch.cuda.synchronize()
    assert bits_equal(inp.view, want), "scale_bf16_ in place"
    inp.check("scale_bf16_ in place")
    out = Guarded(1, n)
    run(L().nv_scale_dev_bf16(x.data_ptr(), out.view.data_ptr(), n, s32.data_ptr(), 0, st()), "nv_scale_dev_bf16")
    assert bits_equal(out.view, want), "scale_dev_bf16"
    out.check("scale_dev_bf16")
    o0 = randn(g, 1, n)
    out = Guarded(1, n, init=o0, fill=PATTERN[BF])
    run(L().nv_scale_dev_bf16(x.data_ptr(), out.view.data_ptr(), n, s32.data_ptr(), 1, st()), "nv_scale_dev_bf16 accumulate")
    assert bits_equal(out.view, bf(o0.to(F64) + want.to(F64))), "scale_dev_bf16 accumulate"
    out.check("scale_dev_bf16 accumulate")
    ro.check("scale")


def test_scale_refuses_n_not_multiple_of_8():
    g = gen(10)
    x, s32 = randn(g, 1, 16), torch.ones(1, dtype=F32, device=dev())
    out = Guarded(1, 16)
    run(L().nv_scale_bf16(x.data_ptr(), out.view.data_ptr(), 12, 2.0, st()), "nv_scale_bf16 n=12", NV_ERR_ARG)
    run(L().nv_scale_dev_bf16(x.data_ptr(), out.view.data_ptr(), 12, s32.data_ptr(), 0, st()), "nv_scale_dev_bf16 n=12", NV_ERR_ARG)
    run(L().nv_scale_dev_bf16(x.data_ptr(), out.view.data_ptr(), 12, s32.data_ptr(), 1, st()), "nv_scale_dev_bf16 n=12", NV_ERR_ARG)
    out.check("scale refusal", torch.zeros(1, 16, dtype=torch.bool, device=dev()))


# ============================================================================================== kv_grad set / accum / inject
@pytest.mark.parametrize("n,d", [(1, 8), (1, 512), (33, 8), (33, 512), (520, 4096)], ids=lambda v: str(v))
def test_exact_kv_grad_set_accum_inject(n, d):
    """acc[rows] = f32(K/V columns of dqkv1) (set: the NaN sentinel must not be read), then += dqkv2, += dqkv3 (each one fp32 add of an
    fp32 and a bf16 value: exact in fp64, so the reference repeats them in the same order), then
    packed[i, d:3d] = bf16(f32(packed[i, d:3d]) + acc[rows[i]]).  rows is a random subset of the accumulator's rows, so the accumulator
    row differs from the packed row; (520, 4096) is 532,480 vectors: the grid strides."""
    g = gen(11, n, d)
    R = n + 6
    rows = randperm(g, R)[:n].contiguous()
    dq = [randn(g, R, 3 * d) for _ in range(3)]
    acc = Guarded(R, 2 * d, dtype=F32)
    ro = ReadOnly(rows=rows, dq0=dq[0], dq1=dq[1], dq2=dq[2])
    kv = lambda t: t[rows.long(), d:].to(F64)
    written = row_mask(R, 2 * d, rows)
    run(L().nv_kv_grad_set_f32(dq[0].data_ptr(), acc.view.data_ptr(), rows.data_ptr(), n, d, st()), "nv_kv_grad_set_f32")
    want = f32r(kv(dq[0]))
    assert bits_equal(acc.view[rows.long()], want), "kv_grad_set"
    acc.check("kv_grad_set", written)
    for t in dq[1:]:
        run(L().nv_kv_grad_accum_f32(t.data_ptr(), acc.view.data_ptr(), rows.data_ptr(), n, d, st()), "nv_kv_grad_accum_f32")
        want = f32r(want.to(F64) + kv(t))
    assert bits_equal(acc.view[rows.long()], want), "kv_grad_accum"
    acc.check("kv_grad_accum", written)
    ro.check("kv_grad set/accum")

    p0 = randn(g, n, 3 * d)
    packed = Guarded(n, 3 * d, init=p0, fill=PATTERN[BF])
    acc.rearm()
    run(L().nv_kv_grad_inject_bf16(packed.view.data_ptr(), acc.view.data_ptr(), rows.data_ptr(), n, d, st()), "nv_kv_grad_inject_bf16")
    want_p = p0.clone()
    want_p[:, d:] = bf(p0[:, d:].to(F64) + want.to(F64))
    assert bits_equal(packed.view, want_p), "kv_grad_inject"
    packed.check("kv_grad_inject", (slice(None), slice(d, 3 * d)))       # the q columns stay
    acc.check("kv_grad_inject reads acc only", torch.zeros(R, 2 * d, dtype=torch.bool, device=dev()))
    ro.check("kv_grad_inject")


# ============================================================================================== RMSNorm forward
def row_scales(M):
    """1e-3, 30, 1, ... : a bound scaled by the global maximum would hide a wrong small row"""
    return torch.tensor([(1e-3, 30.0, 1.0)[m % 3] for m in range(M)], dtype=F64, device=dev())[:, None]


def rstd_rho(d):
    D = 8 * math.ceil(d / 2048) + 10
    return SECOND * (gamma(D) / 2 + (REL_MATH + E) / 2 + REL_MATH)


@pytest.mark.parametrize("eps", [1e-6, 1e-5])
@pytest.mark.parametrize("M", [1, 5])
@pytest.mark.parametrize("d", [8, 24, 1000, 2048, 2056, 5120, 8192, 8200])
def test_bounded_rmsnorm_fwd(d, M, eps):
    """rstd within rho x, y inside the interval of the module docstring; rows of scale 1e-3, 30 and 1; at M = 5 the last row is all
    zero: rstd = rsqrt(eps) must be finite and y exactly zero.  A second launch passes a null rstd pointer (C ABI) and must give the
    same y."""
    g = gen(12, d, M, int(eps * 1e7))
    x = bf(randn(g, M, d).to(F64) * row_scales(M))
    if M == 5:
        x[4] = 0
    w = bf(1.0 + 0.3 * randn(g, 1, d).to(F64))[0]
    y, rs = Guarded(M, d), Guarded(1, M, dtype=F32)
    ro = ReadOnly(x=x, w=w)
    what = f"rmsnorm_fwd M={M} d={d} eps={eps}"
    run(L().nv_rmsnorm_fwd_bf16(x.data_ptr(), w.data_ptr(), y.view.data_ptr(), rs.view.data_ptr(), M, d, eps, st()), what)
    eps32 = torch.tensor(eps, dtype=F32, device=dev()).to(F64)
    x64 = x.to(F64)
    r64 = 1.0 / torch.sqrt((x64 * x64).sum(1) / d + eps32)
    rho = rstd_rho(d)
    check_bound(rs.view[0], r64, rho * r64, "rmsnorm_fwd rstd", what)
    t = x64 * r64[:, None]
    dt = (rho + E) * t.abs()
    w64 = w.to(F64)[None]
    check_interval(y.view, bf(w64 * bf(t - dt).to(F64)), bf(w64 * bf(t + dt).to(F64)), "rmsnorm_fwd y", what)
    if M == 5:
        assert bool((y.view[4] == 0).all()) and math.isfinite(rs.view[0, 4].item())
    y.check(what)
    rs.check(what)
    y2 = Guarded(M, d)
    run(L().nv_rmsnorm_fwd_bf16(x.data_ptr(), w.data_ptr(), y2.view.data_ptr(), None, M, d, eps, st()), what + " (null rstd)")
    assert bits_equal(y2.view, y.view), "null rstd changes y"
    y2.check(what + " (null rstd)")
    ro.check(what)


# ============================================================================================== RMSNorm backward
def rmsnorm_bwd_case(M, d, resid):
    g = gen(13, M, d, int(resid))
    blk = torch.arange(M, device=dev()) // 1024                       # rows m and m + 1024 are walked by the same block
    xs = torch.tensor([1.0, 25.0, 0.04], dtype=F64, device=dev())[blk][:, None]
    ds = torch.tensor([1.0, 0.05, 8.0], dtype=F64, device=dev())[blk][:, None]
    x = bf(randn(g, M, d).to(F64) * xs)
    dy = bf(randn(g, M, d).to(F64) * ds)
    w = bf(1.0 + 0.3 * randn(g, 1, d).to(F64))[0]
    rg = randn(g, M, d) if resid else None
    gw0 = randn(g, 1, d)
    x64, dy64, w64 = x.to(F64), dy.to(F64), w.to(F64)[None]
    rstd = f32r(1.0 / torch.sqrt((x64 * x64).sum(1) / d + 1e-6))    # an fp32 INPUT of the backward: any positive values would do
    rs = rstd.to(F64)[:, None]
    dx = Guarded(M, d)
    gw = Guarded(1, d, init=gw0, fill=PATTERN[BF])
    ws = torch.empty(L().nv_rmsnorm_bwd_workspace_bytes(d) // 4, dtype=F32, device=dev())
    ro = ReadOnly(dy=dy, x=x, w=w, rstd=rstd, **({"resid_grad": rg} if resid else {}))
    what = f"rmsnorm_bwd M={M} d={d} resid={int(resid)}"
    run(L().nv_rmsnorm_bwd_bf16(dy.data_ptr(), x.data_ptr(), w.data_ptr(), rstd.data_ptr(), rg.data_ptr() if resid else None,
                                dx.view.data_ptr(), gw.view.data_ptr(), ws.data_ptr(), M, d, st()), what)
    D = 8 * math.ceil(d / 2048) + 10
    X = x64 * rs
    Dh = bf(dy64 * w64).to(F64)
    mean = (Dh * X).sum(1, keepdim=True) / d
    A = (Dh.abs() * X.abs()).sum(1, keepdim=True)
    dm = SECOND * (gamma(D + 2) * A / d + REL_MATH * mean.abs())
    O = rs * (Dh - X * mean)
    Eo = SECOND * (rs * (X.abs() * dm + 3 * E * X.abs() * mean.abs() + E * Dh.abs()) + E * O.abs())
    E1 = Eo + U * (O.abs() + Eo)
    if resid:
        r64 = rg.to(F64)
        check_bound(dx.view, r64 + O, E1 + (U + E) * SECOND * (r64.abs() + O.abs() + E1), "rmsnorm_bwd dx", what)
    else:
        check_bound(dx.view, O, E1, "rmsnorm_bwd dx", what)
    T = dy64 * bf(X).to(F64)                                            # over ALL rows: every block's carried partial counts
    S, Sa = T.sum(0), T.abs().sum(0)
    Es = (M + 1) * E * Sa
    Ei = Es + U * (S.abs() + Es)
    g64 = gw0[0].to(F64)
    check_bound(gw.view[0], g64 + S, Ei + (U + E) * SECOND * (g64.abs() + S.abs() + Ei), "rmsnorm_bwd gw", what)
    dx.check(what)
    gw.check(what)
    ro.check(what)


@pytest.mark.parametrize("resid", [False, True], ids=["plain", "resid"])
@pytest.mark.parametrize("M", [1, 17, 63, 64, 65, 1024, 1025, 2100])
def test_bounded_rmsnorm_bwd_rows(M, resid):
    """d = 256.  M = 63 / 64 / 65 sit on the 4-way unrolled loop of the partial reduction (p + 48 < P), M > 1024 makes a block walk
    two or three rows (scales 1 / 25 / 0.04 in x and 1 / 0.05 / 8 in dy for rows m, m + 1024, m + 2048): a `dot`, an xhat or a reduction
    buffer left over from the previous row would be far outside the per-row bound, and gw is checked against the sum over all rows."""
    rmsnorm_bwd_case(M, 256, resid)


@pytest.mark.parametrize("resid", [False, True], ids=["plain", "resid"])
@pytest.mark.parametrize("M,d", [(3, 8192), (5, 8), (5, 24), (40, 1000), (40, 5120)], ids=lambda v: str(v))
def test_bounded_rmsnorm_bwd_widths(M, d, resid):
    """d = 8 and 24 leave most of the block idle and end the reduction grid inside a block of 16 columns (c < d); 1000 and 5120 end
    inside a vector pass; 8192 is the widest the kernel takes"""
    rmsnorm_bwd_case(M, d, resid)


def test_rmsnorm_bwd_refuses_d_above_8192():
    M, d = 2, 8200
    g = gen(14)
    x, dy, w = randn(g, M, d), randn(g, M, d), randn(g, 1, d)
    rstd = torch.ones(M, dtype=F32, device=dev())
    dx, gw = Guarded(M, d), Guarded(1, d, init=randn(g, 1, d), fill=PATTERN[BF])
    ws = Guarded(1, L().nv_rmsnorm_bwd_workspace_bytes(d) // 4, dtype=F32)
    run(L().nv_rmsnorm_bwd_bf16(dy.data_ptr(), x.data_ptr(), w.data_ptr(), rstd.data_ptr(), None, dx.view.data_ptr(),
                                gw.view.data_ptr(), ws.view.data_ptr(), M, d, st()), "nv_rmsnorm_bwd_bf16 d=8200", NV_ERR_SHAPE)
    none = lambda t: torch.zeros(t.view.shape, dtype=torch.bool, device=dev())
    dx.check("refusal: dx", none(dx))
    gw.check("refusal: gw", none(gw))
    ws.check("refusal: workspace", none(ws))


# ============================================================================================== SwiGLU
def sweep_values():
    """bf16 gate values over [-90, 90] with +-0, +-20, +-88 and the two neighbours of the fp32 overflow of expf(-g) (-88.5, -89)"""
    v = torch.cat([torch.linspace(-90, 90, 1441, device=dev(), dtype=F64),
                   torch.tensor([0.0, -0.0, 20.0, -20.0, 88.0, -88.0, -88.5, -89.0, 88.5, 89.0, -87.5, -90.0, 90.0], device=dev(), dtype=F64)])
    return v.to(BF)


def swiglu_inputs(M, ff, key, sweep):
    g = gen(15, M, ff, key, int(sweep))
    gu = randn(g, M, 2 * ff, scale=2.0)
    dh = randn(g, M, ff, scale=2.0)
    if sweep:
        sv = sweep_values()
        k = min(sv.numel(), M * ff)
        idx = torch.arange(k, device=dev())
        r, c = idx // ff, idx % ff
        sign = lambda: (randint(g, 0, 2, k, dtype=F64) * 2 - 1)
        mag = lambda: 0.5 + 1.5 * torch.rand(k, generator=g, device=dev(), dtype=F64)
        gu[r, c] = sv[-k:]
        gu[r, ff + c] = (sign() * mag()).to(BF)                       # |u|, |dh| in [0.5, 2]: no product falls below the normal range
        dh[r, c] = (sign() * mag()).to(BF)
    return gu, dh


def sigmoid_parts(g64):
    """(sg, silu, overflow) in fp64 with the fp32 overflow of expf(-g) applied: e^-g >= 2^128 gives sg = 0 and silu = -0 exactly"""
    ex = torch.exp(-g64)
    over = ex >= 2.0 ** 128
    sg = torch.where(over, torch.zeros_like(g64), 1.0 / (1.0 + ex))
    silu = torch.where(over, -torch.zeros_like(g64), g64 / (1.0 + ex))
    return sg, silu, over


RHO_S = SECOND * (2 * REL_MATH + E)


@pytest.mark.parametrize("sweep", [False, True], ids=["normal", "sweep"])
@pytest.mark.parametrize("M,ff", [(1, 8), (1, 1408), (123, 8), (123, 1408), (600, 7040)], ids=lambda v: str(v))
def test_bounded_swiglu_fwd(M, ff, sweep):
    """h = bf16(bf16(silu(g)) * u).  (600, 7040) is 528,000 vectors: the grid strides.  The sweep cases must stay finite: silu(g) is a
    finite -0 below the overflow of expf(-g)."""
    gu, _ = swiglu_inputs(M, ff, 0, sweep)
    h = Guarded(M, ff)
    ro = ReadOnly(gu=gu)
    what = f"swiglu_fwd M={M} ff={ff} {'sweep' if sweep else 'normal'}"
    run(L().nv_swiglu_fwd_bf16(gu.data_ptr(), h.view.data_ptr(), M, ff, st()), what)
    g64, u64 = gu[:, :ff].to(F64), gu[:, ff:].to(F64)
    _, silu, _ = sigmoid_parts(g64)
    ds = RHO_S * silu.abs()
    check_interval(h.view, bf(bf(silu - ds).to(F64) * u64), bf(bf(silu + ds).to(F64) * u64), "swiglu_fwd", what)
    h.check(what)
    ro.check(what)


@pytest.mark.parametrize("sweep", [False, True], ids=["normal", "sweep"])
@pytest.mark.parametrize("M,ff", [(1, 8), (1, 1408), (123, 8), (123, 1408), (600, 7040)], ids=lambda v: str(v))
def test_bounded_swiglu_bwd(M, ff, sweep):
    """dgu[:, ff:] = bf16(dh * bf16(g sg)), dgu[:, :ff] = bf16(bf16(dh u) * silu'(g)), intervals as derived in the module docstring"""
    gu, dh = swiglu_inputs(M, ff, 1, sweep)
    dgu = Guarded(M, 2 * ff)
    ro = ReadOnly(gu=gu, dh=dh)
    what = f"swiglu_bwd M={M} ff={ff} {'sweep' if sweep else 'normal'}"
    run(L().nv_swiglu_bwd_bf16(gu.data_ptr(), dh.data_ptr(), dgu.view.data_ptr(), M, ff, st()), what)
    g64, u64, d64 = gu[:, :ff].to(F64), gu[:, ff:].to(F64), dh.to(F64)
    sg, _, _ = sigmoid_parts(g64)
    dsg = RHO_S * sg + TINY
    q = g64 * sg
    dq = SECOND * (g64.abs() * dsg + E * q.abs())
    check_interval(dgu.view[:, ff:], bf(d64 * bf(q - dq).to(F64)), bf(d64 * bf(q + dq).to(F64)), "swiglu_bwd du", what)
    a = 1.0 - sg
    da = dsg + E * a.abs()
    b = g64 * a
    db = g64.abs() * da + E * b.abs()
    t = 1.0 + b
    dt = db + E * t.abs()
    sp = sg * t
    dsp = SECOND * (sg * dt + t.abs() * dsg + E * sp.abs())
    P = bf(d64 * u64).to(F64)
    wv = P * sp
    dw = P.abs() * dsp + E * (wv.abs() + P.abs() * dsp)
    check_interval(dgu.view[:, :ff], bf(wv - dw), bf(wv + dw), "swiglu_bwd dg", what)
    dgu.check(what)
    ro.check(what)
