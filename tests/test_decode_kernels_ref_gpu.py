"""GPU: the decode-step kernels -- csrc/gemv_stream.hip, csrc/gemv_bf16.hip, the GEMV, quantiser and de-quantiser of csrc/fp8w.hip
and nv_rope_scatter_rows_bf16 -- against references that share no code with them (tests/decode_ref.py, checked on the CPU by
test_decode_ref_cpu.py).

EXACT cases.  Operands are small integers on a dyadic grid, so that every fp32 partial sum is exact whatever the wave split, and the
result is fixed bit for bit by integer arithmetic and refkit.bf_round_int:  bf16(sum)  or  bf16(R + bf16(sum)).
    bf16 weights : |x| <= 4, |W| <= 4, |R| <= 64                                          (16 K < 2^24)
    fp8, 2^e     : codes of the integers |q| <= 15, per-row scales 2^-3 .. 2^3, |x| <= 2   (grid 2^-3: sum <= 2 * 960 K)
    fp8, k/128   : s = k / 128 with k in 128 .. 255: s q has up to 12 significant bits, the operand bf16(s q) = bf_round_int(k q) / 128
                   really rounds; |x| <= 2, K <= 2048 (grid 2^-7: sum <= 2 * 3840 K).  Separates bf16(s q) from any other placement
                   of the scale.
    RMSNorm      : rows of +-2^a with a different a per row and eps = 0: bf16(x rstd) = +-1 for any rsqrtf within 2^-9, the operand is
                   sign(x) * norm_w exactly (|norm_w| <= 4) -- a rstd from another row moves a row by a power of two.
    SwiGLU       : the same operands: gate and up are exact integers; h = bf16(bf16(silu(g)) u) lies between that chain at
                   silu (1 - REL_MATH) and at silu (1 + REL_MATH) (refkit.check_interval).  At most 2 % of the elements may have an
                   interval that is not a point (asserted here and, from the reference alone, on the CPU).
decode_ref.gemv_int asserts sum |x||w| < 2^24 grid units for every case, from the operands.

BOUNDED cases (non-integer data; the bound is derived, never measured).  want = the fp64 product on the (de-quantised) operand,
A = sum |x||w|: the fp32 accumulation of K products through at most K + 8 roundings (K steps, the in-lane parity sum, the 8 wave
partials) is within gamma(K + 8) A; one bf16 rounding of the sum: E1 = gamma(K + 8) A + u (|S| + gamma A).  With R the result is
bf16(R + bf16(S)): E2 = E1 + (u + e) SECOND (|R| + |S| + E1).

Every output is a refkit.Guarded view with a padded leading dimension and one row more than M; x, W, R live in buffers with padded
leading dimensions whose pad columns hold NaN (a read of them shows in the result) and are compared bit for bit afterwards.

Which gemv_stream_kernel<FP8, WIDE, UMAX, MODE> a shape reaches depends on the device's CU count: the cases are generated from it
(decode_ref.stream_cases) and test_stream_cases_reach_every_instantiation asserts, with the mirror of dispatch(), that they reach all
42 instantiations and every block / wave / stage edge on the device the suite runs on."""
import pytest
import torch

import decode_ref as D
from refkit import (BF, F32, F64, I32, I64, E, U, SECOND, NV_ERR_ARG, NV_ERR_SHAPE, Guarded, ReadOnly, bf, gamma, gen, randn, dev,
                    bits_equal, check_bound, check_interval, bf_round_int)
from test_rowops_ref_gpu import rope_tables, rope_reference, positions, row_mask, L, st, run

pytestmark = pytest.mark.gpu

CUS = torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256
STREAM_CASES = D.stream_cases(CUS)


# ================================================================================================ operands and launch
def padded(t, ld):
    """t [rows, width] -> (buffer [rows, ld] whose pad columns hold NaN (bf16) / the NaN code 0x7f (e4m3fn), its view [rows, width])"""
    rows, width = t.shape
    buf = torch.empty(rows, ld, dtype=t.dtype, device=dev())
    if t.dtype == torch.uint8:
        buf.fill_(0x7f)
    else:
        buf.view(torch.int16).fill_(0x7FC0)
    buf[:, :width] = t.to(dev())
    assert buf.data_ptr() % 16 == 0
    return buf, buf[:, :width]


def weights(g, N, K, kind, e_max=3):
    """-> (device weight [N, K] bf16 or uint8 codes, device scales or None, w in grid units (CPU int64), grid bits)"""
    if kind == "bf16":
        w = D.rand_ints(g, -4, 4, N, K)
        return w.to(BF), None, w, 0
    lim = 3 if kind == "fp8one" else 15
    q = D.rand_ints(g, -lim, lim, N, K)
    codes = D.e4m3_codes_of_ints(q)
    if kind == "fp8one":
        return codes, torch.ones(N, dtype=F32), q, 0
    if kind == "fp8pow2":
        e = D.rand_ints(g, -e_max, e_max, N)
        return codes, (2.0 ** e.to(F64)).to(F32), q * (2 ** (e + e_max))[:, None], e_max
    assert kind == "fp8k128"
    k = D.rand_ints(g, 128, 255, N)
    return codes, (k.to(F64) / 128).to(F32), bf_round_int(k[:, None] * q)[0], 7


def launch(entry, A, lda, a_rows, W, ldw, S, out, R, ldr, M, N, K, mode=0, norm_w=None, expect=0, what=""):
    p = lambda t: None if t is None else t.data_ptr()
    if entry == "pre":
        rc = L().nv_gemv_pre(p(A), p(a_rows), p(W), p(S), out.view.data_ptr(), p(R), M, N, K, lda, ldw, out.geom[1][0], ldr, int(mode >= 1),
                             p(norm_w), 0.0, int(mode == 2), st())
    elif entry == "gemv_bf16":
        rc = L().nv_gemv_bf16(p(A), p(W), out.view.data_ptr(), p(R), M, N, K, lda, ldw, out.geom[1][0], ldr, 2 if R is not None else 0, st())
    else:
        rc = L().nv_gemv_fp8w(p(A), p(W), p(S), out.view.data_ptr(), p(R), M, N, K, lda, ldw, out.geom[1][0], ldr, 2 if R is not None else 0,
                              st())
    run(rc, f"{entry} {what}", expect)


def exact_case(entry, kind, M, N, K, mode=0, resid=False, gather=False, seed=0, pad=8):
    """one exact case of nv_gemv_bf16 / nv_gemv_fp8w / nv_gemv_pre (modes 0 and 1) -> info of the reference"""
    fp8 = kind != "bf16"
    what = f"{entry} {kind} M={M} N={N} K={K} mode={mode} resid={resid} gather={gather}"
    g = D.cpu_gen(seed, M, N, K, mode, len(kind), int(resid), int(gather))
    rows_a = M + 5 if gather else M
    if mode >= 1:
        x, sign = D.norm_operands(g, M, K, rows=rows_a)
        nw = D.rand_ints(g, -4, 4, K)
        x_i = sign * nw[None]
        norm_w = nw.to(BF).to(dev())
    else:
        x_i = D.rand_ints(g, -2, 2, rows_a, K) if fp8 else D.rand_ints(g, -4, 4, rows_a, K)
        if gather:
            x_i[:, 0] = torch.arange(rows_a) % 5 - 2                    # rows differ whatever the draw
        x, norm_w = x_i.to(BF), None
    a_rows = torch.randperm(rows_a, generator=g)[:M].to(I32) if gather else None
    Wd, S, w_u, gb = weights(g, N, K, kind, e_max=2 if mode >= 1 else 3)
    r_i = D.rand_ints(g, -64, 64, M, N) if resid else None
    sel = x_i[a_rows.long()] if gather else x_i
    v, info = D.gemv_int(sel.to(dev()), w_u.to(dev()), None if r_i is None else (r_i * (1 << gb)).to(dev()))
    want = D.units_to_bf16(v, gb)
    wpad = 16 if fp8 else 8
    Abuf, A = padded(x, K + pad)
    Wbuf, Wv = padded(Wd, K + (wpad if pad else 0))
    Rbuf, Rv = padded(r_i.to(BF), N + pad) if resid else (None, None)
    S = None if S is None else S.to(dev())
    a_rows = None if a_rows is None else a_rows.to(dev())
    out = Guarded(M + 1, N, ld=N + pad)
    ro = ReadOnly(**{k: t for k, t in dict(A=Abuf, W=Wbuf, R=Rbuf, S=S, rows=a_rows, norm_w=norm_w).items() if t is not None})
    launch(entry, A, Abuf.stride(0), a_rows, Wv, Wbuf.stride(0), S, out, Rv, N + pad if resid else 0, M, N, K, mode, norm_w, what=what)
    got = out.view[:M]
    assert bits_equal(got, want), (f"{what}: {int((got != want).sum())} of {want.numel()} elements differ; first at "
                                   f"{(got != want).nonzero()[0].tolist()}")
    out.check(what, (slice(0, M), slice(None)))
    ro.check(what)
    return info


# ================================================================================================ 1. dispatch coverage
def test_stream_cases_reach_every_instantiation():
    """the mirror of dispatch() applied to the cases the next test runs, at THIS device's CU count"""
    got = D.coverage(STREAM_CASES, CUS)
    inst = sorted(f[1:] for f in got if isinstance(f, tuple))
    print(f"REF_COVERAGE {CUS} CUs, {len(STREAM_CASES)} cases reach {len(inst)} instantiations (FP8, WIDE, UMAX, MODE): {inst}")
    print(f"REF_COVERAGE edges: {sorted(f for f in got if isinstance(f, str))}")
    missing = D.REQUIRED - got
    assert not missing, f"not reached at {CUS} CUs: {sorted(map(str, missing))}"


def swiglu_run(M, N, K, fp8, seed, what, pad=8):
    x, sign, nw, Wi = D.swiglu_case(M, N, K, fp8, seed)
    v, _ = D.gemv_int((sign * nw[None]).to(dev()), Wi.to(dev()))
    gu = D.units_to_bf16(v, 0)
    a, b = D.swiglu_interval(gu[:, :N // 2], gu[:, N // 2:])
    share = (a != b).float().mean().item()
    assert share <= 0.02, f"{what}: {share:.3%} of the elements have a non-point interval"
    Wd = D.e4m3_codes_of_ints(Wi) if fp8 else Wi.to(BF)
    S = torch.ones(N, dtype=F32, device=dev()) if fp8 else None
    Abuf, A = padded(x, K + pad)
    Wbuf, Wv = padded(Wd, K + (16 if fp8 else 8))
    norm_w = nw.to(BF).to(dev())
    out = Guarded(M + 1, N // 2, ld=N // 2 + pad)
    ro = ReadOnly(**{k: t for k, t in dict(A=Abuf, W=Wbuf, S=S, norm_w=norm_w).items() if t is not None})
    launch("pre", A, Abuf.stride(0), None, Wv, Wbuf.stride(0), S, out, None, 0, M, N, K, 2, norm_w, what=what)
    check_interval(out.view[:M], a, b, "gemv_pre swiglu", what)
    out.check(what, (slice(0, M), slice(None)))                          # the write set is [M, N/2] only
    ro.check(what)


@pytest.mark.parametrize("fp8,M,N,K,mode", STREAM_CASES, ids=lambda v: str(int(v)))
def test_exact_stream_dispatch_case(fp8, M, N, K, mode):
    """nv_gemv_pre on a shape generated from the CU count (see the coverage test): modes 0 (with R), 1 and 2"""
    if mode == 2:
        swiglu_run(M, N, K, fp8, 11, f"stream case fp8={fp8} M={M} N={N} K={K} swiglu")
    else:
        exact_case("pre", "fp8pow2" if fp8 else "bf16", M, N, K, mode=mode, resid=mode == 0, seed=12)


# ================================================================================================ 2. plain streamer and generic GEMV
PLAIN = [("gemv_bf16", "bf16"), ("pre", "bf16"), ("gemv_fp8w", "fp8pow2"), ("pre", "fp8pow2"), ("gemv_fp8w", "fp8k128"), ("pre", "fp8k128")]


@pytest.mark.parametrize("resid", [False, True], ids=["store", "resid"])
@pytest.mark.parametrize("M", [1, 7, 8, 9, 16])
@pytest.mark.parametrize("entry,kind", PLAIN, ids=[f"{e}-{k}" for e, k in PLAIN])
def test_exact_plain_gemv(entry, kind, M, resid):
    """37 units (uneven over the blocks), 9 K steps of the streamer (bf16 K = 576; fp8 K = 1152) over 8 waves"""
    info = exact_case(entry, kind, M, 8 * 37, 1152 if kind != "bf16" else 576, resid=resid, seed=21)
    assert info["big"] > 0, "no sum above 256: the case does not exercise the bf16 rounding"


def test_exact_fp8_scaled_operand_longest_k():
    """s = k/128 at K = 2048, the largest K at which the sums stay exact on the 2^-7 grid; must contain rounding ties"""
    info = exact_case("gemv_fp8w", "fp8k128", 16, 8 * 21, 2048, resid=True, seed=22)
    assert info["big"] > 0


@pytest.mark.parametrize("resid", [False, True], ids=["store", "resid"])
@pytest.mark.parametrize("N", [1, 15, 17, 100])
@pytest.mark.parametrize("entry,kind,K", [("gemv_bf16", "bf16", 32), ("gemv_bf16", "bf16", 96), ("gemv_fp8w", "fp8pow2", 64),
                                          ("gemv_fp8w", "fp8k128", 192)])
def test_exact_generic_fallback(entry, kind, K, N, resid):
    """shapes the streamer refuses (K % 64 / K % 128, N % 8, N < 16): gemv_bf16_kernel / gemv_fp8w_kernel <RESID, NTILE = 1> with a
    ragged last column tile, waves without steps (K / 32 or K / 64 steps < 8 waves) and the one-step tail loop"""
    assert D.stream_plan(5, N, K, kind != "bf16", 0, CUS) is None
    for M in (5, 16):
        exact_case(entry, kind, M, N, K, resid=resid, seed=23)


@pytest.mark.parametrize("resid", [False, True], ids=["store", "resid"])
@pytest.mark.parametrize("entry,kind,N,K", [("gemv_bf16", "bf16", 5121, 5120), ("gemv_fp8w", "fp8pow2", 5129, 192)])
def test_exact_generic_two_tiles_per_block(entry, kind, N, K, resid):
    """NTILE = 2 (bf16: K >= 5120 and N >= 5120; fp8: N >= 5120) on a shape the streamer refuses, last tile ragged (N % 32 = 1 / 9).
    NTILE = 4 is reachable only through the NV_GEMV_NTILE measurement knob, which is read once per process: not covered here."""
    assert D.stream_plan(9, N, K, kind != "bf16", 0, CUS) is None
    exact_case(entry, kind, 9, N, K, resid=resid, seed=24)


def test_refusals_leave_the_output_untouched():
    """M = 17, a base that is not 16-byte aligned and a leading dimension of W that breaks the row alignment: NV_ERR_SHAPE from
    nv_gemv_bf16, nv_gemv_fp8w and nv_gemv_pre; RMSNorm with K = 8256 > 8192 and SwiGLU with N = 8 (mod 16): NV_ERR_SHAPE; SwiGLU
    without RMSNorm or with a residual: NV_ERR_ARG.  Nothing is written."""
    g = D.cpu_gen(31)
    N, K = 64, 256
    x = D.rand_ints(g, -4, 4, 18, K + 8).to(BF).to(dev())
    Wb, Wq = D.rand_ints(g, -4, 4, N, K + 24).to(BF).to(dev()), D.e4m3_codes_of_ints(D.rand_ints(g, -15, 15, N, K + 24)).to(dev())
    S = torch.ones(N, dtype=F32, device=dev())
    Rt = D.rand_ints(g, -64, 64, 18, N).to(BF).to(dev())
    nw = torch.ones(8256, dtype=BF, device=dev())
    out = Guarded(18, N, ld=N + 8)
    for entry, W, Sx, ldw_bad in (("gemv_bf16", Wb, None, K + 4), ("pre", Wb, None, K + 4), ("gemv_fp8w", Wq, S, K + 8), ("pre", Wq, S, K + 8)):
        ldw = K + 16
        launch(entry, x, K + 8, None, W, ldw, Sx, out, Rt, N, 17, N, K, expect=NV_ERR_SHAPE, what="M = 17")
        launch(entry, x[0, 1:], K + 8, None, W, ldw, Sx, out, Rt, N, 4, N, K, expect=NV_ERR_SHAPE, what="misaligned A")
        launch(entry, x, K + 8, None, W[0, (1 if Sx is None else 8):], ldw, Sx, out, Rt, N, 4, N, K, expect=NV_ERR_SHAPE, what="misaligned W")
        launch(entry, x, K + 8, None, W, ldw_bad, Sx, out, Rt, N, 4, N, K, expect=NV_ERR_SHAPE, what="bad ldw")
        launch(entry, x, K + 4, None, W, ldw, Sx, out, Rt, N, 4, N, K, expect=NV_ERR_SHAPE, what="bad lda")
    big = D.rand_ints(g, -1, 1, 4, 8256).to(BF).to(dev())
    Wl = D.rand_ints(g, -1, 1, 16, 8256).to(BF).to(dev())
    launch("pre", big, 8256, None, Wl, 8256, None, out, None, 0, 4, 16, 8256, mode=1, norm_w=nw, expect=NV_ERR_SHAPE, what="RMSNorm K=8256")
    for n_bad in (24, 40):
        launch("pre", x, K + 8, None, Wb, K + 24, None, out, None, 0, 4, n_bad, K, mode=2, norm_w=nw, expect=NV_ERR_SHAPE, what=f"SwiGLU N={n_bad}")
    rc = L().nv_gemv_pre(x.data_ptr(), None, Wb.data_ptr(), None, out.view.data_ptr(), None, 4, N, K, K + 8, K + 24, N + 8, 0, 0, None, 0.0, 1, st())
    run(rc, "SwiGLU without RMSNorm", NV_ERR_ARG)
    rc = L().nv_gemv_pre(x.data_ptr(), None, Wb.data_ptr(), None, out.view.data_ptr(), Rt.data_ptr(), 4, N, K, K + 8, K + 24, N + 8, N, 1,
                         nw.data_ptr(), 0.0, 1, st())
    run(rc, "SwiGLU with a residual", NV_ERR_ARG)
    out.check("refusals", torch.zeros(18, N, dtype=torch.bool, device=dev()))


RANDOM = [("gemv_bf16", False, 8 * 53, 1024), ("pre", False, 8 * 53, 1024), ("gemv_bf16", False, 100, 96), ("gemv_fp8w", True, 8 * 53, 1024),
          ("pre", True, 8 * 53, 1024), ("gemv_fp8w", True, 100, 192)]


@pytest.mark.parametrize("resid", [False, True], ids=["store", "resid"])
@pytest.mark.parametrize("entry,fp8,N,K", RANDOM, ids=[f"{e}-{'fp8' if f else 'bf16'}-N{n}" for e, f, n, k in RANDOM])
def test_random_data_derived_bound(entry, fp8, N, K, resid):
    """non-integer bf16 x and W (fp8: codes and scales of fp8.quantize_rows, reference on decode_ref's de-quantisation of them) against
    the fp64 product; the bound of the module docstring"""
    from navillm_amd import fp8 as fp8mod
    M = 13
    g = gen(41, N, K, int(fp8), int(resid), len(entry))
    x, W = randn(g, M, K), randn(g, N, K, scale=0.05)
    R = randn(g, M, N) if resid else None
    S = None
    Wop = W
    if fp8:
        q, S = fp8mod.quantize_rows(W)
        Wop = D.dequant_reference(q.cpu(), S.cpu()).to(dev())
        W = q
    Abuf, A = padded(x, K + 8)
    Wbuf, Wv = padded(W, K + 16)
    Rbuf, Rv = padded(R, N + 8) if resid else (None, None)
    out = Guarded(M + 1, N, ld=N + 8)
    what = f"random {entry} fp8={fp8} N={N} K={K} resid={resid}"
    launch(entry, A, K + 8, None, Wv, K + 16, S, out, Rv, N + 8 if resid else 0, M, N, K, what=what)
    S64 = x.to(F64) @ Wop.to(F64).T
    Aabs = x.to(F64).abs() @ Wop.to(F64).abs().T
    ga = gamma(K + 8) * Aabs
    bound = ga + U * (S64.abs() + ga)
    want = S64
    if resid:
        bound = bound + (U + E) * SECOND * (R.to(F64).abs() + S64.abs() + bound)
        want = S64 + R.to(F64)
    check_bound(out.view[:M], want, bound, "gemv random", what)
    out.check(what, (slice(0, M), slice(None)))


# ================================================================================================ 3. folded modes of nv_gemv_pre
@pytest.mark.parametrize("kind", ["bf16", "fp8pow2"])
@pytest.mark.parametrize("M", [1, 8, 13])
def test_exact_row_gather(kind, M):
    """a_rows: M of M + 5 distinct integer rows under a permutation, with and without R"""
    for resid in (False, True):
        exact_case("pre", kind, M, 8 * 11, 256, resid=resid, gather=True, seed=51)


@pytest.mark.parametrize("kind", ["bf16", "fp8pow2"])
@pytest.mark.parametrize("K", [64, 2048, 2112, 8192])
def test_exact_rmsnorm_prologue(kind, K):
    """1, 2 and 4 of the 2048-element chunks of the row sum (fp8 needs K % 128 = 0: 128 / 2176 in place of 64 / 2112); M = 3, 8 and 16
    (the rows are reduced two at a time by the two half-blocks), plain and gathered rows"""
    if kind != "bf16":
        K = {64: 128, 2112: 2176}.get(K, K)
    for M, gather in ((3, False), (8, True), (16, False), (13, True)):
        exact_case("pre", kind, M, 8 * 5, K, mode=1, gather=gather, seed=52)


@pytest.mark.parametrize("M,N,K,fp8", D.SWIGLU_CASES, ids=lambda v: str(int(v)))
def test_swiglu_epilogue_interval(M, N, K, fp8):
    swiglu_run(M, N, K, fp8, 7, f"swiglu M={M} N={N} K={K} fp8={fp8}")


# ================================================================================================ 4. quantiser and de-quantiser
def quant_rows_2560():
    """K = 2560 = 20 binades x 128 mantissas (a second trip of the 256 x 8 loop)"""
    pat = torch.arange(0x3A00, 0x4400, dtype=torch.int32).to(torch.int16).view(BF)          # every bf16 in [2^-11, 2^9)
    sgn = torch.where(torch.arange(2560) % 3 == 0, -1.0, 1.0).to(BF)
    r0 = torch.where(pat.float() <= 448.0, pat, torch.zeros_like(pat))                        # amax = 448: s = 1, every tie at bit 20,
    #                                                                                           the subnormal grid, 8 -> first normal
    r1 = (r0.to(F64) * 2.0 ** -30).to(BF) * sgn                                                # the same with s = 2^-30
    mags = torch.cat([torch.arange(0x4080 - 128 * b, 0x4100 - 128 * b, dtype=torch.int32) for b in range(18)]).to(torch.int16).view(BF)
    r2 = torch.cat([mags, torch.zeros(256, dtype=BF)]) * sgn                                   # 18 binades below amax = 7.96875
    r3 = torch.zeros(2560, dtype=BF)                                                           # s = 1, all codes 0
    sub = (torch.arange(2560, dtype=torch.int32) % 128).to(torch.int16).view(BF)               # bf16 subnormals, amax = 127 * 2^-133
    r4 = torch.where(torch.arange(2560) % 2 == 0, sub, -sub)
    g = D.cpu_gen(61)
    rnd = (torch.randn(4, 2560, generator=g) * torch.tensor([1e-3, 0.05, 1.0, 300.0])[:, None]).to(BF)
    return torch.stack([r0, r1, r2, r3, r4] + list(rnd))


def quant_check(W, what):
    N, K = W.shape
    want_q, want_s = D.quant_reference(W)                                                       # on the CPU (fp32 subnormals kept)
    Wbuf, Wv = padded(W, K + 8)
    ldq = (K + 16) // 16 * 16                                                                   # keeps the guarded view 16-byte aligned
    Q = Guarded(N, K, dtype=torch.uint8, ld=ldq, fill=0x7f)
    Sg = Guarded(N, 1, dtype=F32)
    ro = ReadOnly(W=Wbuf)
    run(L().nv_fp8_quant_rows(Wv.data_ptr(), Q.view.data_ptr(), Sg.view.data_ptr(), N, K, K + 8, ldq, st()), what)
    got_q, got_s = Q.view.cpu(), Sg.view.cpu().flatten()
    assert bits_equal(got_s, want_s), f"{what}: scales differ in rows {(got_s != want_s).nonzero().flatten().tolist()}: {got_s} vs {want_s}"
    bad = (got_q != want_q)
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} codes differ, per row {bad.sum(1).tolist()}; first at {bad.nonzero()[0].tolist()}: "
                                 f"got {int(got_q[bad][0]):#x} want {int(want_q[bad][0]):#x}")
    Q.check(what)
    Sg.check(what, (slice(None), slice(None)))
    ro.check(what)
    return want_q, want_s


def test_quantiser_every_magnitude_class_ties_subnormals_saturation():
    W = quant_rows_2560()
    q, s = quant_check(W, "nv_fp8_quant_rows K=2560")
    assert float(s[0]) == 1.0 and float(s[1]) == 2.0 ** -30 and float(s[3]) == 1.0 and 0 < float(s[4]) < 2.0 ** -126
    mag = q & 0x7f
    assert int(mag[3].max()) == 0 and int(q[3].max()) == 0                                      # the all-zero row: code 0, no sign
    assert int(mag.max()) == 0x7e and not bool((mag == 0x7f).any())                             # saturation, never the NaN code
    assert set(range(1, 9)) <= set(mag[0].tolist()) and set(range(0x7f)) <= set(mag[:3].flatten().tolist())
    y0 = W[0].to(F64).abs()                                                                     # s = 1: the fp32 quotient is w itself
    grid = torch.tensor(D.E4M3_POS, dtype=F64)
    mid = (grid[:-1] + grid[1:]) / 2
    assert int(torch.isin(y0, mid).sum()) >= 100, "row 0 holds too few exact ties"
    assert int(mag[4].max()) == 0x7e and bool((mag[4][(torch.arange(2560) % 128) == 0] == 0).all())   # subnormal amax: finite codes


def test_quantiser_smallest_row():
    g = D.cpu_gen(62)
    W = (torch.randn(3, 8, generator=g) * 2).to(BF)
    W[1] = 0
    quant_check(W, "nv_fp8_quant_rows K=8")


def test_dequantiser_all_codes_times_eight_bit_scales():
    """bf16(s q) for the 256 codes x s = k/128, k = 128 .. 255 (the product has up to 12 significant bits: the bf16 rounding is real),
    padded ldq and ldo"""
    codes = torch.arange(256, dtype=torch.int32).to(torch.uint8)[None].repeat(128, 1)
    s = (torch.arange(128, 256, dtype=F64) / 128).to(F32)
    want = D.dequant_reference(codes, s)
    Qbuf, Qv = padded(codes, 256 + 16)
    out = Guarded(128, 256, ld=256 + 8)
    sd = s.to(dev())
    ro = ReadOnly(Q=Qbuf, s=sd)
    run(L().nv_fp8_dequant_rows(Qv.data_ptr(), sd.data_ptr(), out.view.data_ptr(), 128, 256, 256 + 16, 256 + 8, st()), "nv_fp8_dequant_rows")
    got = out.view.cpu()
    nan = torch.isnan(want)
    assert int(nan.sum()) == 256 and torch.equal(torch.isnan(got), nan)
    assert bits_equal(torch.where(nan, torch.zeros_like(got), got), torch.where(nan, torch.zeros_like(want), want))
    assert int((want.to(F64) != s.to(F64)[:, None] * torch.tensor(D.E4M3, dtype=F64)[None])[~nan].sum()) > 5000      # it really rounds
    out.check("nv_fp8_dequant_rows", (slice(None), slice(None)))
    ro.check("nv_fp8_dequant_rows")


# ================================================================================================ 5. rope-scatter
@pytest.mark.parametrize("M", [1, 11, 16])
@pytest.mark.parametrize("hd", [16, 64, 128])
def test_exact_rope_scatter_decode_rows(hd, M):
    """dst[rows[m]] = [rope(q) | rope(k) | v]: q|k = float64 -> float32 -> bfloat16 of the rotation, v copied bit for bit, the other rows
    of a destination with M + 9 rows untouched.  (The entry point requires ld == 3 H hd -- a padded ld is NV_ERR_ARG, asserted by
    test_rowops_ref_gpu.py::test_rope_refusals -- so the padding here is the guard around the destination.)"""
    H = 3
    g = gen(71, hd, M)
    cos_t, sin_t = rope_tables(g, hd, "indep")
    W, R = 3 * H * hd, M + 9
    src = randn(g, M, W)
    pos = positions(g, M)
    rows = torch.randperm(R, generator=D.cpu_gen(72, hd, M))[:M].to(I32).to(dev())
    dst = Guarded(R, W)
    ro = ReadOnly(src=src, cos=cos_t, sin=sin_t, pos=pos, rows=rows)
    what = f"rope_scatter hd={hd} M={M}"
    run(L().nv_rope_scatter_rows_bf16(src.data_ptr(), cos_t.data_ptr(), sin_t.data_ptr(), pos.data_ptr(), rows.data_ptr(), dst.view.data_ptr(),
                                      M, H, hd, W, st()), what)
    want = rope_reference(src, cos_t, sin_t, pos, H, hd, 1.0)
    got = dst.view[rows.long()]
    assert bits_equal(got[:, 2 * H * hd:], src[:, 2 * H * hd:]), f"{what}: the v columns are not a bit copy"
    assert bits_equal(got[:, :2 * H * hd], want[:, :2 * H * hd]), f"{what}: q|k differ from the fp64 rotation"
    assert not bits_equal(want[:, :2 * H * hd], src[:, :2 * H * hd]) or M == 1
    dst.check(what, row_mask(R, W, rows))
    ro.check(what)
