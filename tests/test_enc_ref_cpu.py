"""CPU: the pure-Python parts of the reference tests of the fp32 encoder kernels (tests/enc_ref.py) -- the mirror of the dispatch of
nv_gemm_f32_ws and what GEMM_CASES reaches through it, the fp64 references against torch's own float64 operators and autograd, and
the Philox keep masks against known words."""
import math

import numpy as np
import pytest
import torch

import enc_ref as R

F64 = torch.float64


# ================================================================================================ GEMM dispatch mirror
def test_gemm_cases_reach_every_required_path():
    got = R.gemm_coverage(R.GEMM_CASES)
    missing = R.GEMM_REQUIRED - got
    assert not missing, f"GEMM_CASES does not reach: {sorted(missing)}"
    # named one by one, so that an edit of GEMM_REQUIRED cannot drop them silently
    for need in ("vec(1, 1)", "vec(1, 0)", "vec(0, 0)", "generic(1, 1)", "generic(1, 0)", "generic(0, 0)",
                 "generic(1, 1) misaligned base", "generic(1, 0) misaligned base", "generic(0, 0) misaligned base",
                 "generic(1, 1) ld%4", "generic(1, 0) ld%4", "generic(0, 0) ld%4",
                 "generic(1, 1) extent%4", "generic(1, 0) extent%4", "generic(0, 0) extent%4",
                 "vec(1, 1) split", "vec(1, 0) split", "vec(0, 0) split", "vec(1, 1) no split", "vec(1, 0) no split", "vec(0, 0) no split",
                 "vec(1, 1) split padded ld", "vec(1, 0) split padded ld", "vec(0, 0) split padded ld",
                 "ksplit<S", "partial last K tile inside a split", "blocks>=512", "null workspace on a split-able shape"):
        assert need in got, need


def test_gemm_cases_stay_small_exact_and_inside_the_workspace():
    for c in R.GEMM_CASES:
        p = R.gemm_case_plan(c)
        assert p["ws_floats"] <= 8 * c.M * c.N, c.name
        assert p["ksplit"] <= 8 and (p["ksplit"] == 1 or p["kchunk"] % R.FBK == 0), c.name
        assert c.K <= 1056 and 64 * c.K + 2048 < R.EXACT_LIMIT, c.name
        assert c.M * c.N <= 65536 or c.name == "L0-blocks512-1x32768x256", c.name
    for name in R.GEMM_BOUNDED:
        assert R.GEMM_BY_NAME[name].expect == 0
    kinds = {(R.gemm_case_plan(R.GEMM_BY_NAME[n])["kernel"], R.GEMM_BY_NAME[n].layout, R.gemm_case_plan(R.GEMM_BY_NAME[n])["ksplit"] > 1)
             for n in R.GEMM_BOUNDED}
    assert kinds == {("vec", L, s) for L in (0, 1, 2) for s in (False, True)} | {("generic", L, False) for L in (0, 1, 2)}


def test_gemm_plan_hand_checked():
    """plans worked out by hand from nv_gemm_f32_ws"""
    P = R.gemm_f32_plan
    p = P(0, 36, 64, 228, 228, 228, 0, 0, True)            # 1 block, 8 K tiles: S = min(1024, 8, 8 // 4) = 2, 4 tiles per slice
    assert (p["kernel"], p["S"], p["kchunk"], p["ksplit"], p["ws_floats"]) == ("vec", 2, 128, 2, 2 * 36 * 64)
    assert (p["a_bytes"], p["b_bytes"]) == ((35 * 228 + 228) * 4, (63 * 228 + 228) * 4)
    p = P(0, 36, 64, 228, 228, 228, 0, 0, False)
    assert (p["kernel"], p["ksplit"], p["kchunk"], p["ws_floats"]) == ("vec", 1, 228, 0)
    p = P(1, 64, 64, 256, 256, 64, 0, 0, True)
    assert (p["S"], p["kchunk"], p["ksplit"]) == (2, 128, 2)
    p = P(2, 20, 68, 1024, 24, 68, 0, 0, True)             # 2 blocks, 32 tiles: S = min(512, 8, 8) = 8
    assert (p["blocks"], p["S"], p["kchunk"], p["ksplit"]) == (2, 8, 128, 8)
    assert (p["a_bytes"], p["b_bytes"]) == ((1023 * 24 + 20) * 4, (1023 * 68 + 68) * 4)
    p = P(0, 12, 64, 1056, 1056, 1060, 0, 0, True)         # 33 tiles: S = 8, 5 tiles per slice, 7 slices cover 1056
    assert (p["S"], p["kchunk"], p["ksplit"], p["ws_floats"]) == (8, 160, 7, 7 * 12 * 64)
    p = P(0, 1, 32768, 256, 256, 256, 0, 0, True)          # 512 blocks: not below 512
    assert (p["blocks"], p["S"], p["ksplit"]) == (512, 0, 1)
    p = P(0, 288, 1024, 1024, 1024, 1024, 0, 0, True)      # the encoder's own shape: 80 blocks, S = min(13, 8, 8)
    assert (p["blocks"], p["S"], p["kchunk"], p["ksplit"]) == (80, 8, 128, 8)
    p = P(0, 64, 64, 224, 224, 224, 0, 0, True)            # 7 tiles: below the threshold of 8
    assert (p["S"], p["ksplit"]) == (0, 1)
    p = P(0, 64, 64, 352, 352, 352, 0, 0, True)            # 11 tiles: S = 2, 6 tiles per slice
    assert (p["S"], p["kchunk"], p["ksplit"]) == (2, 192, 2)
    for args in ((0, 36, 64, 38, 38, 38, 0, 0, True), (0, 36, 64, 36, 37, 36, 0, 0, True), (0, 36, 64, 36, 36, 38, 0, 0, True),
                 (0, 36, 64, 36, 36, 36, 4, 0, True), (0, 36, 64, 36, 36, 36, 0, 12, True), (1, 36, 130, 8, 8, 132, 0, 0, True),
                 (2, 65, 132, 8, 68, 132, 0, 0, True), (2, 68, 130, 8, 68, 132, 0, 0, True)):
        assert P(*args)["kernel"] == "generic", args
    assert P(1, 36, 64, 8, 8, 64, 0, 0, True)["kernel"] == "vec" and P(2, 68, 132, 7, 68, 132, 0, 0, True)["kernel"] == "vec"
    assert P(3, 8, 8, 8, 8, 8, 0, 0, True)["kernel"] == "refused" and P(0, -1, 8, 8, 8, 8, 0, 0, True)["kernel"] == "refused"
    assert P(0, 0, 8, 8, 8, 8, 0, 0, True)["kernel"] == "none" and P(2, 8, 0, 8, 8, 8, 0, 0, True)["kernel"] == "none"
    p = P(2, 8, 12, 0, 12, 16, 0, 0, True)                 # K = 0: zero-byte windows, no split
    assert (p["kernel"], p["a_bytes"], p["b_bytes"], p["ksplit"]) == ("vec", 0, 0, 1)


@pytest.mark.parametrize("name", ["L0-vec-65x132x36-ld+4+8", "L1-split-36x64x228", "L2-gen-65x129x33-acc", "L0-k0-8x12-bias-acc"])
def test_gemm_reference_against_float64_loops(name):
    c = R.GEMM_BY_NAME[name]
    A, B, bias, C0 = R.gemm_int_operands(c)
    want, mag = R.gemm_reference(c, A, B, bias, C0)
    a = lambda m, k: A[k, m] if c.layout == 2 else A[m, k]
    b = lambda n, k: B[k, n] if c.layout in (1, 2) else B[n, k]
    g = R.cpu_gen(5)
    for m, n in zip(R.rand_ints(g, 0, c.M - 1, 12).tolist(), R.rand_ints(g, 0, c.N - 1, 12).tolist()):
        v = sum(int(a(m, k)) * int(b(n, k)) for k in range(c.K)) + (int(bias[n]) if bias is not None else 0) + (int(C0[m, n]) if c.acc else 0)
        assert int(want[m, n]) == v
    assert int(mag.max()) < R.EXACT_LIMIT and want.shape == (c.M, c.N)


# ================================================================================================ fp64 references
@pytest.mark.parametrize("M,d,eps", [(1, 1, 1e-5), (3, 7, 1e-12), (5, 257, 1e-5)])
def test_layernorm_references_against_torch(M, d, eps):
    g = R.cpu_gen(M, d)
    x = torch.randn(M, d, generator=g, dtype=F64).requires_grad_()
    w = torch.randn(d, generator=g, dtype=F64).requires_grad_()
    b = torch.randn(d, generator=g, dtype=F64).requires_grad_()
    dy = torch.randn(M, d, generator=g, dtype=F64)
    y = torch.nn.functional.layer_norm(x, (d,), w, b, eps)
    y.backward(dy)
    yr, mean, rstd = R.layernorm_fwd_ref(x.detach(), w.detach(), b.detach(), eps)
    tol = dict(rtol=1e-9, atol=1e-9)
    assert torch.allclose(yr, y.detach(), **tol)
    assert torch.allclose(mean, x.detach().mean(1), **tol) and torch.allclose(rstd, (x.detach().var(1, unbiased=False) + eps).rsqrt(), **tol)
    dx, gw, gb = R.layernorm_bwd_ref(dy, x.detach(), w.detach(), mean, rstd)
    scale = float(rstd.max())                                   # d = 1: rstd = eps^-1/2 amplifies the cancellation of dx = 0
    assert torch.allclose(dx, x.grad, rtol=1e-8, atol=1e-12 * scale * scale + 1e-9)
    assert torch.allclose(gw, w.grad, **tol) and torch.allclose(gb, b.grad, **tol)


def test_gelu_references_against_torch():
    v = torch.cat([torch.linspace(-6, 6, 241, dtype=F64), torch.tensor([0.0, -0.0, 1e-40, -32.0, 32.0], dtype=F64)]).requires_grad_()
    dy = torch.linspace(-2, 2, v.numel(), dtype=F64)
    y = torch.nn.functional.gelu(v)
    y.backward(dy)
    assert torch.allclose(R.gelu_fwd_ref(v.detach()), y.detach(), rtol=1e-12, atol=1e-300)
    dx, cdf, pdf = R.gelu_bwd_ref(v.detach(), dy)
    assert torch.allclose(dx, v.grad, rtol=1e-10, atol=1e-14)
    assert torch.all((cdf >= 0) & (cdf <= 1) & (pdf >= 0))


@pytest.mark.parametrize("B,N,heads,hd,p", [(2, 5, 2, 4, 0.0), (2, 9, 3, 8, 0.25)])
def test_mha_references_against_autograd(B, N, heads, hd, p):
    g = R.cpu_gen(B, N, heads, hd)
    h = heads * hd
    qkv = torch.randn(B * N, 3 * h, generator=g, dtype=F64).requires_grad_()
    lens = torch.tensor([N, 1, max(1, N // 2)][:B])
    keep = (torch.rand(B, heads, N, N, generator=g) >= p).to(F64)
    dout = torch.randn(B * N, h, generator=g, dtype=F64)
    # an independent graph: per (b, head) slices, explicit exp / sum
    outs = []
    for b in range(B):
        cols = []
        for hh in range(heads):
            q = qkv[b * N:(b + 1) * N, hh * hd:(hh + 1) * hd]
            k = qkv[b * N:(b + 1) * N, h + hh * hd:h + (hh + 1) * hd]
            v = qkv[b * N:(b + 1) * N, 2 * h + hh * hd:2 * h + (hh + 1) * hd]
            L = int(lens[b])
            s = (q @ k[:L].t()) / math.sqrt(hd)
            e = torch.exp(s - s.max(dim=1, keepdim=True).values.detach())
            pr = e / e.sum(dim=1, keepdim=True)
            if p > 0:
                pr = pr * keep[b, hh, :, :L] / (1 - p)
            cols.append(pr @ v[:L])
        outs.append(torch.cat(cols, dim=1))
    out = torch.cat(outs, dim=0)
    out.backward(dout)
    o_ref, P = R.mha_fwd_ref(qkv.detach(), lens, B, N, heads, hd, keep, p)
    assert torch.allclose(o_ref, out.detach(), rtol=1e-11, atol=1e-12)
    assert torch.allclose(P.sum(-1), torch.ones(B, heads, N, dtype=F64), atol=1e-12)
    for b in range(B):
        assert torch.all(P[b, :, :, int(lens[b]):] == 0)
    dq = R.mha_bwd_ref(qkv.detach(), P, dout, B, N, heads, hd, keep, p)
    assert torch.allclose(dq, qkv.grad, rtol=1e-10, atol=1e-12)
    gk = dq.reshape(B, N, 3, h)
    for b in range(B):
        assert torch.all(gk[b, int(lens[b]):, 1:] == 0)             # k and v rows of padded keys get no gradient


# ================================================================================================ Philox
def _philox_scalar(c, k):
    """Philox4x32-10 on Python ints (Salmon et al., SC'11), written out independently of sample_ref's numpy version"""
    c, k = list(c), list(k)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return c


# counter 0 under seed 0 is the first known-answer vector of the Random123 distribution; the second has a non-zero high word
# (counter 2^32 + 5 -> c0 = 5, c1 = 1) and a seed with two different halves, worked out with _philox_scalar
WORDS_ZERO = [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
SEED_B, CTR_B = 0x123456789ABCDEF0, (1 << 32) + 5
WORDS_B = [0x092CECB1, 0xF2A0DD41, 0x8A672FE8, 0x931BED00]


def test_philox_known_words():
    assert _philox_scalar([0, 0, 0, 0], [0, 0]) == WORDS_ZERO
    assert _philox_scalar([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2) == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]      # Random123 KAT
    assert _philox_scalar([5, 1, 0, 0], [0x9ABCDEF0, 0x12345678]) == WORDS_B
    assert [int(w[0]) for w in R.philox_words(0, [0])] == WORDS_ZERO
    assert [int(w[0]) for w in R.philox_words(SEED_B, [CTR_B])] == WORDS_B


def _u(word):
    return np.float32((word >> 8) * 2.0 ** -24)


def test_dropout_keep_word_and_counter_convention():
    # u of the four words of counter 0 / seed 0: 0.3990, 0.8805, 0.7357, 0.6055; of counter B: 0.0358, 0.9478, 0.5406, 0.5746
    uz, ub = [_u(w) for w in WORDS_ZERO], [_u(w) for w in WORDS_B]
    assert [round(float(u), 4) for u in uz] == [0.3990, 0.8805, 0.7357, 0.6055]
    assert [round(float(u), 4) for u in ub] == [0.0358, 0.9478, 0.5406, 0.5746]
    for p in (0.0, 0.1, 0.5, 0.6, 0.75, 0.9):
        k = R.dropout_keep(0, 0, 4, p)
        assert k.tolist() == [bool(u >= np.float32(p)) for u in uz], p
        # group 1 of offset 2^32 + 4 is counter B: the offset's high word reaches c1, elements 4..7 take words 0..3
        k = R.dropout_keep(SEED_B, CTR_B - 1, 7, p)
        assert k.shape == (7,) and k[4:].tolist() == [bool(u >= np.float32(p)) for u in ub[:3]], p
    assert R.dropout_keep(0, 0, 3, 0.5).tolist() == [False, True, True]                 # n % 4 != 0: a cut group
    # keep iff u >= p exactly at the threshold, in fp32
    assert bool(R.dropout_keep(0, 0, 1, float(uz[0]))[0]) and not bool(R.dropout_keep(0, 0, 1, float(np.nextafter(uz[0], np.float32(1))))[0])
    # the offset wraps modulo 2^64
    assert R.dropout_keep(0, (1 << 64) - 1, 8, 0.5)[4:].tolist() == [bool(u >= 0.5) for u in uz]


def test_mha_keep_word_and_counter_convention():
    for p in (0.1, 0.5, 0.95):
        # element e = 2 of offset 2^32 + 3 is counter B: word 0 only
        k = R.mha_keep(SEED_B, CTR_B - 2, 1, 1, 2, p)
        assert k.shape == (1, 1, 2, 2) and bool(k[0, 0, 1, 0]) == bool(_u(WORDS_B[0]) >= np.float32(p))
        k = R.mha_keep(0, 0, 1, 1, 1, p)
        assert bool(k[0, 0, 0, 0]) == bool(_u(WORDS_ZERO[0]) >= np.float32(p))
    # e = ((b heads + hh) N + a) N + c: the flat order of a [B, heads, N, N] array
    B, heads, N = 2, 3, 5
    k = R.mha_keep(7, 11, B, heads, N, 0.5)
    e = ((1 * heads + 2) * N + 3) * N + 4
    w0 = int(R.philox_words(7, [11 + e])[0][0])
    assert bool(k[1, 2, 3, 4]) == bool(_u(w0) >= np.float32(0.5))
    assert 0.3 < k.mean() < 0.7
