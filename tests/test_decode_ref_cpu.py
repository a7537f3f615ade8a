"""CPU: the pure-Python parts of the decode-kernel reference tests (tests/decode_ref.py) -- the mirror of the weight streamer's
dispatch at three CU counts, the exact-integer GEMV reference against fp64, refkit.bf_round_int against float64 -> float32 ->
bfloat16, the e4m3fn table and encoder against torch.float8_e4m3fn, and the share of SwiGLU elements whose interval is not a
point."""
import pytest
import torch

import decode_ref as D
from refkit import BF, F32, F64, I64, bf, bf_round_int


@pytest.mark.parametrize("cus", [64, 256, 304])
def test_generated_cases_reach_every_instantiation_and_edge(cus):
    cases = D.stream_cases(cus)
    got = D.coverage(cases, cus)
    assert not (D.REQUIRED - got), f"not reached at {cus} CUs: {sorted(map(str, D.REQUIRED - got))}"
    assert len(D.instantiations()) == 42
    assert max(N * K * (1 if fp8 else 2) for fp8, M, N, K, mode in cases) <= 8 << 20          # the largest weight: a few MiB


@pytest.mark.parametrize("cus", [64, 256, 304])
def test_dispatch_mirror_hand_checked_plans(cus):
    """plans worked out by hand from dispatch(): grid = min(items, cus), umax = ceil(items / grid), capped at 16 (8 when M > 8)"""
    p = D.stream_plan(8, 8 * (cus + 3), 64, False, 0, cus)
    assert (p["wide"], p["umax"], p["grid"], p["sg"]) == (False, 2, cus, 4) and sorted(set(p["nu"])) == [1, 2] and p["nu"].count(2) == 3
    assert p["nsteps"] == [1, 0, 0, 0, 0, 0, 0, 0]
    p = D.stream_plan(9, 8 * (8 * cus + 1), 128, True, 0, cus)
    assert (p["wide"], p["umax"], p["enlarged"], p["grid"]) == (True, 8, True, cus + 1) and min(p["nu"]) < 8
    p = D.stream_plan(8, 8 * (8 * cus + 1), 64, False, 0, cus)
    assert (p["umax"], p["enlarged"], p["grid"], max(p["nu"])) == (16, False, cus, 9)
    p = D.stream_plan(16, 16 * (4 * cus + 1), 64, False, 2, cus)                               # pairs: 4 items = 8 units per block
    assert (p["umax"], p["enlarged"], p["grid"]) == (8, True, cus + 1) and set(p["nu"]) <= {6, 8}
    p = D.stream_plan(1, 16, 64 * 17, False, 0, cus)                                            # 17 steps over 8 waves: 3,3,3,3,3,2,0,0
    assert p["nsteps"] == [3, 3, 3, 3, 3, 2, 0, 0] and p["grid"] == 2 and p["nu"] == [1, 1]
    p = D.stream_plan(1, 16, 128 * 40, True, 1, cus)
    assert p["nsteps"] == [5] * 8
    for bad in ((17, 64, 64, False, 0), (0, 64, 64, False, 0), (4, 60, 64, False, 0), (4, 64, 96, False, 0), (4, 64, 192, True, 0),
                (4, 24, 64, False, 2), (4, 64, 8256, False, 1), (4, 4, 64, False, 0)):
        assert D.stream_plan(*bad, cus) is None, bad
    assert D.stream_plan(4, 64, 8256 - 64, False, 1, cus) is not None and D.stream_plan(4, 64, 8256 + 56, False, 0, cus) is None
    assert D.stream_plan(4, 64, 8320, False, 0, cus) is not None                                # K > 8192 is fine without RMSNorm


def test_bf_round_int_composes_like_float64_float32_bfloat16():
    g = torch.Generator().manual_seed(5)
    v = torch.cat([torch.arange(-70000, 70000), torch.randint(-(1 << 24) + 1, 1 << 24, (200000,), generator=g),
                   torch.tensor([255, 256, 257, 258, 259, 385, 383, (1 << 24) - 1, 3825, 3832, 3848])]).to(I64)
    r, tie, big = bf_round_int(v)
    assert torch.equal(r.to(F64), bf(v.to(F64)).to(F64))
    assert int(tie.sum()) > 0 and bool(tie[v == 257].all()) and not bool(tie[v == 258].any())
    # two roundings in a row, as the residual epilogue does them, on a 2^-7 grid: bf16(R + bf16(S))
    s, rr = v[:100000], (torch.randint(-64, 65, (100000,), generator=g) << 7).to(I64)
    inner = bf_round_int(s)[0]
    outer = bf_round_int(rr + inner)[0]
    want = bf(rr.to(F64) / 128 + bf(s.to(F64) / 128).to(F64)).to(F64) * 128
    assert torch.equal(outer.to(F64), want)


def test_integer_gemv_reference_equals_fp64_and_sees_a_missing_rounding():
    g = D.cpu_gen(3)
    x, w = D.rand_ints(g, -4, 4, 9, 1024), D.rand_ints(g, -4, 4, 40, 1024)
    r = D.rand_ints(g, -64, 64, 9, 40)
    v, info = D.gemv_int(x, w)
    acc = x.to(F64) @ w.to(F64).T
    assert torch.equal(D.units_to_bf16(v, 0), bf(acc))
    v2, info2 = D.gemv_int(x, w, r)
    assert torch.equal(D.units_to_bf16(v2, 0), bf(r.to(F64) + bf(acc).to(F64)))
    single = bf(r.to(F64) + acc)                                   # what dropping the inner rounding would give
    assert int((single != D.units_to_bf16(v2, 0)).sum()) > 0, "the case cannot tell bf16(R + bf16(S)) from bf16(R + S)"
    assert info["big"] > 0
    with pytest.raises(AssertionError):
        D.gemv_int(x * (1 << 14), w)


def test_scaled_fp8_operand_rounds_and_separates_the_scale_placements():
    """s = k/128, k in 128..255, integer codes |q| <= 15: bf16(s q) = bf_round_int(k q) / 128 really rounds, and a GEMV with the scale
    applied to the accumulator instead differs from the documented one"""
    k = torch.arange(128, 256, dtype=I64)[:, None]
    q = torch.arange(-15, 16, dtype=I64)[None]
    op, tie, big = bf_round_int(k * q)
    assert torch.equal(op.to(F64) / 128, bf(k.to(F64) / 128 * q.to(F64)).to(F64))
    assert int((op != k * q).sum()) > 1000 and int(op.abs().max()) <= 3840
    g = D.cpu_gen(4)
    ks, qs = D.rand_ints(g, 128, 255, 24), D.rand_ints(g, -15, 15, 24, 2048)
    x = D.rand_ints(g, -2, 2, 5, 2048)
    w_u = bf_round_int(ks[:, None] * qs)[0]
    v, _ = D.gemv_int(x, w_u)
    other = bf((x.to(F64) @ qs.to(F64).T) * (ks.to(F64) / 128)[None])
    assert int((other != D.units_to_bf16(v, 7)).sum()) > 0


def test_e4m3_table_and_encoder_against_torch_float8():
    codes = torch.arange(256, dtype=torch.uint8)
    want = codes.view(torch.float8_e4m3fn).to(F32)
    mine = torch.tensor(D.E4M3, dtype=F32)
    assert torch.equal(torch.isnan(mine), torch.isnan(want)) and int(torch.isnan(mine).sum()) == 2
    ok = ~torch.isnan(want)
    assert torch.equal(mine[ok], want[ok]) and torch.equal(torch.signbit(mine[ok]), torch.signbit(want[ok]))
    assert D.E4M3[0x7e] == 448.0 and D.E4M3[0x08] == 2.0 ** -6 and D.E4M3[0x07] == 7 * 2.0 ** -9
    g = torch.Generator().manual_seed(9)
    y = torch.cat([torch.randn(100000, generator=g) * 100, torch.randn(100000, generator=g) * 0.02,
                   (torch.tensor(D.E4M3_POS[:-1]) + torch.tensor(D.E4M3_POS[1:])) / 2,             # every tie
                   torch.tensor([448.0, 449.0, 463.9, 0.0, -0.0, 2.0 ** -10, 3 * 2.0 ** -10, 15 * 2.0 ** -10, 15.5 * 2.0 ** -10])]).to(F32)
    y = torch.cat([y, -y]).clamp(-464, 464)
    sat = y.clamp(-448, 448)                                        # torch's conversion does not saturate: clamp for it
    assert torch.equal(D.e4m3_rne(y), sat.to(torch.float8_e4m3fn).view(torch.uint8))
    q = torch.arange(-15, 16)
    assert torch.equal(D.e4m3_codes_of_ints(q), q.to(F32).to(torch.float8_e4m3fn).view(torch.uint8))
    W = (torch.randn(6, 64, generator=g) * 3).to(BF)
    W[1] = 0
    c, s = D.quant_reference(W)
    s_t = torch.where(W.float().abs().amax(1) > 0, W.float().abs().amax(1) / 448.0, torch.ones(6))
    assert torch.equal(s, s_t) and float(s[1]) == 1.0 and int(c[1].max()) == 0
    assert torch.equal(c, (W.float() / s_t[:, None]).to(torch.float8_e4m3fn).view(torch.uint8))
    assert torch.equal(D.dequant_reference(c, s), (c.view(torch.float8_e4m3fn).float() * s[:, None]).to(BF))


def test_rmsnorm_operands_are_an_integer_problem():
    """x = +-2^a: the mean square is 4^a exactly (a sum of K equal powers of two is exact in fp32 at every K used, and the quotient by
    K is exact), and bf16(x * rstd) = +-1 for every rstd within 2^-9 of 2^-a"""
    for K in (64, 2048, 2112, 8192):
        x, sign = D.norm_operands(D.cpu_gen(K), 16, K)
        ms = (x.to(F32) ** 2).sum(1) / K
        a = torch.log2(x[:, 0].abs().to(F64))
        assert torch.equal(ms.to(F64), 4.0 ** a) and len(set(a.tolist())) == 16
        for rel in (1 - 2.0 ** -9, 1 + 2.0 ** -9):
            rstd = (2.0 ** -a * rel).to(F32)
            assert torch.equal((x.to(F32) * rstd[:, None]).to(BF).to(F64), sign.to(F64))


def test_swiglu_interval_share_is_below_two_percent():
    """which bf16 integers g have bf16(silu(g) (1 -+ REL_MATH)) on two sides of a rounding boundary: the interval of h is a point
    for every other gate value whatever `up` is.  At most 2 % of the elements of the cases used on the GPU may have one."""
    g_all = bf(torch.arange(-40000, 40001, dtype=F64)).unique()
    lo, hi = D.swiglu_interval(g_all, torch.ones_like(g_all))
    flippy = g_all[lo != hi].to(F64)
    print(f"bf16 integers in +-40000 whose silu may round either way: {flippy.tolist()}")
    assert flippy.numel() <= 0.02 * g_all.numel()
    worst = 0.0
    for M, N, K, fp8 in D.SWIGLU_CASES:
        x, sign, nw, W = D.swiglu_case(M, N, K, fp8, 7)
        v, _ = D.gemv_int(sign * nw[None], W)
        gu = D.units_to_bf16(v, 0)
        a, b = D.swiglu_interval(gu[:, :N // 2], gu[:, N // 2:])
        share = (a != b).float().mean().item()
        worst = max(worst, share)
        assert share <= 0.02, (M, N, K, fp8, share)
    print(f"largest share of non-point SwiGLU intervals over the cases: {worst:.4%}")
