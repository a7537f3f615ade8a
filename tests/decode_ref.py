"""Pure-Python / torch pieces of the decode-kernel reference tests (test_decode_ref_cpu.py checks them without a GPU,
test_decode_kernels_ref_gpu.py uses them on the device): a mirror of the weight streamer's host dispatch and per-wave K split
(csrc/gemv_stream.hip), the case generator that is built from the device's CU count, the exact-integer GEMV reference, the e4m3fn
code table with its round-to-nearest-even encoder, and the operands of the RMSNorm / SwiGLU cases.

Exactness.  Operands live on a dyadic grid (integers times 2^-g).  A product of two bf16 values is exact in fp32, and as long as
sum |x| |w| stays below 2^24 grid units every partial sum is an integer below 2^24 units -- exact in fp32 whatever the order, the
wave split or the MFMA's internal tree.  The kernel's result is then fixed by integer arithmetic and refkit.bf_round_int (round to
nearest even at 8 significant bits, which does not depend on the grid's power of two)."""
import math

import torch

from refkit import F32, F64, I64, BF, REL_MATH, bf, bf_round_int

GS_WAVES = 8
STAGE_STEPS = {2: 4, 4: 2, 8: 1, 16: 1}          # SG of GsCfg<UMAX>
EXACT_LIMIT = 1 << 24


# ------------------------------------------------------------------------------------------------ dispatch mirror
def stream_accepts(M, N, K, fp8, mode, lda=None, ldw=None):
    """the shape checks of nv_gemv_pre (alignment of the base pointers aside)"""
    lda = K if lda is None else lda
    ldw = K if ldw is None else ldw
    if mode >= 1 and K > 8192:
        return False
    if M < 1 or M > 16 or N < 8 or (N & 7) or (lda & 7) or (mode == 2 and (N & 15)):
        return False
    if fp8:
        return not ((K & 127) or (ldw & 15))
    return not ((K & 63) or (ldw & 7))


def stream_plan(M, N, K, fp8, mode, cus):
    """mirror of dispatch<FP8, WIDE, MODE>() and of the kernel's block / wave split -> dict, or None where the streamer refuses"""
    if not stream_accepts(M, N, K, fp8, mode):
        return None
    wide = M > 8
    ucap = 8 if wide else 16
    per_item = 2 if mode == 2 else 1
    units = N // 8
    items = units // per_item
    grid = min(items, cus)
    umax = (items + grid - 1) // grid * per_item
    enlarged = umax > ucap
    if enlarged:
        cap_items = ucap // per_item
        grid = (items + cap_items - 1) // cap_items
        umax = ucap
    if umax <= 2:
        U = 2
    elif umax <= 4:
        U = 4
    elif umax <= 8 or wide:
        U = 8
    else:
        U = 16
    nu = [((b + 1) * items // grid - b * items // grid) * per_item for b in range(grid)]
    assert max(nu) <= U and sum(nu) == units
    steps = K // (128 if fp8 else 64)
    per = (steps + GS_WAVES - 1) // GS_WAVES
    nsteps = [max(min(steps, (w + 1) * per) - w * per, 0) for w in range(GS_WAVES)]
    assert sum(nsteps) == steps
    return dict(fp8=bool(fp8), wide=wide, umax=U, mode=mode, grid=grid, nu=nu, nsteps=nsteps, sg=STAGE_STEPS[U], enlarged=enlarged)


def instantiations():
    """every gemv_stream_kernel<FP8, WIDE, UMAX, MODE> the host can select"""
    return {(f, w, u, m) for f in (False, True) for w in (False, True) for u in ((2, 4, 8) if w else (2, 4, 8, 16)) for m in (0, 1, 2)}


def features(plan):
    f = {("inst", plan["fp8"], plan["wide"], plan["umax"], plan["mode"])}
    if min(plan["nu"]) < plan["umax"]:
        f.add("nu<UMAX")
    if min(plan["nu"]) != max(plan["nu"]):
        f.add("uneven nu")
    if 0 in plan["nsteps"]:
        f.add("wave with 0 steps")
    for n in plan["nsteps"]:
        if n and plan["sg"] == 4 and n % 4:
            f.add(f"SG4 tail {n % 4}")
        if n and plan["sg"] == 2 and n % 2:
            f.add("SG2 tail 1")
    if plan["wide"] and plan["enlarged"]:
        f.add("WIDE grid enlarged")
    if not plan["wide"] and plan["enlarged"]:
        f.add("narrow grid enlarged")
    return f


REQUIRED = ({("inst",) + i for i in instantiations()} |
            {"nu<UMAX", "uneven nu", "wave with 0 steps", "SG4 tail 1", "SG4 tail 2", "SG4 tail 3", "SG2 tail 1", "WIDE grid enlarged"})
K_STEPS = (1, 3, 9, 17, 40)


def stream_cases(cus):
    """(fp8, M, N, K, mode) built from the CU count: N = 8 (cus k + r) (mode 2: 16 (cus k + r) for gate|up).  Large N goes with one
    K step; the K-step edges go with small N (UMAX 2 and 4, whose stages hold 4 and 2 steps)."""
    out = []
    for fp8 in (False, True):
        KL = 128 if fp8 else 64
        for M in (7, 16):                                           # narrow (one MFMA per load) and WIDE
            for mode in (0, 1, 2):
                w = 16 if mode == 2 else 8
                # items per block 1..2 / 3..4 / 4..5 of 8 / 8..9 (narrow: UMAX 16; WIDE: grid enlarged), uneven, nu < UMAX
                ks = ((1, 3), (3, 5), (4, 5), (8, 1)) if mode != 2 else ((0, 7), (1, 3), (2, 5), (4, 1))
                for k, r in ks:
                    items = cus * k + r
                    if mode == 2 and k == 0:
                        items = min(r, cus)
                    out.append((fp8, M, w * items, KL, mode))
        for steps in K_STEPS:                                       # K-step edges: waves without steps, stage tails
            for mode, M in ((0, 5), (1, 12), (2, 3)):
                out.append((fp8, M, 8 * 3 if mode != 2 else 16 * 2, KL * steps, mode))           # UMAX 2 (mode 2: 4): one block each
            out.append((fp8, 9, 8 * (cus + 1), KL * steps, 0) if steps <= 3 else (fp8, 2, 8 * 2, KL * steps, 0))
        out.append((fp8, 4, 8 * (16 * cus + 1), KL, 0))              # narrow grid grown past the CU count
    return out


def coverage(cases, cus):
    got = set()
    for fp8, M, N, K, mode in cases:
        p = stream_plan(M, N, K, fp8, mode, cus)
        assert p is not None, (fp8, M, N, K, mode)
        got |= features(p)
    return got


# ------------------------------------------------------------------------------------------------ exact integer GEMV
def gemv_int(x_i, w_u, r_u=None):
    """x_i [M, K] integers, w_u [N, K] and r_u [M, N] in grid units (int64) -> the kernel's result in grid units:
    bf16(sum) or bf16(r + bf16(sum)).  Asserts the condition under which every fp32 partial sum is exact."""
    worst = x_i.abs().to(F64) @ w_u.abs().to(F64).T
    assert float(worst.max()) < EXACT_LIMIT, "sum |x||w| reaches 2^24 grid units: the fp32 sums are no longer order-independent"
    s = (x_i.to(F64) @ w_u.to(F64).T).to(I64)
    v, tie, big = bf_round_int(s)
    info = dict(ties=int(tie.sum()), big=int(big.sum()))
    if r_u is not None:
        assert int((r_u.abs() + v.abs()).max()) < EXACT_LIMIT
        v, tie2, _ = bf_round_int(r_u + v)
        info["ties"] += int(tie2.sum())
    return v, info


def units_to_bf16(v, grid_bits):
    """grid units with <= 8 significant bits -> bf16 (exact)"""
    return (v.to(F64) * 2.0 ** -grid_bits).to(F32).to(BF)


# ------------------------------------------------------------------------------------------------ e4m3fn
def e4m3_value(code):
    """OCP e4m3fn: 1 sign, 4 exponent (bias 7), 3 mantissa bits; no infinities, S.1111.111 is NaN"""
    sign = -1.0 if code & 0x80 else 1.0
    e, m = (code >> 3) & 15, code & 7
    if e == 15 and m == 7:
        return math.nan
    if e == 0:
        return sign * m * 2.0 ** -9
    return sign * (8 + m) * 2.0 ** (e - 10)


E4M3 = [e4m3_value(c) for c in range(256)]
E4M3_POS = E4M3[:0x7f]                              # codes 0 .. 0x7e: 0 .. 448, increasing


def e4m3_codes_of_ints(q):
    """integers |q| <= 16 -> their (exact) e4m3fn codes, uint8"""
    table = torch.zeros(33, dtype=torch.uint8)
    for v in range(-16, 17):
        table[v + 16] = next(c for c in range(256) if E4M3[c] == v and (c < 0x80) == (v >= 0))
    return table.to(q.device)[(q + 16).long()]


def e4m3_rne(y):
    """fp32 tensor -> e4m3fn codes, round to nearest (ties to the even code), saturating at 0x7e = 448; exact fp64 comparisons
    (the difference of an fp32 value and a 4-bit grid value within 2^-9 .. 2^9 is exact in fp64)"""
    a = y.abs().to(F64)
    grid = torch.tensor(E4M3_POS, dtype=F64, device=y.device)
    hi = torch.bucketize(a, grid).clamp(max=0x7e)            # first grid value >= a
    lo = (hi - 1).clamp(min=0)
    dlo, dhi = a - grid[lo], grid[hi] - a
    code = torch.where(dhi < dlo, hi, torch.where(dlo < dhi, lo, torch.where(hi % 2 == 0, hi, lo)))
    code = torch.where(a >= 448.0, torch.full_like(code, 0x7e), code)
    sign = (y.to(F32).view(torch.int32) >> 24) & 0x80
    return (code | sign.to(code.dtype)).to(torch.uint8)


def quant_reference(W):
    """nv_fp8_quant_rows: s = fp32(amax / 448) (1 for an all-zero row), codes = RNE_e4m3fn(fp32(w / s)).  The fp64 quotient of two
    fp32 values rounded to fp32 is the correctly rounded fp32 quotient (53 >= 2 * 24 + 2), subnormal results included."""
    w64 = W.to(F64)
    amax = w64.abs().amax(1)
    s = torch.where(amax > 0, (amax / 448.0).to(F32), torch.ones_like(amax, dtype=F32))
    y = (w64 / s.to(F64)[:, None]).to(F32)
    return e4m3_rne(y), s


def dequant_reference(codes, s):
    """bf16(s * q): the product of an fp32 scale and a 4-bit code value is formed in fp32 (one rounding), then rounded to bf16"""
    q = torch.tensor(E4M3, dtype=F64, device=codes.device)[codes.long()]
    return bf((s.to(F64)[:, None] * q).to(F32).to(F64))


# ------------------------------------------------------------------------------------------------ RMSNorm / SwiGLU operands
def cpu_gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k) + 29) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def rand_ints(g, lo, hi, *shape):
    """int64 in [lo, hi] (CPU generator: the CPU test sees the operands the GPU test uses)"""
    return torch.randint(lo, hi + 1, shape, generator=g)


def norm_operands(g, M, K, rows=None):
    """rows of +-2^a with a different a per row (a in -6 .. 9) -> (x bf16 [rows, K], signs int64).  With eps = 0 the mean square is
    exactly 4^a, rsqrtf returns 2^-a to within a few ulp, and bf16(x * rstd) = +-1 for any rstd within 2^-9 of 2^-a."""
    rows = M if rows is None else rows
    sign = rand_ints(g, 0, 1, rows, K) * 2 - 1
    a = (torch.randperm(16, generator=g)[:rows] - 6) if rows <= 16 else (torch.arange(rows) % 16 - 6)
    x = (sign.to(F64) * (2.0 ** a.to(F64))[:, None]).to(BF)
    return x, sign


SILU_CUTOFF = -88.72                                 # expf(-g) overflows fp32 below it: the kernel's quotient is g / inf = -0


def silu64(g64):
    s = g64 / (1.0 + torch.exp(-g64))
    return torch.where(g64 < SILU_CUTOFF, torch.zeros_like(s), s)


def swiglu_interval(g_bf, u_bf):
    """h = bf16(bf16(silu(g)) * u) at silu (1 - REL_MATH) and silu (1 + REL_MATH); the product of two bf16 values is exact in fp32"""
    s = silu64(g_bf.to(F64))
    ends = []
    for f in (1.0 - REL_MATH, 1.0 + REL_MATH):
        ends.append(bf(bf(s * f).to(F64) * u_bf.to(F64)))
    return ends[0], ends[1]


SWIGLU_CASES = [(7, 16 * 19, 64, False), (16, 16 * 19, 128, True), (3, 32, 2048, False), (12, 48, 1024, True), (5, 16, 64, False),
                (9, 16, 128, True)]                       # (M, N, K, fp8): N = 16 is the smallest accepted, N / 2 = 24 is 8 (mod 16)


def swiglu_case(M, N, K, fp8, seed):
    """operands of a MODE 2 case: x = +-2^a rows, norm_w and W integers -> (x, sign, norm_w, W ints [N, K]); gate = rows [0, N/2) of
    W, up = rows [N/2, N).  |norm_w| <= 4, |W| <= 2 (bf16) / <= 3 (fp8 codes, scale 1): |sum| <= 12 K."""
    g = cpu_gen(seed, M, N, K, int(fp8))
    x, sign = norm_operands(g, M, K)
    nw = rand_ints(g, -4, 4, K)
    W = rand_ints(g, -3, 3, N, K) if fp8 else rand_ints(g, -2, 2, N, K)
    return x, sign, nw, W
