"""GPU: every bf16 GEMM path (nv_gemm_bf16_ws, nv_gemm_bf16_rope_cfg, nv_gemm_fp8w; csrc/gemm_bf16.hip) against an fp64 reference
computed with torch on the device.

Two kinds of input.

EXACT: A and B are integers drawn uniformly from {-3 .. 3}, stored as bf16.  Every product and every partial sum is an integer
below 2^24 (9 * K <= 2^24, asserted), so the fp32 accumulator is exact whatever the K order, tile, pipeline depth or split count,
and the documented result is a pure function of the fp64 sum:
    EPI_STORE bf16(acc) | EPI_ACCUM bf16(C0 + bf16(acc)) | EPI_RESID bf16(R + bf16(acc)) | EPI_BIAS bf16(acc + bias[n])
C0, R and bias are even integers in [-510, 510] (bf16 holds them, the fp32 add is exact).  These cases assert torch.equal.  Sums pass
256 -- where bf16 stops holding every integer -- at K >= 1024, and an odd acc under an even addend above 256 is an exact tie
(257 -> 256, 259 -> 260): every exact case asserts that its reference contains a tie and a value above 256, except EPI_STORE at
K < 1024, where inputs from {-3 .. 3} cannot reach 256 (|acc| <= 9 K; in practice ~4 sqrt(K)).  The rounding of the reference
(float64 -> float32 -> bfloat16 by torch) is itself checked against explicit integer arithmetic.

RANDOM: normal inputs keep the fp32-accumulate claim honest on non-integer data.  With x the fp64 sum, S = sum_k |a_k||b_k|,
E = (K + 1) * 2^-24 * S (fp32 accumulation in any order) and u = 2^-8 (one bf16 rounding), per element:
    EPI_STORE, EPI_BIAS :  |got - x|       <= E + u (|x| + E)
    EPI_ACCUM, EPI_RESID:  |got - (R + x)| <= E + u (|x| + E) + u (|R| + |x| + E)
Nothing is measured into these bounds.  The largest err / bound seen is printed (`pytest -s`) and recorded in DESIGN.md section 2.

Every call writes into a view of a larger NaN-filled buffer (extra columns up to ldc, guard rows above and below): everything
outside [0, M) x [0, N) must be bitwise unchanged.  Every call is given a valid decoy R even where the epilogue reads none."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
NT, NN, TN = 0, 1, 2
STORE, ACCUM, RESID, BIAS, SWIGLU, ROPE = 0, 1, 2, 3, 4, 5
EPI_NAME = {STORE: "store", ACCUM: "accum", RESID: "resid", BIAS: "bias", SWIGLU: "swiglu"}
LAYOUT_NAME = {NT: "NT", NN: "NN", TN: "TN"}
NV_ERR_SHAPE = -2
U = 2.0 ** -8
GUARD = 3                       # guard rows above and below every output view


def dev():
    return torch.device("cuda:0")


def gen(seed, device="cuda:0"):
    return torch.Generator(device=device).manual_seed(seed)


def ints(rows, cols, seed, lo=-3, hi=3, pad=8):
    """integers uniform in {lo .. hi} as a bf16 STRIDED view (ld = cols rounded up to 8, + pad)"""
    ld = (cols + 7) // 8 * 8 + pad
    t = torch.randint(lo, hi + 1, (rows, ld), generator=gen(seed), device=dev()).to(BF)
    return t[:, :cols]


def even_ints(rows, cols, seed):
    return (2 * torch.randint(-255, 256, (rows, cols), generator=gen(seed), device=dev())).to(BF)


def normal(rows, cols, seed, scale=1.0, pad=8):
    ld = (cols + 7) // 8 * 8 + pad
    t = (torch.randn(rows, ld, generator=gen(seed), device=dev()) * scale).to(BF)
    return t[:, :cols]


# ---------------------------------------------------------------------------------------------- the launch plan, restated
def tail_split(rem, KT):
    """csrc/gemm_bf16.hip tail_split(): K-slices of the tiles of a last, partial round of 256"""
    if rem <= 0 or rem > 128:
        return 1
    max_split, min_slice = (8, 8) if rem <= 16 else (6, 20)
    split = min(256 // rem, max_split, KT // min_slice, 512 // rem)
    return split if split >= 2 else 1


def has_cut_off_instance(layout, epi):
    return (layout == NT and epi in (STORE, RESID, ROPE)) or (layout == NN and epi == STORE)


def plan(layout, epi, tile, M, N, K):
    """(fragment rows per wave, tiles, rem, split) of a 256-wide tile launch with the workspace (tile = 8, 84..87, 94, 95)"""
    tme = 8 if tile == 8 else tile % 10
    if not has_cut_off_instance(layout, epi):
        tme = 8
    tiles = -(-M // (32 * tme)) * -(-N // 256)
    rem = tiles % 256
    return tme, tiles, rem, tail_split(rem, -(-K // 64))


# ---------------------------------------------------------------------------------------------- references
def bf_round(x64):
    return x64.to(F32).to(BF)


def bf_round_int(v):
    """round-to-nearest-even of int64 values to 8 significant bits (the bf16 grid), by integer arithmetic; -> (rounded, tie, big)"""
    a = v.abs()
    e = torch.zeros_like(a)
    for k in range(17):
        e += (a >= (1 << (8 + k))).to(a.dtype)
    q = a >> e
    rem = a - (q << e)
    half = torch.where(e > 0, torch.ones_like(a) << (e - 1).clamp(min=0), torch.zeros_like(a))
    tie = (e > 0) & (rem == half)
    up = (e > 0) & ((rem > half) | (tie & ((q & 1) == 1)))
    r = (q + up.to(a.dtype)) << e
    return torch.where(v < 0, -r, r), tie, a > 256


def acc64(layout, A, B):
    a, b = A.to(F64), B.to(F64)
    return a @ b.t() if layout == NT else (a @ b if layout == NN else a.t() @ b)


def abs64(layout, A, B):
    return acc64(layout, A.abs(), B.abs())


def exact_reference(acc, epi, addend, K):
    """documented result on exact-integer data (bf16 tensor); asserts the rounding against integer arithmetic and, where the inputs
    can reach it, that the case contains a tie and a value above 256"""
    assert 9 * K <= 2 ** 24
    ai = acc.round().to(torch.int64)
    assert torch.equal(ai.to(F64), acc), "exact-integer inputs must give an integer fp64 sum"
    if epi == STORE:
        pre = ai
    elif epi == BIAS:
        pre = ai + addend.to(F64).to(torch.int64)
    else:
        inner, _, _ = bf_round_int(ai)
        assert torch.equal(bf_round(acc).to(F64), inner.to(F64)), "reference rounding (inner) disagrees with integer arithmetic"
        pre = inner + addend.to(F64).to(torch.int64)
    want_i, tie, big = bf_round_int(pre)
    want = bf_round(pre.to(F64))
    assert torch.equal(want.to(F64), want_i.to(F64)), "reference rounding disagrees with integer arithmetic"
    if epi != STORE or K >= 1024:
        assert bool(tie.any()) and bool(big.any()), f"case has no tie / no value above 256 (ties {int(tie.sum())}, big {int(big.sum())})"
    return want


_ratio = {"max": 0.0}


def check_random(got, x, S, K, epi, addend, what):
    """the derived per-element bound of the module docstring"""
    E = (K + 1) * 2.0 ** -24 * S
    b = E + U * (x.abs() + E)
    if epi in (ACCUM, RESID):
        r = addend.to(F64)
        want = r + x
        b = b + U * (r.abs() + x.abs() + E)
    elif epi == BIAS:
        want = x + addend.to(F64)
        b = E + U * (want.abs() + E)
    else:
        want = x
    g = got.to(F64)
    assert torch.isfinite(g).all(), f"{what}: non-finite output"
    err = (g - want).abs()
    ratio = (err / b.clamp(min=1e-300)).max().item()
    _ratio["max"] = max(_ratio["max"], ratio)
    print(f"GEMM_REF_RATIO {what}: max err/bound {ratio:.4f}  (running max {_ratio['max']:.4f})")
    assert ratio <= 1.0, f"{what}: err/bound {ratio:.4f}; max err {err.max().item():.4e}"


# ---------------------------------------------------------------------------------------------- guarded output + launch
class Out:
    """an [M, width] bf16 view with row stride ldc, `off` elements into a NaN-filled buffer with GUARD rows above and below"""

    def __init__(self, M, width, ldc=None, off=0, init=None):
        ldc = width + 8 if ldc is None else ldc
        assert ldc >= width
        n = (M + 2 * GUARD) * ldc + off + 16
        self.buf = torch.full((n,), float("nan"), dtype=BF, device=dev())
        start = GUARD * ldc + off
        assert start >= 0 and start + (M - 1) * ldc + width <= n - GUARD * ldc
        self.view = torch.as_strided(self.buf, (M, width), (ldc, 1), start)
        if init is not None:
            self.view.copy_(init)
        self.outside = torch.ones(n, dtype=torch.bool, device=dev())
        torch.as_strided(self.outside, (M, width), (ldc, 1), start).fill_(False)
        self.before = self.buf.view(torch.int16)[self.outside].clone()

    def check_write_set(self, what):
        after = self.buf.view(torch.int16)[self.outside]
        assert torch.equal(after, self.before), f"{what}: wrote outside [0, M) x [0, N) ({int((after != self.before).sum())} elements)"


def workspace():
    from navillm_amd import ops
    ops._gemm_ws(dev())
    return ops._gemm_ws_cache[ops._st()]


def launch(layout, A, B, out, R, epi, tile, ws=True, expect=0):
    """nv_gemm_bf16_ws on views (what ops.gemm_bf16 calls, without its shape rules); R is always a valid tensor"""
    from navillm_amd import ops
    if layout == NT:
        (M, K), N = A.shape, B.shape[0]
    elif layout == NN:
        (M, K), N = A.shape, B.shape[1]
    else:
        (K, M), N = A.shape, B.shape[1]
    assert out.shape[0] == M and out.shape[1] == (2 * N if epi == SWIGLU else N) and out.stride(1) == 1
    assert A.stride(1) == 1 and B.stride(1) == 1
    w = workspace()
    ldr = R.stride(0) if R.dim() == 2 else 0
    rc = ops._L().nv_gemm_bf16_ws(layout, A.data_ptr(), B.data_ptr(), out.data_ptr(), R.data_ptr(), M, N, K, A.stride(0), B.stride(0),
                                  out.stride(0), ldr, epi, tile, w.data_ptr() if ws else None, ops._st())
    assert rc == expect, f"nv_gemm_bf16_ws returned {rc}"
    torch.cuda.synchronize()
    if ws:
        assert not bool(w[:4096].any()), "split-K ticket words are not zero after the launch"


def operands(layout, M, N, K, seed, make=ints):
    if layout == NT:
        return make(M, K, seed), make(N, K, seed + 1)
    if layout == NN:
        return make(M, K, seed), make(K, N, seed + 1)
    return make(K, M, seed), make(K, N, seed + 1)


_cache = {}


def exact_case(layout, M, N, K, seed):
    """operands + fp64 sum of an exact-integer case, built once per shape and shared across tiles and epilogues"""
    key = (layout, M, N, K, seed)
    if key not in _cache:
        if len(_cache) > 6:
            _cache.clear()
        A, B = operands(layout, M, N, K, seed)
        _cache[key] = (A, B, acc64(layout, A, B))
    return _cache[key]


def addend_for(epi, M, N, seed):
    """C0 / R: even integers [M, N]; bias: even integers [N] (inside a longer allocation)"""
    if epi == BIAS:
        return even_ints(1, N + 8, seed)[0, :N]
    return even_ints(M, N, seed)


def run_exact(layout, epi, tile, M, N, K, seed, ldc=None, off=0, ws=True, odd_r=False):
    """one exact-integer launch: result == documented function of the fp64 sum, write set, tickets; -> the [M, N] result"""
    A, B, acc = exact_case(layout, M, N, K, seed)
    add = addend_for(epi, M, N, seed + 7)
    want = exact_reference(acc, epi, add, K)
    out = Out(M, N, ldc, off, init=add if epi == ACCUM else None)
    if epi == RESID and odd_r:                       # R with an odd row stride, one element off its allocation's alignment
        ldr = N + 1 + N % 2
        rbuf = torch.zeros((M * ldr + 9,), dtype=BF, device=dev())
        R = torch.as_strided(rbuf, (M, N), (ldr, 1), 1)
        R.copy_(add)
    elif epi in (RESID, BIAS):
        R = add
    else:
        R = torch.full((M, N + 8), float("nan"), dtype=BF, device=dev())[:, :N]      # decoy: must not be read
    what = f"{LAYOUT_NAME[layout]} {EPI_NAME[epi]} tile {tile} {M}x{N}x{K} ldc {out.view.stride(0)} off {off}"
    launch(layout, A, B, out.view, R, epi, tile, ws)
    out.check_write_set(what)
    got = out.view
    if not torch.equal(got, want):
        bad = (got.view(torch.int16) != want.view(torch.int16))
        idx = torch.nonzero(bad)[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())}/{bad.numel()} elements differ from the exact reference; first at {idx}: "
                             f"got {got[tuple(idx)].item()} want {want[tuple(idx)].item()} (acc {acc[tuple(idx)].item()})")
    return got.clone()


def swiglu_reference(acc, gu):
    """swiglu_bwd_elem on dh = bf16(acc) in fp64 with its two bf16 roundings; -> d(gate|up) fp64 [M, 2N]"""
    N = acc.shape[1]
    dh = bf_round(acc).to(F64)
    g, u = gu[:, :N].to(F64), gu[:, N:].to(F64)
    sg = 1.0 / (1.0 + torch.exp(-g))
    du = dh * bf_round(g * sg).to(F64)
    dg = bf_round(dh * u).to(F64) * (sg * (1.0 + g * (1.0 - sg)))
    return torch.cat([dg, du], 1)


def run_swiglu(tile, M, N, K, seed, ldc=None, off=0, ws=True, odd_r=False):
    """NN + EPI_SWIGLU_BWD on exact-integer dx, W and a random-normal gate|up: the bound of
    test_kernels_gpu.py::test_gemm_swiglu_bwd_epilogue_equals_two_pass (2^-7 relative + 1e-3 of the tensor maximum; SiLU is not exact)"""
    A, B, acc = exact_case(NN, M, N, K, seed)
    if odd_r:
        ldr = 2 * N + 1
        rbuf = torch.zeros((M * ldr + 9,), dtype=BF, device=dev())
        gu = torch.as_strided(rbuf, (M, 2 * N), (ldr, 1), 1)
        gu.copy_(normal(M, 2 * N, seed + 9))
    else:
        gu = normal(M, 2 * N, seed + 9)
    want = swiglu_reference(acc, gu)
    out = Out(M, 2 * N, ldc, off)
    what = f"NN swiglu tile {tile} {M}x{N}x{K} ldc {out.view.stride(0)} off {off}"
    launch(NN, A, B, out.view, gu, SWIGLU, tile, ws)
    out.check_write_set(what)
    got = out.view.to(F64)
    assert torch.isfinite(got).all(), f"{what}: non-finite output inside [0, M) x [0, 2N)"
    tol = 2.0 ** -7 * want.abs() + 1e-3 * want.abs().max()
    err = (got - want).abs()
    assert bool((err <= tol).all()), f"{what}: {int((err > tol).sum())} elements off; max err {err.max().item():.4e}"
    return out.view.clone()


EPIS = {NT: (STORE, ACCUM, RESID, BIAS), NN: (STORE, ACCUM, RESID, BIAS, SWIGLU), TN: (STORE, ACCUM, RESID, BIAS)}
TILES = (1, 8, 84, 85, 86, 87, 94, 95, 0)


# ---------------------------------------------------------------------------------------------- the reference's own rounding
def test_reference_rounding_ties_to_even():
    v = torch.tensor([255, 256, 257, 258, 259, 260, 261, 511, 513, 515, 1025, 1026, 1027, 1028, 1030, -257, -259, 65793], device=dev())
    want = torch.tensor([255, 256, 256, 258, 260, 260, 260, 512, 512, 516, 1024, 1024, 1024, 1024, 1032, -256, -260, 66048], device=dev())
    r, tie, big = bf_round_int(v)
    assert torch.equal(r, want)
    assert torch.equal(bf_round(v.to(F64)).to(F64), want.to(F64))
    assert tie.tolist()[:7] == [False, False, True, False, True, False, True] and big.tolist()[:3] == [False, False, True]
    # and a sampled sub-block of an fp64 device sum against a CPU recomputation
    A, B, acc = exact_case(NT, 333, 520, 1024, 100)
    sub = A[:17].cpu().to(F64) @ B[500:].cpu().to(F64).t()
    assert torch.equal(acc[:17, 500:].cpu(), sub)


# ---------------------------------------------------------------------------------------------- layout x epilogue x tile
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("layout,epi", [(l, e) for l in (NT, NN, TN) for e in EPIS[l]],
                         ids=[f"{LAYOUT_NAME[l]}-{EPI_NAME[e]}" for l in (NT, NN, TN) for e in EPIS[l]])
def test_exact_layout_epilogue_tile(layout, epi, tile):
    """every epilogue dispatch_epi accepts for a layout on every tile configuration: ragged M and N edges (333 x 520: 8 columns in
    the last 256-wide tile, 77 rows in the last 128-row one), strided A and B views, ldc = N + 8 (staged stores), K = 1024 (NT, NN) /
    1061 (TN, ragged contraction)"""
    M, N, K = 333, 520, 1061 if layout == TN else 1024
    if epi == SWIGLU:
        run_swiglu(tile, M, N, K, 100)
    else:
        run_exact(layout, epi, tile, M, N, K, 100)


@pytest.mark.parametrize("epi", [STORE, ACCUM], ids=["store", "accum"])
@pytest.mark.parametrize("K", [1, 7, 63, 64, 65, 8300])
def test_exact_tn_ragged_k(K, epi):
    """the weight-gradient form (TN, 256-wide tile, workspace) with a ragged contraction length, down to a single row"""
    run_exact(TN, epi, 8, 300, 264, K, 200)


# ---------------------------------------------------------------------------------------------- split-K tail
def run_split_case(layout, epi, tile, M, N, K, seed, rem, split, **kw):
    tme, tiles, rem_, split_ = plan(layout, epi, tile, M, N, K)
    assert (rem_, split_) == (rem, split), (f"this case no longer splits as intended: {LAYOUT_NAME[layout]} {EPI_NAME[epi]} tile {tile} "
                                            f"{M}x{N}x{K} has {tiles} tiles, rem {rem_}, split {split_}; wanted rem {rem}, split {split}")
    if epi == SWIGLU:
        a = run_swiglu(tile, M, N, K, seed, ws=True, **kw)
        b = run_swiglu(tile, M, N, K, seed, ws=False, **kw)
    else:
        a = run_exact(layout, epi, tile, M, N, K, seed, ws=True, **kw)
        b = run_exact(layout, epi, tile, M, N, K, seed, ws=False, **kw)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16)), "split-K result differs from the unsplit run"


SPLIT_K = {2: 1024, 3: 1536, 4: 2048, 5: 2560, 6: 3072, 7: 3584, 8: 4096}


@pytest.mark.parametrize("tile", [8, 84, 85, 86, 87])
@pytest.mark.parametrize("layout", [NT, NN, TN], ids=["NT", "NN", "TN"])
@pytest.mark.parametrize("split", sorted(SPLIT_K), ids=[f"rem2-split{s}" for s in sorted(SPLIT_K)])
def test_exact_splitk_every_split_count(split, layout, tile):
    """M = 100, N = 512: two tail tiles and no full tile for every tile height; the K-tile count sets 2 .. 8 slices, so the band
    reduction shares 4, 5, 6, 7 and 8 fragment rows over every slice count (unevenly, and with slices that own no band).  Bit for bit
    the unsplit run and the reference, for STORE and every reading epilogue of the layout."""
    K = SPLIT_K[split]
    for epi in (STORE, ACCUM, RESID) + ((SWIGLU,) if layout == NN else ()):
        run_split_case(layout, epi, tile, 100, 512, K, 300, 2, split)


# (M, N, K, rem, split) on the full 256 x 256 tile
SPLIT_SHAPES = [(670, 22016, 4096, 2, 8),        # 258 tiles: 256 full + 2 tail
                (2104, 3072, 4096, 108, 2),      # the rem > 16 branch: min(256 / rem, 6, K-tiles / 20)
                (700, 5120, 2560, 60, 2),
                (700, 5120, 4096, 60, 3),
                (700, 5120, 5120, 60, 4),
                (700, 4096, 6400, 48, 5),
                (700, 3072, 7680, 36, 6)]


@pytest.mark.parametrize("layout", [NT, NN, TN], ids=["NT", "NN", "TN"])
@pytest.mark.parametrize("M,N,K,rem,split", SPLIT_SHAPES, ids=[f"{m}x{n}x{k}-rem{r}-split{s}" for m, n, k, r, s in SPLIT_SHAPES])
def test_exact_splitk_other_tails(M, N, K, rem, split, layout):
    for epi in (STORE, ACCUM, RESID):
        run_split_case(layout, epi, 8, M, N, K, 400, rem, split)
    _cache.clear()


# ---------------------------------------------------------------------------------------------- element-wise epilogue
ELEMENTWISE = [(NT, STORE), (NT, ACCUM), (NT, RESID), (NT, BIAS), (NN, STORE), (NN, SWIGLU), (TN, ACCUM), (TN, RESID), (TN, BIAS)]


@pytest.mark.parametrize("tile", [1, 8, 84])
@pytest.mark.parametrize("extra", [0, 1, 3], ids=["ldcN", "ldcN+1", "ldcN+3"])
@pytest.mark.parametrize("N", [77, 129, 250])
def test_exact_elementwise_epilogue(N, extra, tile):
    """N % 8 != 0 rules the staged stores out: per-element stores, with ldc = N, N + 1, N + 3, C one element (2 bytes) off its
    allocation's alignment, R with an odd row stride and one element off"""
    M, K = 150, 1024
    for layout, epi in ELEMENTWISE:
        if epi == SWIGLU:
            run_swiglu(tile, M, N, K, 500 + N, ldc=2 * N + extra, off=1, odd_r=True)
        else:
            run_exact(layout, epi, tile, M, N, K, 500 + N, ldc=N + extra, off=1, odd_r=True)


@pytest.mark.parametrize("tile", [8, 84])
@pytest.mark.parametrize("why", ["ldc%8", "C+2B", "ldr%8", "R+2B"])
def test_exact_elementwise_epilogue_each_trigger(why, tile):
    """N % 8 == 0: each of the other conditions alone sends the launch down the element-wise path"""
    M, N, K = 150, 264, 1024
    A, B, acc = exact_case(NT, M, N, K, 600)
    add = even_ints(M, N, 607)
    want = exact_reference(acc, RESID, add, K)
    ldc, off, ldr, roff = {"ldc%8": (N + 4, 0, N + 8, 0), "C+2B": (N + 8, 1, N + 8, 0), "ldr%8": (N + 8, 0, N + 3, 0),
                           "R+2B": (N + 8, 0, N + 8, 1)}[why]
    rbuf = torch.zeros((M * ldr + 16,), dtype=BF, device=dev())
    R = torch.as_strided(rbuf, (M, N), (ldr, 1), roff)
    R.copy_(add)
    out = Out(M, N, ldc, off)
    launch(NT, A, B, out.view, R, RESID, tile)
    out.check_write_set(why)
    assert torch.equal(out.view, want)


@pytest.mark.parametrize("tile", [8, 84])
def test_exact_elementwise_epilogue_splitk_odd_n(tile):
    """a split-K tail (100 x 511 x 2048: two tail tiles, four slices) whose bands are stored element by element"""
    for layout, epi in ((NT, STORE), (NT, ACCUM), (NT, RESID), (NN, SWIGLU), (TN, ACCUM)):
        run_split_case(layout, epi, tile, 100, 511, 2048, 700, 2, 4, ldc=(2 if epi == SWIGLU else 1) * 511 + 1, off=1, odd_r=True)


# ---------------------------------------------------------------------------------------------- random-normal inputs
@pytest.mark.parametrize("tile", [1, 8, 85, 0])
@pytest.mark.parametrize("layout", [NT, NN, TN], ids=["NT", "NN", "TN"])
@pytest.mark.parametrize("M,N,K", [(333, 520, 1024), (100, 512, 4096)], ids=["333x520x1024", "100x512x4096-split8"])
def test_random_normal_derived_bound(M, N, K, layout, tile):
    Kc = K + 37 if layout == TN else K
    A, B = operands(layout, M, N, Kc, 800, make=normal)
    x, S = acc64(layout, A, B), abs64(layout, A, B)
    for epi in (STORE, ACCUM, RESID, BIAS):
        add = normal(1, N + 8, 811)[0, :N] if epi == BIAS else normal(M, N, 811, pad=0)
        out = Out(M, N, init=add if epi == ACCUM else None)
        R = add if epi in (RESID, BIAS) else torch.full((M, N), float("nan"), dtype=BF, device=dev())
        what = f"{LAYOUT_NAME[layout]} {EPI_NAME[epi]} tile {tile} {M}x{N}x{Kc} normal"
        launch(layout, A, B, out.view, R, epi, tile)
        out.check_write_set(what)
        check_random(out.view, x, S, Kc, epi, add, what)


# ---------------------------------------------------------------------------------------------- RoPE epilogue
@pytest.mark.parametrize("tile", [84, 8, 0])
def test_rope_epilogue_fp64_reference(tile):
    """nv_gemm_bf16_rope_cfg on exact-integer x and W: the reference applies the documented rotation (HF apply_rotary_pos_emb in
    bf16: out = bf16(bf16(x cos) + bf16(-+ partner sin)), partner 64 columns away inside a 128-wide head) to bf16(acc) with the bf16
    tables, in fp64.  Bound: the STORE bound carried through the rotation, plus one rounding of the rotated value; on this data the
    STORE error is zero, so the rounded reference must also be met bit for bit.  Columns >= rope_cols are plain stores."""
    from navillm_amd import ops
    M, H, hd, K = 300, 2, 128, 1024
    d = H * hd
    N, cols = 3 * d, 2 * d
    A, W, acc = exact_case(NT, M, N, K, 900)
    S = abs64(NT, A, W)
    pos = ((torch.arange(M, dtype=torch.int32) * 7) % 211).to(dev())
    inv = 1.0 / (10000.0 ** (torch.arange(0, hd, 2, dtype=torch.float32) / hd))
    ang = torch.arange(256, dtype=torch.float32)[:, None] * inv[None, :]
    cos_t = torch.cat([ang.cos(), ang.cos()], 1).to(BF).to(dev())
    sin_t = torch.cat([ang.sin(), ang.sin()], 1).to(BF).to(dev())
    x = bf_round(acc).to(F64)
    E = (K + 1) * 2.0 ** -24 * S
    bx = E + U * (acc.abs() + E)                                        # STORE bound on what is rotated
    col = torch.arange(cols, device=dev())
    lo = (col % hd) < hd // 2
    partner = torch.where(lo, col + hd // 2, col - hd // 2)
    c = cos_t[pos.long()][:, col % (hd // 2)].to(F64)
    s = sin_t[pos.long()][:, col % (hd // 2)].to(F64) * torch.where(lo, -1.0, 1.0).to(F64)
    y, by = x[:, partner], bx[:, partner]
    rot = bf_round(x[:, :cols] * c).to(F64) + bf_round(y * s).to(F64)
    want = torch.cat([bf_round(rot), bf_round(acc[:, cols:])], 1)
    out = Out(M, N)
    rc = ops._L().nv_gemm_bf16_rope_cfg(A.data_ptr(), W.data_ptr(), out.view.data_ptr(), cos_t.data_ptr(), sin_t.data_ptr(), pos.data_ptr(),
                                        M, N, K, A.stride(0), W.stride(0), out.view.stride(0), 0, cols, tile, workspace().data_ptr(), ops._st())
    assert rc == 0
    torch.cuda.synchronize()
    out.check_write_set(f"rope tile {tile}")
    got = out.view.to(F64)
    assert torch.isfinite(got).all()
    carried = bx[:, :cols] * c.abs() + by * s.abs()
    bound = carried + U * (rot.abs() + carried)
    err = (got[:, :cols] - rot).abs()
    assert bool((err <= bound).all()), f"rope tile {tile}: max err/bound {(err / bound.clamp(min=1e-300)).max().item():.4f}"
    assert torch.equal(out.view, want), "RoPE epilogue differs from the rounded fp64 reference on exact data"


# ---------------------------------------------------------------------------------------------- fp8 codes
@pytest.mark.parametrize("epi", [STORE, RESID], ids=["store", "resid"])
@pytest.mark.parametrize("tile", [84, 85])
@pytest.mark.parametrize("mode", [7, 9])
def test_fp8w_exact(mode, tile, epi):
    """nv_gemm_fp8w on integer-valued e4m3 codes and power-of-two scales: bf16(s q) is exact, s on the fp32 accumulator (mode 9) is
    exact, so both modes must give the documented function of the fp64 sum bit for bit"""
    from navillm_amd import ops
    M, N, K = 300, 520, 1024
    A = ints(M, K, 1000)
    qf = torch.randint(-3, 4, (N, K + 16), generator=gen(1001, "cpu")).to(F32)
    q8 = qf.to(torch.float8_e4m3fn)
    assert torch.equal(q8.to(F32), qf)                                   # small integers are e4m3 values
    codes = q8.view(torch.uint8).to(dev())[:, :K]
    scales = (2.0 ** torch.randint(-2, 3, (N,), generator=gen(1002, "cpu")).to(F32)).to(dev())
    assert 9 * 4 * K * 4 <= 2 ** 24                                      # sums of multiples of 1/4 below 36 K: exact in fp32
    acc = A.to(F64) @ (qf[:, :K].to(dev()).to(F64) * scales.to(F64)[:, None]).t()
    add = even_ints(M, N, 1003)
    pre = bf_round(acc).to(F64) + add.to(F64) if epi == RESID else acc
    want = bf_round(pre)
    assert bool((pre.abs() > 256).any())
    out = Out(M, N)
    R = add if epi == RESID else torch.full((M, N), float("nan"), dtype=BF, device=dev())
    rc = ops._L().nv_gemm_fp8w(A.data_ptr(), codes.data_ptr(), scales.data_ptr(), out.view.data_ptr(), R.data_ptr(), M, N, K, A.stride(0),
                               codes.stride(0), out.view.stride(0), R.stride(0), epi, mode, tile, workspace().data_ptr(), ops._st())
    assert rc == 0
    torch.cuda.synchronize()
    out.check_write_set(f"fp8w mode {mode} tile {tile}")
    assert torch.equal(out.view, want)


def test_fp8w_refused_shape_leaves_out_untouched():
    from navillm_amd import ops
    M, N, K = 300, 520, 96                                               # K % 64 != 0
    A = ints(M, K, 1010)
    codes = torch.zeros((N, 128), dtype=torch.uint8, device=dev())[:, :K]
    scales = torch.ones(N, dtype=F32, device=dev())
    out = Out(M, N)
    whole = out.buf.view(torch.int16).clone()
    rc = ops._L().nv_gemm_fp8w(A.data_ptr(), codes.data_ptr(), scales.data_ptr(), out.view.data_ptr(), None, M, N, K, A.stride(0),
                               codes.stride(0), out.view.stride(0), 0, STORE, 7, 84, workspace().data_ptr(), ops._st())
    torch.cuda.synchronize()
    assert rc == NV_ERR_SHAPE
    assert torch.equal(out.buf.view(torch.int16), whole)


# ---------------------------------------------------------------------------------------------- the 7B bench shapes
@pytest.mark.parametrize("N,K", [(12288, 4096), (4096, 4096), (22016, 4096), (4096, 11008)])
@pytest.mark.parametrize("M", [8300, 4200, 670])
def test_exact_bench_shapes_planned_tile(M, N, K):
    """the Linear shapes of the 7B training step through the planned tile: forward (NT, y = x W^T), dgrad (NN, dx = dy W; the
    down-projection's with the SwiGLU-backward epilogue) and wgrad (TN + EPI_ACCUM, dW += dy^T x)"""
    _cache.clear()
    x, W, dy = ints(M, K, 1100), ints(N, K, 1101), ints(M, N, 1102)
    assert 9 * max(M, N, K) <= 2 ** 24

    def one(layout, A, B, epi, rows, cols, Kc, seed):
        acc = acc64(layout, A, B)
        add = addend_for(epi, rows, cols, seed)
        want = exact_reference(acc, epi, add, Kc)
        out = Out(rows, cols, init=add if epi == ACCUM else None)
        launch(layout, A, B, out.view, add, epi, 0)
        out.check_write_set(f"bench {LAYOUT_NAME[layout]} {rows}x{cols}x{Kc}")
        assert torch.equal(out.view, want), f"bench {LAYOUT_NAME[layout]} {EPI_NAME[epi]} {rows}x{cols}x{Kc}"

    one(NT, x, W, STORE, M, N, K, 1103)
    one(TN, dy, x, ACCUM, N, K, M, 1104)
    if (N, K) == (4096, 11008):
        _cache[(NN, M, K, N, 1105)] = (dy, W, acc64(NN, dy, W))
        run_swiglu(0, M, K, N, 1105)
        _cache.clear()
    else:
        one(NN, dy, W, STORE, M, K, N, 1106)


# ---------------------------------------------------------------------------------------------- K = 0
@pytest.mark.parametrize("tile", [1, 8, 84, 0])
@pytest.mark.parametrize("layout", [NT, NN, TN], ids=["NT", "NN", "TN"])
def test_k0_is_the_empty_sum(layout, tile):
    """K == 0 (include/navillm_hip.h): STORE writes zeros, ACCUM leaves bf16(C0), RESID writes bf16(R), BIAS writes bf16(bias[n]);
    A and B are not read (they are 32-byte NaN-filled allocations here)"""
    from navillm_amd import ops
    M, N = 333, 520
    A = torch.full((16,), float("nan"), dtype=BF, device=dev())
    for epi in (STORE, ACCUM, RESID, BIAS):
        add = normal(1, N + 8, 1200)[0, :N] if epi == BIAS else normal(M, N, 1200, pad=0)
        out = Out(M, N, init=add if epi == ACCUM else None)
        R = add if epi in (RESID, BIAS) else torch.full((M, N), float("nan"), dtype=BF, device=dev())
        rc = ops._L().nv_gemm_bf16_ws(layout, A.data_ptr(), A.data_ptr(), out.view.data_ptr(), R.data_ptr(), M, N, 0, 8, 8, out.view.stride(0),
                                      R.stride(0) if R.dim() == 2 else 0, epi, tile, workspace().data_ptr(), ops._st())
        assert rc == 0
        torch.cuda.synchronize()
        out.check_write_set(f"K=0 {LAYOUT_NAME[layout]} {EPI_NAME[epi]} tile {tile}")
        want = torch.zeros((M, N), dtype=BF, device=dev()) if epi == STORE else (add.expand(M, N) if epi == BIAS else add)
        assert torch.equal(out.view, want), f"K=0 {LAYOUT_NAME[layout]} {EPI_NAME[epi]} tile {tile}"
