"""Shared pieces of the fp64-reference GPU tests of the row-op and loss/optimizer kernels (test_rowops_ref_gpu.py,
test_loss_optim_ref_gpu.py): guarded buffers, read-only snapshots, the reference rounding and the two kinds of assertion.

Rounding.  `bf(x64)` is float64 -> float32 -> bfloat16 by torch (round-to-nearest-even twice; test_gemm_ref_gpu.py checks that
composition against integer arithmetic).  It reproduces "one correctly rounded fp32 operation, then the bf16 conversion" bit for
bit whenever the fp64 value of the operation is exact (a product of a bf16 and an fp32 value has 32 significant bits, a sum of two
values of comparable size is exact as well).

Constants shared by every derived bound:  u = 2^-8 (one bf16 rounding), e = 2^-24 (one fp32 rounding), REL_MATH = 4 * 2^-23:
a stated cap of 4 ulp on expf / logf / rsqrtf / sqrtf / division of the device (no ulp table ships with the ROCm installation this
was written on; an fp32 ulp is at most 2^-23 of the value), TINY = 2^-126: the smallest normal fp32 (and bf16) number -- a result
below it may lose all its bits (subnormal spacing, or a flush-to-zero denormal mode), so a bound that would otherwise be purely
relative carries it as an absolute term.  SECOND = 1.01 covers the products of two such relative errors (each is < 2^-7).
Nothing in a bound is measured on the kernel."""
import torch

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
I32, I64 = torch.int32, torch.int64
U = 2.0 ** -8
E = 2.0 ** -24
KULP = 4
REL_MATH = KULP * 2.0 ** -23
TINY = 2.0 ** -126
SECOND = 1.01
GUARD = 3                         # guard rows above and below every guarded view
NAN_BITS = {BF: 0x7FC0, F32: 0x7FC00000}
PATTERN = {BF: 0x4049, F32: 0x40490FDB}     # pi: a fixed pattern for buffers the kernel reads and modifies
NV_ERR_ARG, NV_ERR_SHAPE = -1, -2


def dev():
    return torch.device("cuda:0")


def gen(*key):
    """a device generator seeded from the case parameters"""
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k) + 17) % (2 ** 31 - 1)
    return torch.Generator(device="cuda:0").manual_seed(seed)


def randn(g, *shape, scale=1.0, dtype=BF):
    return (torch.randn(*shape, generator=g, device=dev()) * scale).to(dtype)


def randint(g, lo, hi, *shape, dtype=I32):
    return torch.randint(lo, hi, shape, generator=g, device=dev()).to(dtype)


def randperm(g, n, dtype=I32):
    return torch.randperm(n, generator=g, device=dev()).to(dtype)


def bf(x64):
    return x64.to(F32).to(BF)


def f32r(x64):
    return x64.to(F32)


def gamma(n):
    """(1 + e)^n - 1 <= n e / (1 - n e): n fp32 roundings in a row"""
    return n * E / (1.0 - n * E)


def _ibits(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}.get(t.element_size(), torch.int64))


def bits_equal(a, b):
    return torch.equal(_ibits(a.contiguous()), _ibits(b.contiguous()))


class Guarded:
    """a [rows, width] view (row stride ld >= width) inside a larger buffer that is filled with a sentinel bit pattern: GUARD rows
    above and below and the columns [width, ld) of every row.  The view starts a multiple of 8 elements into the buffer (16-byte
    aligned, as flat.py's ALIGN = 64 guarantees in production).  `init` fills the view; `check(what, written)` asserts that nothing
    outside `written` (a [rows, width] bool mask, a column slice / row index pair, or everything in the view) changed a bit."""

    def __init__(self, rows, width, dtype=BF, ld=None, init=None, fill=None):
        ld = width if ld is None else ld
        assert ld >= width
        guard = (min(GUARD * ld, 1 << 16) + 7) // 8 * 8
        n = guard + rows * ld + guard + 8
        bits = NAN_BITS[dtype] if fill is None else fill
        self.buf = torch.empty((n,), dtype=dtype, device=dev())
        _ibits(self.buf).fill_(bits)
        self.geom = ((rows, width), (ld, 1), guard)
        self.view = torch.as_strided(self.buf, *self.geom)
        assert self.view.data_ptr() % 16 == 0
        if init is not None:
            self.view.copy_(init)
        self.before = _ibits(self.buf).clone()

    def rearm(self):
        self.before = _ibits(self.buf).clone()

    def initial(self):
        """the view's content at the last (re)arm"""
        return torch.as_strided(self.before, *self.geom).view(self.buf.dtype)

    def check(self, what, written=None):
        changed = _ibits(self.buf) != self.before
        inside = torch.as_strided(changed, *self.geom)
        if written is None:
            inside.fill_(False)
        else:
            inside[written] = False
        n = int(changed.sum())
        assert n == 0, f"{what}: {n} elements outside the documented write set changed"


class ReadOnly:
    """snapshots of the inputs a kernel promises (const) not to write; check() compares them bit for bit"""

    def __init__(self, **tensors):
        self.t = tensors
        self.snap = {k: v.clone() for k, v in tensors.items()}

    def check(self, what):
        for k, v in self.t.items():
            assert bits_equal(v, self.snap[k]), f"{what}: the read-only input `{k}` was modified"


_ratios = {}


def report(family, what, ratio):
    _ratios[family] = max(_ratios.get(family, 0.0), ratio)
    print(f"REF_RATIO {family} | {what}: max err/bound {ratio:.4f}  (family max so far {_ratios[family]:.4f})")


def check_bound(got, want, bound, family, what):
    """|got - want| <= bound element by element (fp64 tensors; got must be finite)"""
    g = got.to(F64)
    assert torch.isfinite(g).all(), f"{what}: non-finite output"
    err = (g - want).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp(min=1e-300)).max().item() if err.numel() else 0.0
    report(family, what, ratio)
    if ratio > 1.0:
        i = int(torch.where(err == 0, torch.zeros_like(err), err / bound.clamp(min=1e-300)).argmax())
        raise AssertionError(f"{what}: err/bound {ratio:.4f} at flat index {i}: got {g.flatten()[i].item():.9g} want "
                             f"{want.flatten()[i].item():.9g} bound {bound.flatten()[i].item():.3e}")


def check_interval(got, a, b, family, what):
    """got lies between a and b (bf16 tensors, either order).  Used where the kernel's result is a MONOTONE function (bf16 roundings
    and exact products) of one fp32 intermediate t known to within +-delta: the result then lies between the same chain evaluated at
    t - delta and at t + delta, with no further slack.  The printed ratio is the distance to the middle of the interval over its
    half width (0 where the interval is a point and the result equals it)."""
    g, a, b = got.to(F64), a.to(F64), b.to(F64)
    assert torch.isfinite(g).all(), f"{what}: non-finite output"
    lo, hi = torch.minimum(a, b), torch.maximum(a, b)
    half, mid = (hi - lo) / 2, (hi + lo) / 2
    dist = (g - mid).abs()
    inf = torch.full_like(dist, float("inf"))
    ratio_t = torch.where(dist <= half, torch.where(half > 0, dist / half.clamp(min=1e-300), torch.zeros_like(dist)), inf)
    bad = (g < lo) | (g > hi)
    ratio = ratio_t.max().item() if ratio_t.numel() else 0.0
    flips = (hi > lo).float().mean().item() if hi.numel() else 0.0
    print(f"REF_INTERVAL {family} | {what}: {flips:.3%} of the elements may round either way")
    if bool(bad.any()):
        i = int(bad.flatten().nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} elements outside their interval; first at flat index {i}: got "
                             f"{g.flatten()[i].item():.9g} not in [{lo.flatten()[i].item():.9g}, {hi.flatten()[i].item():.9g}]")
    report(family, what, ratio)


def bf_round_int(v):
    """round-to-nearest-even of int64 values to 8 significant bits (the bf16 grid) by integer arithmetic -> (rounded, tie, above 256)"""
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
