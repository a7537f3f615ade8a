"""Pure-Python / torch pieces of the reference tests of the fp32 encoder kernels (navillm_amd/csrc/enc_f32.hip): checked without
a GPU by test_enc_ref_cpu.py, used on the device by test_enc_kernels_ref_gpu.py.  Nothing here needs a GPU or shares code with the
kernels.

  * gemm_f32_plan mirrors the host dispatch of nv_gemm_f32_ws line for line: which of the six kernels runs (the generic
    gemm_f32_kernel in its loader orientations, gemm_f32_vec_kernel<true,true> / <true,false> / <false,false>), whether K is split,
    and the workspace extent.  GEMM_CASES is the case list of the GPU test; gemm_features() names what each case reaches and
    GEMM_REQUIRED what the list as a whole has to reach.
  * fp64 references of LayerNorm forward / backward, of the attention core forward / backward (a given 0/1 keep mask and p; P is
    returned before dropout, as the kernel stores it) and of GELU forward / backward.  They are device-agnostic torch: the CPU test
    compares them with torch's own float64 operators and autograd, the GPU test feeds them device tensors.
  * dropout_keep / mha_keep: the keep masks of nv_dropout_f32 and nv_mha_*_drop_f32 from sample_ref.philox4x32_10 (numpy).

Exactness of the GEMM cases.  Operands are integers in [-8, 8], bias and the initial C integers below 2^10: with K <= 1056 every
partial sum is an integer below 64 * 1056 + 2^11 < 2^24, exact in fp32 in any order, under any split and inside the MFMA."""
import math
from collections import namedtuple

import numpy as np
import torch

from sample_ref import philox4x32_10

F32, F64, I64 = torch.float32, torch.float64, torch.int64
FBM, FBN, FBK = 64, 64, 32
EXACT_LIMIT = 1 << 24


# ================================================================================================ GEMM: mirror of nv_gemm_f32_ws
def gemm_f32_plan(layout, M, N, K, lda, ldb, a_ptr_mod16, b_ptr_mod16, has_workspace):
    """-> dict(kernel, a_kc, b_kc, aligned, blocks, ktiles, S, ksplit, kchunk, ws_floats, a_bytes, b_bytes).  kernel is
    'refused' (NV_ERR_ARG), 'none' (NV_OK without a launch), 'vec' or 'generic'; S is the slice count aimed at (0: the split
    branch is not entered), ksplit the slices launched (1: no split), ws_floats the workspace floats written and read."""
    out = dict(kernel="refused", a_kc=None, b_kc=None, aligned=False, blocks=0, ktiles=0, S=0, ksplit=1, kchunk=K, ws_floats=0,
               a_bytes=0, b_bytes=0)
    if M < 0 or N < 0 or K < 0 or layout not in (0, 1, 2):
        return out
    if M == 0 or N == 0:
        out["kernel"] = "none"
        return out
    a_kc, b_kc = layout != 2, layout == 0
    aligned = (a_ptr_mod16 == 0 and b_ptr_mod16 == 0 and lda % 4 == 0 and ldb % 4 == 0 and
               (K % 4 == 0 if a_kc else M % 4 == 0) and (K % 4 == 0 if b_kc else N % 4 == 0))
    gx, gy = (N + FBN - 1) // FBN, (M + FBM - 1) // FBM
    blocks, ktiles = gx * gy, (K + FBK - 1) // FBK
    out.update(kernel="vec" if aligned else "generic", a_kc=a_kc, b_kc=b_kc, aligned=aligned, blocks=blocks, ktiles=ktiles)
    if not aligned:
        return out
    a_rows, a_cols = (M, K) if a_kc else (K, M)
    b_rows, b_cols = (N, K) if b_kc else (K, N)
    out["a_bytes"] = ((a_rows - 1) * lda + a_cols) * 4 if K > 0 else 0
    out["b_bytes"] = ((b_rows - 1) * ldb + b_cols) * 4 if K > 0 else 0
    if has_workspace and blocks < 512 and ktiles >= 8:
        S = min((1024 + blocks - 1) // blocks, 8, ktiles // 4)
        out["S"] = S
        if S >= 2:
            kchunk = ((ktiles + S - 1) // S) * FBK
            ksplit = (K + kchunk - 1) // kchunk
            out.update(kchunk=kchunk, ksplit=ksplit)
            if ksplit > 1:
                out["ws_floats"] = ksplit * M * N
    return out


GemmCase = namedtuple("GemmCase", "name layout M N K pa pb pc a_off b_off bias acc ws null expect")


def _gc(name, layout, M, N, K, pa=0, pb=0, pc=3, a_off=0, b_off=0, bias=True, acc=0, ws=True, null=None, expect=0):
    return GemmCase(name, layout, M, N, K, pa, pb, pc, a_off, b_off, bias, acc, ws, null, expect)


def gemm_dims(c):
    """-> (a_rows, a_cols, lda, b_rows, b_cols, ldb, ldc): layout 0 NT A[M,K] B[N,K]; 1 NN A[M,K] B[K,N]; 2 TN A[K,M] B[K,N]
    (layout 3, refused, gets the extents of layout 0)"""
    a_rows, a_cols = (c.K, c.M) if c.layout == 2 else (c.M, c.K)
    b_rows, b_cols = (c.K, c.N) if c.layout in (1, 2) else (c.N, c.K)
    return a_rows, a_cols, a_cols + c.pa, b_rows, b_cols, b_cols + c.pb, c.N + c.pc


def gemm_case_plan(c):
    _, _, lda, _, _, ldb, _ = gemm_dims(c)
    if c.null:
        return gemm_f32_plan(3, c.M, c.N, c.K, lda, ldb, 0, 0, c.ws)
    return gemm_f32_plan(c.layout, c.M, c.N, c.K, lda, ldb, (4 * c.a_off) % 16, (4 * c.b_off) % 16, c.ws)


def _gemm_cases():
    cs = []
    for L in (0, 1, 2):
        Mo = 68 if L == 2 else 65                       # layout 2 needs M % 4 == 0 on the vector path
        t = f"L{L}"
        # ---- vector kernel, no split (ktiles < 8)
        cs += [_gc(f"{t}-vec-{Mo}x132x36", L, Mo, 132, 36),
               _gc(f"{t}-vec-36x64x4", L, 36, 64, 4),
               _gc(f"{t}-vec-{Mo}x132x36-nobias-acc", L, Mo, 132, 36, bias=False, acc=1),
               _gc(f"{t}-vec-36x64x36-acc-ldc=N", L, 36, 64, 36, acc=1, pc=0),
               # padded leading dimensions, ld % 4 == 0: still the vector kernel; the pad columns hold NaN
               _gc(f"{t}-vec-{Mo}x132x36-ld+4+8", L, Mo, 132, 36, pa=4, pb=8, pc=5),
               _gc(f"{t}-vec-64x128x64-ld+8+4", L, 64, 128, 64, pa=8, pb=4, pc=1)]
        # ---- split-K
        cs += [_gc(f"{t}-split-36x64x228", L, 36, 64, 228),                              # S 2, kchunk 128, last slice 3 tiles + 4
               _gc(f"{t}-split-36x64x228-ld+4+4-acc", L, 36, 64, 228, pa=4, pb=4, acc=1),
               _gc(f"{t}-split-36x64x228-nobias", L, 36, 64, 228, bias=False),
               _gc(f"{t}-split-64x64x256-nobias-acc", L, 64, 64, 256, bias=False, acc=1),
               _gc(f"{t}-split-20x68x1024", L, 20, 68, 1024, pa=4),                      # ksplit 8, two column tiles
               _gc(f"{t}-split-12x64x1056-acc", L, 12, 64, 1056, pb=4, acc=1),           # S 8, ksplit 7
               _gc(f"{t}-nows-36x64x228", L, 36, 64, 228, ws=False),                     # null workspace: the same shape unsplit
               _gc(f"{t}-nows-36x64x228-acc", L, 36, 64, 228, ws=False, acc=1, pa=4, pb=4)]
        # ---- generic kernel: a base pointer one element off, an odd leading dimension
        cs += [_gc(f"{t}-gen-a+1-36x64x36", L, 36, 64, 36, a_off=1),
               _gc(f"{t}-gen-b+1-36x64x36", L, 36, 64, 36, b_off=1, acc=1),
               _gc(f"{t}-gen-lda+1-36x64x36", L, 36, 64, 36, pa=1, bias=False, acc=1),
               _gc(f"{t}-gen-ldb+1-36x64x36", L, 36, 64, 36, pb=1, bias=False),
               _gc(f"{t}-gen-ldb+2-{Mo}x132x228-ws", L, Mo, 132, 228, pb=2),             # a split-able shape that must not split
               _gc(f"{t}-gen-100x130x7", L, 100, 130, 7, pa=2 if L == 2 else 1, pb=3),
               _gc(f"{t}-gen-65x129x33-acc", L, 65, 129, 33, acc=1, pc=0),
               _gc(f"{t}-gen-65x129x33-nobias", L, 65, 129, 33, bias=False, pa=5, pb=7)]
        # ---- K = 0: the bias broadcast (or C + bias); M = 0 / N = 0: NV_OK, nothing written
        cs += [_gc(f"{t}-k0-8x12-bias", L, 8, 12, 0, pa=4, pb=4),
               _gc(f"{t}-k0-8x12-bias-acc", L, 8, 12, 0, pa=4, pb=4, acc=1),
               _gc(f"{t}-k0-8x12-nobias", L, 8, 12, 0, pa=4, pb=4, bias=False),
               _gc(f"{t}-k0-7x9-generic", L, 7, 9, 0, pa=3, pb=3, a_off=1),
               _gc(f"{t}-m0", L, 0, 12, 8, pa=4, pb=4),
               _gc(f"{t}-n0", L, 8, 0, 8, pa=4, pb=4)]
    # free dimension % 4 != 0 of a transposed operand: generic although K % 4 == 0
    cs += [_gc("L1-gen-N%4-36x130x8", 1, 36, 130, 8), _gc("L2-gen-M%4-65x132x8", 2, 65, 132, 8), _gc("L2-gen-N%4-68x130x8", 2, 68, 130, 8),
           # K % 4 != 0 of a K-contiguous operand (layout 2 has none: its generic cases above come from M, N, ld)
           _gc("L0-gen-K%4-36x64x38", 0, 36, 64, 38), _gc("L1-gen-K%4-36x64x38", 1, 36, 64, 38)]
    # blocks = 512: no split even with a workspace (the one case with M N above 64 K elements)
    cs += [_gc("L0-blocks512-1x32768x256", 0, 1, 32768, 256, pc=0)]
    # refusals: NV_ERR_ARG, nothing written
    cs += [_gc("layout3", 3, 8, 12, 8, expect=-1), _gc("nullA", 0, 8, 12, 8, null="A", expect=-1), _gc("nullB", 1, 8, 12, 8, null="B", expect=-1),
           _gc("nullC", 2, 8, 12, 8, null="C", expect=-1)]
    return cs


GEMM_CASES = _gemm_cases()
GEMM_BY_NAME = {c.name: c for c in GEMM_CASES}
assert len(GEMM_BY_NAME) == len(GEMM_CASES)

# the subset run with non-integer data against fp64: each vector instantiation with and without split, one generic per layout
GEMM_BOUNDED = ["L0-vec-65x132x36-ld+4+8", "L1-vec-65x132x36-ld+4+8", "L2-vec-68x132x36-ld+4+8", "L0-split-20x68x1024", "L1-split-36x64x228-ld+4+4-acc",
                "L2-split-12x64x1056-acc", "L0-gen-65x129x33-acc", "L1-gen-100x130x7", "L2-gen-65x129x33-nobias"]


def gemm_features(c):
    """what one case reaches, as strings"""
    if c.expect != 0:
        return {"refused"}
    p = gemm_case_plan(c)
    _, _, lda, _, _, ldb, _ = gemm_dims(c)
    f = set()
    if p["kernel"] == "none":
        return {"no launch"}
    kc = (int(p["a_kc"]), int(p["b_kc"]))
    if p["kernel"] == "vec":
        f.add(f"vec{kc}")
        f.add(f"vec{kc} {'split' if p['ksplit'] > 1 else 'no split'}")
        if c.pa and c.pb:
            f.add(f"vec{kc} padded ld")
        if c.M % 64 or c.N % 64:
            f.add(f"vec{kc} ragged tile")
        if c.M < 64:
            f.add(f"vec{kc} M<64")
        if c.K % 32:
            f.add(f"vec{kc} K%32")
        if p["ksplit"] > 1:
            f.add(f"split bias={int(c.bias)} acc={c.acc}")
            if p["ksplit"] < p["S"]:
                f.add("ksplit<S")
            if c.K % 32:
                f.add("partial last K tile inside a split")
            if c.pa and c.pb:
                f.add(f"vec{kc} split padded ld")
        else:
            f.add(f"unsplit bias={int(c.bias)} acc={c.acc}")
            if c.ws and p["blocks"] >= 512 and p["ktiles"] >= 8:
                f.add("blocks>=512")
            if not c.ws and p["blocks"] < 512 and p["ktiles"] >= 8:
                f.add("null workspace on a split-able shape")
        if c.K == 0:
            f.add("vec K=0")
    else:
        f.add(f"generic{kc}")
        f.add(f"generic bias={int(c.bias)} acc={c.acc}")
        if c.a_off % 4 or c.b_off % 4:
            f.add(f"generic{kc} misaligned base")
        if lda % 4 or ldb % 4:
            f.add(f"generic{kc} ld%4")
        if (c.K % 4 and (p["a_kc"] or p["b_kc"])) or (not p["a_kc"] and c.M % 4) or (not p["b_kc"] and c.N % 4):
            f.add(f"generic{kc} extent%4")
        if c.K == 0:
            f.add("generic K=0")
    return f


_KC = [(1, 1), (1, 0), (0, 0)]
GEMM_REQUIRED = ({f"vec{k}" for k in _KC} | {f"vec{k} split" for k in _KC} | {f"vec{k} no split" for k in _KC} |
                 {f"vec{k} padded ld" for k in _KC} | {f"vec{k} split padded ld" for k in _KC} | {f"vec{k} ragged tile" for k in _KC} |
                 {f"vec{k} M<64" for k in _KC} | {f"vec{k} K%32" for k in _KC} |
                 {f"generic{k}" for k in _KC} | {f"generic{k} misaligned base" for k in _KC} | {f"generic{k} ld%4" for k in _KC} |
                 {f"generic{k} extent%4" for k in _KC} |
                 {f"split bias={b} acc={a}" for b in (0, 1) for a in (0, 1)} | {f"unsplit bias={b} acc={a}" for b in (0, 1) for a in (0, 1)} |
                 {f"generic bias={b} acc={a}" for b in (0, 1) for a in (0, 1)} |
                 {"ksplit<S", "partial last K tile inside a split", "blocks>=512", "null workspace on a split-able shape", "vec K=0",
                  "generic K=0", "no launch", "refused"})


def gemm_coverage(cases):
    got = set()
    for c in cases:
        got |= gemm_features(c)
    return got


def cpu_gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k) + 41) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def rand_ints(g, lo, hi, *shape):
    """int64 in [lo, hi] (CPU generator)"""
    return torch.randint(lo, hi + 1, shape, generator=g)


def name_key(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name))


def gemm_int_operands(c):
    """-> (A, B, bias or None, C0) of the exact case as CPU int64 tensors in the storage orientation of the layout"""
    a_rows, a_cols, _, b_rows, b_cols, _, _ = gemm_dims(c)
    g = cpu_gen(name_key(c.name))
    A, B = rand_ints(g, -8, 8, a_rows, a_cols), rand_ints(g, -8, 8, b_rows, b_cols)
    bias = rand_ints(g, -1023, 1023, c.N) if c.bias else None
    return A, B, bias, rand_ints(g, -1023, 1023, c.M, c.N)


def gemm_reference(c, A, B, bias, C0):
    """C[M,N] = sum_k A(m,k) B(n,k) (+ bias[n]) (+ C0 when c.acc), in the dtype of the operands (int64 or float64)
    -> (C, sum_k |A||B| + |bias| + |C0|)"""
    At = A.t() if c.layout == 2 else A
    Bt = B if c.layout in (1, 2) else B.t()
    out, mag = At @ Bt, At.abs() @ Bt.abs()
    if bias is not None:
        out, mag = out + bias[None], mag + bias.abs()[None]
    if c.acc:
        out, mag = out + C0, mag + C0.abs()
    return out, mag


# ================================================================================================ fp64 references
def layernorm_fwd_ref(x, w, b, eps):
    """x [M, d], w, b [d] float64 -> (y, mean [M], rstd [M]); biased variance, as nn.LayerNorm"""
    mean = x.mean(dim=1)
    var = ((x - mean[:, None]) ** 2).mean(dim=1)
    rstd = 1.0 / torch.sqrt(var + eps)
    return (x - mean[:, None]) * rstd[:, None] * w[None] + b[None], mean, rstd


def layernorm_bwd_ref(dy, x, w, mean, rstd):
    """the gradient for GIVEN mean / rstd [M] (the kernel's inputs) -> (dx, gw, gb)"""
    xh = (x - mean[:, None]) * rstd[:, None]
    dxh = dy * w[None]
    s1, s2 = dxh.mean(dim=1, keepdim=True), (dxh * xh).mean(dim=1, keepdim=True)
    return rstd[:, None] * (dxh - s1 - xh * s2), (dy * xh).sum(dim=0), dy.sum(dim=0)


def split_qkv(qkv, B, N, heads, hd):
    """qkv [B*N, 3 h] (q | k | v, head hh in columns hh*hd .. hh*hd+hd of each) -> q, k, v [B, heads, N, hd]"""
    t = qkv.reshape(B, N, 3, heads, hd).permute(2, 0, 3, 1, 4)
    return t[0], t[1], t[2]


def mha_fwd_ref(qkv, lens, B, N, heads, hd, keep=None, p=0.0):
    """-> (out [B*N, h], P [B, heads, N, N] BEFORE dropout).  Keys >= lens[b] are padding (probability 0); `keep` [B,heads,N,N] 0/1
    and p: the probabilities are multiplied by keep / (1 - p) before P.V."""
    q, k, v = split_qkv(qkv, B, N, heads, hd)
    s = (q @ k.transpose(-1, -2)) / math.sqrt(hd)
    pad = torch.arange(N, device=qkv.device)[None, :] >= lens.to(qkv.device)[:, None]                  # [B, N]
    s = s.masked_fill(pad[:, None, None, :], float("-inf"))
    P = torch.softmax(s, dim=-1)
    Pm = P if keep is None or p == 0.0 else P * keep.to(P.dtype) / (1.0 - p)
    out = (Pm @ v).permute(0, 2, 1, 3).reshape(B * N, heads * hd)
    return out, P


def mha_bwd_ref(qkv, P, dout, B, N, heads, hd, keep=None, p=0.0):
    """the gradient for a GIVEN P (the kernel's input) -> dqkv [B*N, 3 h]"""
    q, k, v = split_qkv(qkv, B, N, heads, hd)
    dO = dout.reshape(B, N, heads, hd).permute(0, 2, 1, 3)
    m = torch.ones_like(P) if keep is None or p == 0.0 else keep.to(P.dtype) / (1.0 - p)
    dP = (dO @ v.transpose(-1, -2)) * m
    dS = P * (dP - (dP * P).sum(dim=-1, keepdim=True))
    scale = 1.0 / math.sqrt(hd)
    dq, dk, dv = (dS @ k) * scale, (dS.transpose(-1, -2) @ q) * scale, (P * m).transpose(-1, -2) @ dO
    return torch.stack([dq, dk, dv], dim=0).permute(1, 3, 0, 2, 4).reshape(B * N, 3 * heads * hd)


def gelu_fwd_ref(v):
    return 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))


def gelu_bwd_ref(v, dy):
    """-> (dx, cdf, pdf)"""
    cdf = 0.5 * (1.0 + torch.erf(v / math.sqrt(2.0)))
    pdf = torch.exp(-0.5 * v * v) / math.sqrt(2.0 * math.pi)
    return dy * (cdf + v * pdf), cdf, pdf


# ================================================================================================ Philox keep masks
_U64 = np.uint64
_M32 = _U64(0xFFFFFFFF)


def philox_words(seed, counter):
    """the four output words of 64-bit counters (array) under `seed`: c0 / c1 = the counter's low / high word, c2 = c3 = 0,
    key = the seed's low / high word"""
    n = np.asarray(counter, dtype=_U64)
    s = _U64(int(seed) & 0xFFFFFFFFFFFFFFFF)
    return philox4x32_10((n & _M32, n >> _U64(32), 0, 0), (s & _M32, s >> _U64(32)))


def word_u(word):
    """u = (word >> 8) * 2^-24 as fp32 (exact; no + 2^-25, unlike sample_ref.philox_u)"""
    return (np.asarray(word, dtype=_U64) >> _U64(8)).astype(np.float32) * np.float32(2.0 ** -24)


def _counters(offset, n):
    return (np.arange(n, dtype=_U64) + _U64(int(offset) & 0xFFFFFFFFFFFFFFFF))            # wraps mod 2^64, as the kernel's sum


def dropout_keep(seed, offset, n, p):
    """nv_dropout_f32: element 4 g + j uses word j of counter offset + g; keep iff float32(u) >= float32(p) -> bool [n]"""
    groups = (n + 3) // 4
    w = philox_words(seed, _counters(offset, groups))
    u = np.stack([word_u(x) for x in w], axis=1).reshape(-1)[:n]
    return u >= np.float32(p)


def mha_keep(seed, offset, B, heads, N, p):
    """nv_mha_*_drop_f32: element e = ((b heads + hh) N + a) N + c uses word 0 of counter offset + e -> bool [B, heads, N, N]"""
    w0 = philox_words(seed, _counters(offset, B * heads * N * N))[0]
    return (word_u(w0) >= np.float32(p)).reshape(B, heads, N, N)
