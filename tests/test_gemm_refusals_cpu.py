"""CPU: the documented refusals of the bf16 GEMM entry points (nv_gemm_bf16, nv_gemm_bf16_ws, nv_gemm_bf16_rope_cfg, nv_gemm_fp8w)
return their documented code (NV_ERR_ARG / NV_ERR_SHAPE, include/navillm_hip.h) before any launch and leave every buffer they were
given untouched; M == 0 or N == 0 returns NV_OK and touches nothing.  The buffers are host memory filled with a sentinel, so these
calls are made only where no GPU is visible.  Only calls that return before a launch are listed."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="refusal calls pass host sentinel buffers: CPU machine only")

NV_OK, NV_ERR_ARG, NV_ERR_SHAPE = 0, -1, -2
STORE, ACCUM, RESID, BIAS, SWIGLU_BWD, ROPE = 0, 1, 2, 3, 4, 5
NT, NN, TN = 0, 1, 2


@pytest.fixture(scope="module")
def L():
    import os
    from navillm_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        from navillm_amd import build
        build.build(verbose=False)
    return lib.load()


def ws(p, layout=NT, A=0, B=0, C=0, R=0, M=64, N=64, K=64, lda=64, ldb=64, ldc=64, ldr=64, epi=STORE, tile=0, w=0):
    """arguments of nv_gemm_bf16_ws: a valid 64 x 64 x 64 call on the buffer at p except for what the case overrides (pointers are
    given as byte offsets from p; None = NULL)"""
    ptr = lambda o: None if o is None else p + o
    return (layout, ptr(A), ptr(B), ptr(C), ptr(R), M, N, K, lda, ldb, ldc, ldr, epi, tile, ptr(w) if w else None, None)


def plain(p, **kw):
    a = ws(p, **kw)
    return a[:14] + (None,)                 # nv_gemm_bf16: no workspace argument


def rope(p, A=0, W=0, C=0, cos=0, sin=0, pos=None, M=64, N=256, K=64, lda=64, ldw=64, ldc=256, S=16, cols=128, tile=0):
    ptr = lambda o: None if o is None else p + o
    return (ptr(A), ptr(W), ptr(C), ptr(cos), ptr(sin), ptr(pos), M, N, K, lda, ldw, ldc, S, cols, tile, None, None)


def fp8(p, A=0, Q=0, s=0, C=0, R=0, M=64, N=256, K=64, lda=64, ldq=64, ldc=256, ldr=256, epi=STORE, mode=7, tile=84):
    ptr = lambda o: None if o is None else p + o
    return (ptr(A), ptr(Q), ptr(s), ptr(C), ptr(R), M, N, K, lda, ldq, ldc, ldr, epi, mode, tile, None, None)


BIG = 70000          # 69999 rows of 32768 elements: 4.59e9 bytes from the base, past the 32-bit span of a buffer descriptor

# entry point, arguments (p = the sentinel buffer's 64-byte aligned address), documented return code, what is wrong
CASES = [
    ("nv_gemm_bf16_ws", lambda p: ws(p, layout=NT, K=96), NV_ERR_SHAPE, "NT K % 64"),
    ("nv_gemm_bf16_ws", lambda p: ws(p, layout=NN, K=32), NV_ERR_SHAPE, "NN K % 64"),
    ("nv_gemm_bf16", lambda p: plain(p, layout=NT, K=100), NV_ERR_SHAPE, "NT K % 64 (no workspace)"),
    ("nv_gemm_bf16_ws", lambda p: ws(p, lda=68), NV_ERR_SHAPE, "lda % 8"),
    ("nv_gemm_bf16_ws", lambda p: ws(p, layout=NN, ldb=65), NV_ERR_SHAPE, "ldb % 8"),
    ("nv_gemm_bf16_ws", lambda p: ws(p, layout=TN, K=7, lda=66), NV_ERR_SHAPE, "TN lda % 8"),
    ("nv_gemm_bf16_ws", lambda p: ws(p, A=2), NV_ERR_SHAPE, "A off 16 B"),
    ("nv_gemm_bf16_ws", lambda p: ws(p, B=8), NV_ERR_SHAPE, "B off 16 B"),
    ("nv_gemm_bf16_ws", lambda p: ws(p, M=-1), NV_ERR_ARG, "M < 0"),
    ("nv_gemm_bf16_ws", lambda p: ws(p, N=-5), NV_ERR_ARG, "N < 0"),
    ("nv_gemm_bf16_ws", lambda p: ws(p, K=-64), NV_ERR_ARG, "K < 0"),
    ("nv_gemm_bf16_ws", lambda p: ws(p, A=None), NV_ERR_ARG, "A NULL"),
    ("nv_gemm_bf16_ws", lambda p: ws(p, B=None), NV_ERR_ARG, "B NULL"),
    ("nv_gemm_bf16_ws", lambda p: ws(p, C=None), NV_ERR_ARG, "C NULL"),
    ("nv_gemm_bf16_ws", lambda p: ws(p, layout=3), NV_ERR_ARG, "layout 3"),
    ("nv_gemm_bf16_ws", lambda p: ws(p, layout=-1), NV_ERR_ARG, "layout -1"),
    ("nv_gemm_bf16_ws", lambda p: ws(p, tile=2), NV_ERR_ARG, "tile_cfg 2"),
    ("nv_gemm_bf16_ws", lambda p: ws(p, tile=83), NV_ERR_ARG, "tile_cfg 83"),
    ("nv_gemm_bf16_ws", lambda p: ws(p, layout=TN, tile=89), NV_ERR_ARG, "tile_cfg 89"),
    ("nv_gemm_bf16_ws", lambda p: ws(p, layout=NN, tile=96), NV_ERR_ARG, "tile_cfg 96"),
    ("nv_gemm_bf16_ws", lambda p: ws(p, epi=6), NV_ERR_ARG, "epilogue 6"),
    ("nv_gemm_bf16_ws", lambda p: ws(p, epi=-1), NV_ERR_ARG, "epilogue -1"),
    ("nv_gemm_bf16_ws", lambda p: ws(p, epi=ROPE), NV_ERR_ARG, "EPI_ROPE through nv_gemm_bf16_ws"),
    ("nv_gemm_bf16", lambda p: plain(p, epi=ROPE), NV_ERR_ARG, "EPI_ROPE through nv_gemm_bf16"),
    ("nv_gemm_bf16_ws", lambda p: ws(p, layout=NN, epi=ROPE), NV_ERR_ARG, "EPI_ROPE on NN"),
    ("nv_gemm_bf16_ws", lambda p: ws(p, layout=TN, epi=ROPE), NV_ERR_ARG, "EPI_ROPE on TN"),
    ("nv_gemm_bf16_ws", lambda p: ws(p, layout=NT, epi=SWIGLU_BWD), NV_ERR_ARG, "EPI_SWIGLU_BWD on NT"),
    ("nv_gemm_bf16_ws", lambda p: ws(p, layout=TN, epi=SWIGLU_BWD), NV_ERR_ARG, "EPI_SWIGLU_BWD on TN"),
    ("nv_gemm_bf16_ws", lambda p: ws(p, epi=RESID, R=None), NV_ERR_ARG, "EPI_RESID R NULL"),
    ("nv_gemm_bf16_ws", lambda p: ws(p, epi=BIAS, R=None), NV_ERR_ARG, "EPI_BIAS R NULL"),
    ("nv_gemm_bf16_ws", lambda p: ws(p, layout=NN, epi=SWIGLU_BWD, R=None), NV_ERR_ARG, "EPI_SWIGLU_BWD R NULL"),
    ("nv_gemm_bf16_rope_cfg", lambda p: rope(p, cos=None), NV_ERR_ARG, "EPI_ROPE cos table NULL"),
    ("nv_gemm_bf16_rope_cfg", lambda p: rope(p, sin=None), NV_ERR_ARG, "sin table NULL"),
    ("nv_gemm_bf16_rope_cfg", lambda p: rope(p, S=0), NV_ERR_ARG, "pos NULL and S 0"),
    ("nv_gemm_bf16_rope_cfg", lambda p: rope(p, cols=64), NV_ERR_ARG, "rope_cols % 128"),
    ("nv_gemm_bf16_rope_cfg", lambda p: rope(p, cols=512), NV_ERR_ARG, "rope_cols > N"),
    ("nv_gemm_bf16_rope_cfg", lambda p: rope(p, cols=-128), NV_ERR_ARG, "rope_cols < 0"),
    ("nv_gemm_bf16_rope_cfg", lambda p: rope(p, N=260, ldc=264), NV_ERR_SHAPE, "rope N % 8"),
    ("nv_gemm_bf16_rope_cfg", lambda p: rope(p, ldc=260), NV_ERR_SHAPE, "rope ldc % 8"),
    ("nv_gemm_bf16_rope_cfg", lambda p: rope(p, C=2), NV_ERR_SHAPE, "rope C off 16 B"),
    ("nv_gemm_bf16_rope_cfg", lambda p: rope(p, K=96), NV_ERR_SHAPE, "rope K % 64"),
    ("nv_gemm_bf16_rope_cfg", lambda p: rope(p, tile=7), NV_ERR_ARG, "rope tile_cfg 7"),
    ("nv_gemm_fp8w", lambda p: fp8(p, K=96), NV_ERR_SHAPE, "fp8 K % 64"),
    ("nv_gemm_fp8w", lambda p: fp8(p, ldq=72), NV_ERR_SHAPE, "fp8 ldq % 16"),
    ("nv_gemm_fp8w", lambda p: fp8(p, lda=68), NV_ERR_SHAPE, "fp8 lda % 8"),
    ("nv_gemm_fp8w", lambda p: fp8(p, s=4), NV_ERR_SHAPE, "fp8 scales off 16 B"),
    ("nv_gemm_fp8w", lambda p: fp8(p, Q=8), NV_ERR_SHAPE, "fp8 codes off 16 B"),
    ("nv_gemm_fp8w", lambda p: fp8(p, mode=6), NV_ERR_ARG, "fp8 mode 6"),
    ("nv_gemm_fp8w", lambda p: fp8(p, mode=10), NV_ERR_ARG, "fp8 mode 10"),
    ("nv_gemm_fp8w", lambda p: fp8(p, epi=ACCUM), NV_ERR_ARG, "fp8 epilogue 1"),
    ("nv_gemm_fp8w", lambda p: fp8(p, epi=BIAS), NV_ERR_ARG, "fp8 epilogue 3"),
    ("nv_gemm_fp8w", lambda p: fp8(p, epi=RESID, R=None), NV_ERR_ARG, "fp8 EPI_RESID R NULL"),
    ("nv_gemm_fp8w", lambda p: fp8(p, tile=8), NV_ERR_ARG, "fp8 tile_cfg 8"),
    ("nv_gemm_fp8w", lambda p: fp8(p, K=0), NV_ERR_ARG, "fp8 K 0"),
    ("nv_gemm_fp8w", lambda p: fp8(p, s=None), NV_ERR_ARG, "fp8 scales NULL"),
    # operand spans above 4 GiB: the sizes alone decide, nothing is read
    ("nv_gemm_bf16_ws", lambda p: ws(p, layout=NT, M=BIG, lda=32768, tile=8), NV_ERR_SHAPE, "NT A spans over 4 GiB"),
    ("nv_gemm_bf16_ws", lambda p: ws(p, layout=NT, N=BIG, ldb=32768, tile=1), NV_ERR_SHAPE, "NT B spans over 4 GiB"),
    ("nv_gemm_bf16_ws", lambda p: ws(p, layout=NN, M=BIG, lda=32768, tile=84), NV_ERR_SHAPE, "NN A spans over 4 GiB"),
    ("nv_gemm_bf16_ws", lambda p: ws(p, layout=NN, K=BIG // 64 * 64 + 64, lda=BIG // 64 * 64 + 64, ldb=32768), NV_ERR_SHAPE,
     "NN B spans over 4 GiB"),
    ("nv_gemm_bf16_ws", lambda p: ws(p, layout=TN, K=BIG, lda=32768), NV_ERR_SHAPE, "TN A spans over 4 GiB"),
    ("nv_gemm_bf16", lambda p: plain(p, layout=TN, K=BIG, ldb=32768), NV_ERR_SHAPE, "TN B spans over 4 GiB"),
    ("nv_gemm_bf16_rope_cfg", lambda p: rope(p, M=BIG, lda=32768, tile=8), NV_ERR_SHAPE, "rope A spans over 4 GiB"),
    ("nv_gemm_fp8w", lambda p: fp8(p, M=BIG, lda=32768), NV_ERR_SHAPE, "fp8 A spans over 4 GiB"),
    ("nv_gemm_fp8w", lambda p: fp8(p, N=BIG, ldq=65536, ldc=BIG + 2), NV_ERR_SHAPE, "fp8 codes span over 4 GiB"),
    # nothing to do
    ("nv_gemm_bf16_ws", lambda p: ws(p, M=0), NV_OK, "M 0"),
    ("nv_gemm_bf16_ws", lambda p: ws(p, layout=TN, N=0, epi=ACCUM), NV_OK, "N 0"),
    ("nv_gemm_bf16", lambda p: plain(p, layout=NN, M=0, N=0, K=0), NV_OK, "M 0 and N 0"),
    ("nv_gemm_bf16_rope_cfg", lambda p: rope(p, M=0), NV_OK, "rope M 0"),
    ("nv_gemm_fp8w", lambda p: fp8(p, M=0), NV_OK, "fp8 M 0"),
    ("nv_gemm_fp8w", lambda p: fp8(p, N=0), NV_OK, "fp8 N 0"),
]


@pytest.mark.parametrize("name,make_args,code,why", CASES, ids=[f"{c[0]}-{c[3].replace(' ', '_')}" for c in CASES])
def test_gemm_refusal_returns_documented_code_and_writes_nothing(L, name, make_args, code, why):
    buf = np.full((1 << 14) + 16, 0xA5A5A5A5, dtype=np.uint32)
    p = (buf.ctypes.data + 63) & ~63
    rc = getattr(L, name)(*make_args(p))
    assert rc == code, f"{name} ({why}): returned {rc}, expected {code}"
    assert bool((buf == 0xA5A5A5A5).all()), f"{name} ({why}): wrote into a buffer"
