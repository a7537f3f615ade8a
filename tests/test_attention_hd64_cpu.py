"""CPU: the attention entry points and the decoder runtime accept head_dim 64 as well as 128, and nothing else.

As in tests/test_attention_refusals_cpu.py the buffers are host memory filled with a sentinel, so the calls are made only where no
GPU is visible: every case here returns before any launch.  An empty problem (B = 0 / S = 0 / T = 0 / M = 0, whichever the wrapper
short-circuits on) at head_dim 64 returns NV_OK and writes nothing -- the width check comes first, so a library that knows head_dim
128 only answers NV_ERR_SHAPE; the documented refusals still hold at head_dim 64; head_dim 32 / 96 / 256 are refused everywhere."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="the calls pass host sentinel buffers: CPU machine only")

NV_OK, NV_ERR_SHAPE = 0, -2


@pytest.fixture(scope="module")
def L():
    import os
    from navillm_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        from navillm_amd import build
        build.build(verbose=False)
    return lib.load()


def _call(L, name, make_args, want):
    """call L.name(*make_args(p)) with p = the sentinel buffer's address in every pointer slot: `want` returned, nothing written"""
    buf = np.full(1 << 14, 0xA5A5A5A5, dtype=np.uint32)
    rc = getattr(L, name)(*make_args(buf.ctypes.data))
    assert rc == want, f"{name}: returned {rc}, expected {want}"
    assert bool((buf == 0xA5A5A5A5).all()), f"{name}: wrote into a buffer"


# name, arguments (p = a pointer, hd = head_dim) of an EMPTY problem, which count is zero
EMPTY = [
    ("nv_attn_fwd_bf16", lambda p, hd: (p, p, p, p, 0, 256, 1, hd, 0, None), "B = 0"),
    ("nv_attn_fwd_bf16", lambda p, hd: (p, p, p, p, 2, 0, 1, hd, 0, None), "S = 0"),
    ("nv_attn_fwd_strided_bf16", lambda p, hd: (p, p, p, p, 0, 200, 256, 1, hd, 0, None), "B = 0"),
    ("nv_attn_fwd_strided_dyn_bf16", lambda p, hd: (p, p, p, p, 0, 256, 1, hd, p, None), "B = 0"),
    ("nv_attn_fwd_varlen_bf16", lambda p, hd: (p, p, p, p, p, 0, 200, 1, hd, 0, None), "B = 0"),
    ("nv_attn_fwd_varlen_bf16", lambda p, hd: (p, p, p, p, p, 2, 0, 1, hd, 0, None), "S_max = 0"),
    ("nv_attn_fwd_episode_bf16", lambda p, hd: (p, p, p, p, p, 0, 1, 1, hd, 256, 1, 64, None), "T = 0"),
    ("nv_attn_fwd_episode_bf16", lambda p, hd: (p, p, p, p, p, 2, 1, 1, hd, 256, 0, 64, None), "n_max = 0"),
    ("nv_attn_decode_bf16", lambda p, hd: (p, p, p, p, 0, 1, hd, 256, None), "M = 0"),
    ("nv_attn_bwd_bf16", lambda p, hd: (p, p, p, p, p, p, p, 0, 256, 1, hd, 0, None), "B = 0"),
    ("nv_attn_bwd_rope_bf16", lambda p, hd: (p, p, p, p, p, p, p, p, p, 0, 256, 1, hd, 0, None), "B = 0"),
    ("nv_attn_bwd_strided_bf16", lambda p, hd: (p, p, p, p, p, p, p, 0, 200, 256, 1, hd, 0, None), "B = 0"),
    ("nv_attn_bwd_strided_kvacc_bf16", lambda p, hd: (p, p, p, p, p, p, p, p, p, 1, 0, 200, 256, 1, hd, 0, None), "B = 0"),
    ("nv_attn_bwd_varlen_bf16", lambda p, hd: (p, p, p, p, p, p, p, p, None, None, 0, 200, 0, 1, hd, 0, None), "B = 0"),
    ("nv_attn_bwd_episode_bf16", lambda p, hd: (p, p, p, p, p, p, p, p, p, None, None, 0, 1, 1, hd, 256, 64, 64, 64, 0, None), "T = 0"),
    ("nv_attn_bwd_episode_acc_bf16", lambda p, hd: (p, p, p, p, p, p, p, p, p, None, None, 0, 1, 1, hd, 256, 64, 64, 64, 0, 1, None), "T = 0"),
]


@pytest.mark.parametrize("name,make_args,why", EMPTY, ids=[f"{r[0]}-{r[2].replace(' ', '')}" for r in EMPTY])
def test_empty_problem_at_head_dim_64_is_ok_and_writes_nothing(L, name, make_args, why):
    _call(L, name, lambda p: make_args(p, 64), NV_OK)


@pytest.mark.parametrize("hd", [32, 96, 256])
@pytest.mark.parametrize("name,make_args,why", EMPTY, ids=[f"{r[0]}-{r[2].replace(' ', '')}" for r in EMPTY])
def test_other_head_dims_are_refused(L, name, make_args, why, hd):
    _call(L, name, lambda p: make_args(p, hd), NV_ERR_SHAPE)


def test_documented_refusals_hold_at_head_dim_64(L):
    """the cases of tests/test_attention_refusals_cpu.py with head_dim 64 in place of 128"""
    import test_attention_refusals_cpu as R
    old = R.HD
    R.HD = 64                                   # its argument builders read the module's HD when they are called
    try:
        for name, make_args, why in R.REFUSALS:
            _call(L, name, make_args, NV_ERR_SHAPE)
    finally:
        R.HD = old


def test_hfround_instrument_stays_128_only(L):
    _call(L, "nv_attn_fwd_hfround_bf16", lambda p: (p, p, p, p, None, 0, 256, 1, 64, 0, None), NV_ERR_SHAPE)
    _call(L, "nv_attn_fwd_hfround_bf16", lambda p: (p, p, p, p, None, 0, 256, 1, 128, 0, None), NV_OK)


def test_decoder_create_accepts_64_and_128_wide_heads(L):
    """nv_decoder_create allocates a host object only (no device call), so it can be exercised here"""
    for d, H, hd, want in ((768, 12, 64, True), (256, 2, 128, True), (768, 8, 96, False), (768, 12, 128, False), (768, 24, 32, False)):
        h = L.nv_decoder_create(2, d, H, hd, 3072, ctypes.c_float(1e-6))
        assert bool(h) == want, (d, H, hd, h)
        if h:
            L.nv_decoder_destroy(h)
