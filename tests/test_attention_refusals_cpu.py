"""CPU: the documented refusals of the attention entry points return NV_ERR_SHAPE before any launch and leave every buffer they
were given untouched.  The buffers are host memory filled with a sentinel, so these calls are made only where no GPU is visible."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="refusal calls pass host sentinel buffers: CPU machine only")

NV_ERR_SHAPE = -2
HD = 128


@pytest.fixture(scope="module")
def L():
    import os
    from navillm_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        from navillm_amd import build
        build.build(verbose=False)
    return lib.load()


def _refused(L, name, make_args):
    """call L.name(*make_args(p)) with p = the sentinel buffer's address in every pointer slot: NV_ERR_SHAPE, nothing written"""
    buf = np.full(1 << 14, 0xA5A5A5A5, dtype=np.uint32)
    p = buf.ctypes.data
    rc = getattr(L, name)(*make_args(p))
    assert rc == NV_ERR_SHAPE, f"{name}: returned {rc}, expected NV_ERR_SHAPE"
    assert bool((buf == 0xA5A5A5A5).all()), f"{name}: wrote into a buffer while refusing"


# name, arguments (p = a pointer), what is wrong
REFUSALS = [
    ("nv_attn_fwd_bf16", lambda p: (p, p, p, p, 1, 256, 1, HD, 64, None), "q_row_min not a multiple of 128"),
    ("nv_attn_fwd_bf16", lambda p: (p, p, p, p, 1, 256, 1, HD, 256, None), "q_row_min >= S"),
    ("nv_attn_fwd_bf16", lambda p: (p, p, p, p, 1, 256, 1, HD, -128, None), "q_row_min < 0"),
    ("nv_attn_fwd_strided_bf16", lambda p: (p, p, p, p, 1, 200, 199, 1, HD, 0, None), "S_stride < S"),
    ("nv_attn_fwd_strided_bf16", lambda p: (p, p, p, p, 1, 200, 256, 1, HD, 100, None), "q_row_min not a multiple of 128"),
    ("nv_attn_fwd_strided_bf16", lambda p: (p, p, p, p, 1, 200, 256, 1, HD, 256, None), "q_row_min >= S"),
    ("nv_attn_fwd_varlen_bf16", lambda p: (p, p, p, p, p, 2, 200, 1, HD, 64, None), "q_row_min not a multiple of 128"),
    ("nv_attn_fwd_varlen_bf16", lambda p: (p, p, p, p, p, 2, 200, 1, HD, 256, None), "q_row_min >= S_max"),
    ("nv_attn_fwd_varlen_bf16", lambda p: (p, p, p, p, p, 2, 200, 1, HD, -2, None), "q_row_min < -1"),
    ("nv_attn_bwd_bf16", lambda p: (p, p, p, p, p, p, p, 1, 256, 1, HD, 64, None), "q_row_min not a multiple of 128"),
    ("nv_attn_bwd_bf16", lambda p: (p, p, p, p, p, p, p, 1, 256, 1, HD, 256, None), "q_row_min >= S"),
    ("nv_attn_bwd_rope_bf16", lambda p: (p, p, p, p, p, p, p, p, p, 1, 256, 1, HD, 384, None), "q_row_min >= S"),
    ("nv_attn_bwd_strided_bf16", lambda p: (p, p, p, p, p, p, p, 1, 200, 199, 1, HD, 0, None), "S_stride < S"),
    ("nv_attn_bwd_strided_bf16", lambda p: (p, p, p, p, p, p, p, 1, 200, 256, 1, HD, 130, None), "q_row_min not a multiple of 128"),
    ("nv_attn_bwd_strided_kvacc_bf16", lambda p: (p, p, p, p, p, p, p, p, p, 1, 1, 200, 199, 1, HD, 0, None), "S_stride < S"),
    ("nv_attn_bwd_strided_kvacc_bf16", lambda p: (p, p, p, p, p, p, p, p, p, 0, 1, 200, 256, 1, HD, 256, None), "q_row_min >= S"),
    ("nv_attn_bwd_varlen_bf16", lambda p: (p, p, p, p, p, p, p, p, None, None, 2, 200, 300, 1, HD, 64, None),
     "q_row_min not a multiple of 128"),
    ("nv_attn_bwd_varlen_bf16", lambda p: (p, p, p, p, p, p, p, p, None, None, 2, 200, 300, 1, HD, 256, None), "q_row_min >= S_max"),
    # episode backward: T, B, H, head_dim, cap, Mp, R, Lp_max, N_max
    ("nv_attn_bwd_episode_bf16", lambda p: (p, p, p, p, p, p, p, p, p, None, None, 129, 1, 1, HD, 256, 64, 200, 64, 1, None), "T > 128"),
    ("nv_attn_bwd_episode_bf16", lambda p: (p, p, p, p, p, p, p, p, p, None, None, 2, 1, 1, HD, 2048, 64, 3200, 64, 1537, None),
     "N_max > 1536"),
    ("nv_attn_bwd_episode_bf16", lambda p: (p, p, p, p, p, p, p, p, p, None, None, 2, 1, 1, HD, 256, 257, 300, 257, 10, None),
     "Lp_max > cap"),
    ("nv_attn_bwd_episode_acc_bf16", lambda p: (p, p, p, p, p, p, p, p, p, p, p, 129, 1, 1, HD, 256, 64, 200, 64, 1, 1, None), "T > 128"),
    ("nv_attn_bwd_episode_acc_bf16", lambda p: (p, p, p, p, p, p, p, p, p, None, None, 2, 1, 1, HD, 2048, 64, 3200, 64, 1537, 1, None),
     "N_max > 1536"),
    ("nv_attn_bwd_episode_acc_bf16", lambda p: (p, p, p, p, p, p, p, p, p, None, None, 2, 1, 1, HD, 256, 300, 400, 300, 10, 0, None),
     "Lp_max > cap"),
    # episode forward: T, B, H, head_dim, cap, n_max, rows
    ("nv_attn_fwd_episode_bf16", lambda p: (p, p, p, p, p, 65536, 1, 1, HD, 256, 1, 64, None), "T * ceil(n_max / 128) > 65535"),
    ("nv_attn_fwd_episode_bf16", lambda p: (p, p, p, p, p, 512, 1, 1, HD, 256, 128 * 128 + 1, 64, None), "T * ceil(n_max / 128) > 65535"),
]


@pytest.mark.parametrize("name,make_args,why", REFUSALS, ids=[f"{r[0]}-{r[2].replace(' ', '_')}" for r in REFUSALS])
def test_attention_refusal_writes_nothing(L, name, make_args, why):
    _refused(L, name, make_args)
