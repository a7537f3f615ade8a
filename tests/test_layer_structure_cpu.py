"""CPU: the decoder layer's launch sequence is written once (navillm_amd/layer.py) -- a text check that no second copy
has grown back in the Python layer."""
import glob
import os
import re

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "navillm_amd")


def _hits(pattern):
    """{file name: number of matches} over navillm_amd/*.py without the op wrappers themselves (ops.py, fp8.py)"""
    out = {}
    for path in sorted(glob.glob(os.path.join(PKG, "*.py"))):
        name = os.path.basename(path)
        if name in ("ops.py", "fp8.py"):
            continue
        n = len(re.findall(pattern, open(path).read()))
        if n:
            out[name] = n
    return out


def test_layer_sequence_has_one_home():
    assert _hits(r"ops\.swiglu_fwd\(") == {"layer.py": 1}
    assert _hits(r"ops\.swiglu_bwd\(") == {"layer.py": 1}
    assert _hits(r"EPI_SWIGLU_BWD") == {"layer.py": 1}                 # the fused alternative sits next to it
    assert _hits(r"EPI_RESID") == {"layer.py": 2}                      # o_proj + residual, down + residual; lm_linear only forwards `epilogue`
    # no positional unpack of a layer's twelve operands: callers read fields of FlatStore.layer(i)
    assert _hits(r"Wqkv, Wo, Wgu, Wd, w1, w2") == {}
