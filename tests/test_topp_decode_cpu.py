"""CPU: the fp64 reference of nucleus (top-p) sampling (tests/topp_ref.py) against a literal restatement of HF's TopPLogitsWarper, its
tie rule, top_p = 1, the share of ambiguous cases among the cases tests/test_topp_decode_gpu.py runs, the torch restatement the host
loop uses, and the ValueErrors of `KVCacheLM.generate` as far as they can be reached without a device."""
import os
import re

import numpy as np
import pytest
import torch

import topp_ref as R
from sample_ref import sample_reference


def _hf_scores(x, ids, T, top_k):
    """what HF hands its top-p warper: logits / T with everything but the top-k survivors among `ids` at -inf"""
    keep = sample_reference(x, ids, T, top_k, 0.5)["ids"]
    s = np.full(x.shape, -np.inf)
    s[keep] = x[keep] / T
    return s


def test_reference_equals_hf_warper_on_tie_free_rows():
    """fp64 randn rows have no two equal logits, so HF's sort order decides nothing: the kept sets are equal"""
    rng = np.random.RandomState(0)
    V = 777
    ids = [v for v in range(V) if not 700 <= v < 705]
    sizes = set()
    for T in (0.3, 1.0, 4.0):
        for top_k in (0, 1, 50):
            for top_p in (1e-6, 0.1, 0.5, 0.9, 0.999):
                x = rng.randn(V) * 2
                x[3] = -np.inf
                ref = R.topp_reference(x, ids, T, top_k, top_p, 0.5)
                assert ref["ids"].tolist() == np.flatnonzero(R.hf_top_p_keep(_hf_scores(x, ids, T, top_k), top_p)).tolist(), (T, top_k, top_p)
                assert ref["kept"] == ref["ids"].size and abs(ref["hi"][-1] - 1.0) < 1e-12 and ref["lo"][0] == 0.0
                sizes.add(ref["kept"])
    assert 1 in sizes and max(sizes) > 300


def test_reference_differs_from_hf_only_inside_the_boundary_tie():
    """over the bf16 cases of the GPU test (ties everywhere): HF keeps a subset, and what it drops of the reference's set shares the
    reference's smallest kept logit -- the tie at the boundary, which HF cuts by sort order and the rule keeps whole"""
    shape = R.SHAPES[0]
    B, V, ldl, sp0 = shape
    lg, fin = R.planted_rows(*shape)
    ids = R.candidates(V, sp0)
    cut = 0
    for T, top_k, top_p in R.kernel_cases(shape):
        for b in range(B):
            ref = R.case_reference(shape, b, T, top_k, top_p)
            if fin[b] or ref["token"] is None:
                continue
            x = lg[b].double().numpy()
            hf = set(np.flatnonzero(R.hf_top_p_keep(_hf_scores(x, ids, T, top_k), top_p)).tolist())
            ours = set(ref["ids"].tolist())
            assert hf <= ours, (b, T, top_k, top_p)
            assert all(x[v] == x[ref["ids"]].min() for v in ours - hf), (b, T, top_k, top_p)
            cut += bool(ours - hf)
    assert cut > 0


def test_the_planted_rows_are_what_their_description_says():
    shape = R.SHAPES[0]
    lg, _ = R.planted_rows(*shape)
    x = lg.double().numpy()
    ref = lambda b, T, k, p: R.case_reference(shape, b, T, k, p)
    # a nucleus of exactly the top token
    assert all(ref(0, T, k, p)["ids"].tolist() == [R.TOP] for T in (0.01, 1.0) for k in R.TOPKS for p in R.TOPPS)
    # the three-way tie at the boundary: kept whole, in front of the top token; HF would keep only one of the three
    r = ref(1, 1.0, 0, 0.5)
    assert r["ids"].tolist() == sorted(R.TIE3) + [R.TOP] and r["kept"] == 4
    hf = R.hf_top_p_keep(_hf_scores(x[1], R.candidates(shape[1], shape[3]), 1.0, 0), 0.5)
    assert hf.sum() == 2 and hf[R.TOP]
    W = 1 + 3 * np.exp(-1.0)
    assert 1.0 < 0.5 * W < 1.0 + np.exp(-1.0)                            # S(tie) < limit < S(tie) + one of the three
    # the tie at the maximum, whatever top_p
    assert all(ref(2, T, k, 1e-6)["ids"].tolist() == [7, 300, shape[1] - 20] for T in R.TEMPS for k in R.TOPKS)
    # top-p cutting inside the top-k set / the top-k set smaller than the nucleus
    lad = R.ladder_ids()
    assert ref(5, 1.0, 50, 0.5)["ids"].tolist() == lad[:6] and ref(5, 1.0, 50, 0.999)["ids"].tolist() == lad[:47]
    assert all(ref(5, 100.0, 50, p)["ids"].tolist() == lad[:50] for p in (0.999,)) and ref(5, 100.0, 50, 0.9)["kept"] < 50
    # ... whose boundary shares the high byte of the bf16 pattern (sign + 7 exponent bits) with the top-k threshold
    hi = lambda v: int(torch.tensor(v, dtype=torch.bfloat16).view(torch.int16)) >> 8
    assert x[5][lad[46]] == 2.75 and x[5][lad[49]] == 2.375 and hi(2.75) == hi(2.375)
    # a boundary among negative logits
    r = ref(6, 100.0, 0, 0.9)
    assert x[6][r["ids"]].min() < 0 and 100 < r["kept"] < 1000
    # NaN / -inf / all -inf
    assert 11 not in ref(6, 100.0, 0, 0.999)["ids"] and 12 not in ref(6, 100.0, 0, 0.999)["ids"]
    assert ref(4, 1.0, 0, 0.5)["token"] is None and ref(4, 1.0, 0, 0.5)["kept"] == 0


def test_top_p_one_is_the_plain_sampled_reference():
    shape = R.SHAPES[0]
    lg, _ = R.planted_rows(*shape)
    ids = R.candidates(shape[1], shape[3])
    for b in (1, 5, 6):
        for top_p in (1.0, None):
            a = R.topp_reference(lg[b].double().numpy(), ids, 0.7, 50, top_p, 0.3)
            w = sample_reference(lg[b].double().numpy(), ids, 0.7, 50, 0.3)
            assert a["token"] == w["token"] and a["ids"].tolist() == w["ids"].tolist() and a["kept"] == w["ids"].size
            assert np.array_equal(a["lo"], w["lo"]) and np.array_equal(a["hi"], w["hi"]) and not a["ambiguous"]


def test_the_ambiguous_flag_and_both_sides_of_the_band():
    """four candidates of weights 1, 1, 1, 1 (T = 1): top_p = 0.5 puts the limit exactly on S of the third -> ambiguous, the two
    alternatives keep 2 and 3; top_p = 0.6 is far from every S"""
    x = np.array([3.0, 2.0, 1.0, 0.0]) * 0 + np.array([0.0, -1e-3, -2e-3, -3e-3])
    r = R.topp_reference(x, range(4), 1000.0, 0, 0.5, 0.5)              # weights 1, e^-1e-6, ...: S / W = 0, .25, .5, .75 within 2e-6
    assert r["ambiguous"] and sorted(a["kept"] for a in r["alt"]) == [2, 3] and r["kept"] in (2, 3)
    r = R.topp_reference(x, range(4), 1000.0, 0, 0.6, 0.5)
    assert not r["ambiguous"] and r["alt"] == () and r["ids"].tolist() == [0, 1, 2]


def test_no_case_of_the_gpu_test_is_ambiguous():
    """the GPU test accepts either decision in an ambiguous case and caps their share at 2 %; with these seeds there is none"""
    n = amb = 0
    for key, ref in R.all_references():
        n += 1
        amb += bool(ref["ambiguous"])
    assert n > 700 and amb == 0, (n, amb)


def test_host_loop_warper_follows_the_rule():
    """kvcache._top_p_warp (fp32 torch, what the host loop applies after top-k) keeps the reference's set"""
    from navillm_amd.kvcache import _top_p_warp
    shape = R.SHAPES[0]
    B, V, ldl, sp0 = shape
    lg, fin = R.planted_rows(*shape)
    rows = [b for b in range(B) if not fin[b] and b != 4]                 # (an all -inf row is NaN after HF's softmax)
    x = lg[rows, :V].float()
    x[:, sp0:sp0 + R.NSPECIAL] = float("-inf")
    x[x.isnan()] = float("-inf")                                        # the host loop has no NaN rule of its own
    for T in (1.0, 100.0):
        for top_p in R.TOPPS:
            out = _top_p_warp(x / T, top_p)
            for j, b in enumerate(rows):
                want = R.case_reference(shape, b, T, 0, top_p)["ids"].tolist()
                assert torch.isfinite(out[j]).nonzero().view(-1).tolist() == want, (b, T, top_p)
                assert torch.equal(out[j][want], (x / T)[j][want])


def test_generate_refuses_a_bad_top_p_before_any_work():
    """the check is generate()'s first act: it is reached on an object that has no buffers, no model and no device at all.  With
    do_sample=False the same values pass it (the call then fails on the missing attributes instead)."""
    from navillm_amd.kvcache import KVCacheLM
    kv = object.__new__(KVCacheLM)
    for bad in (0, 0.0, -0.1, 1.5, float("nan"), float("inf"), "0.9", True, 1 + 0j, [0.5]):
        with pytest.raises(ValueError, match="top_p"):
            KVCacheLM.generate(kv, [[1, 5]], do_sample=True, top_p=bad)
        with pytest.raises(AttributeError):
            KVCacheLM.generate(kv, [[1, 5]], do_sample=False, top_p=bad)
    for good in (None, 1.0, 1, 0.9, 1e-6, np.float32(0.5)):
        with pytest.raises(AttributeError):                            # past the check
            KVCacheLM.generate(kv, [[1, 5]], do_sample=True, top_p=good)


def test_topp_header_binding_and_library_agree():
    """include/navillm_hip_topp.h <-> lib.TOPP_SIGNATURES <-> the built .so, symbol for symbol; the main header and table do not
    know the two names; argument errors of both entries return before any launch"""
    from navillm_amd import lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "navillm_hip_topp.h")).read()
    declared = set(re.findall(r"\b(nv_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(lib.TOPP_SIGNATURES) == {"nv_decode_pick_sample_topp_bf16", "nv_decoder_sample_topp_step"}
    assert not declared & set(lib.SIGNATURES)
    assert len(lib.TOPP_SIGNATURES["nv_decode_pick_sample_topp_bf16"][1]) == 23 and len(lib.TOPP_SIGNATURES["nv_decoder_sample_topp_step"][1]) == 32
    L = lib.load()                                    # binds both tables: raises when the library does not export a name
    one = 1 << 12                                     # (any non-null pointer value will do: nothing is launched)
    args = dict(logits=one, ldl=1024, V=1006, special0=1000, nspecial=5, off=None, tok=None, nxt=None, n_nodes=0, node=None, temperature=0.7,
                top_k=50, top_p=0.9, rng=one, u_out=None, kept_out=None, state=one, out=one, max_steps=4, B=7, eos=2, pad=0, stream=None)
    bad = [("top_p", v) for v in (0.0, -0.1, 1.5, float("nan"), float("inf"))] + [("temperature", 0.0), ("top_k", -1), ("rng", None), ("ldl", 1000)]
    for k, v in bad:
        assert L.nv_decode_pick_sample_topp_bf16(*dict(args, **{k: v}).values()) == -1, (k, v)
    assert L.nv_decode_pick_sample_topp_bf16(*dict(args, V=(1 << 23) + 1, ldl=(1 << 23) + 8).values()) == -1      # the 64-bit masses
    assert L.nv_decoder_sample_topp_step(*([None] * 4), 0, 0, 0, 0, None, None, None, 0, None, 1.0, 0, 0.9, None, None, None, None, None, 0, None,
                                         None, None, 0, 0, 0, 0, None, 0, None) == -1
