"""CPU: the numpy reference of the repetition penalty (tests/procs_ref.py) against torch over every bf16 pattern, the C ABI of the
processors (header <-> lib.PROC_SIGNATURES <-> the built library, refusals before any launch), the ValueErrors of
`KVCacheLM.generate`, the symbols a processor-free call takes, and the inputs of tests/test_procs_decode_gpu.py."""
import inspect
import os
import re
import types

import numpy as np
import pytest
import torch

import procs_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_penalty_rule_over_every_bf16_pattern():
    """procs_ref.penalise_bits == torch.where(s < 0, s.float() * p32, s.float() / p32).to(bfloat16) on all 65 536 patterns: bit for
    bit on the 65 282 that are no NaN; a NaN comes out as a NaN on both sides (WHICH NaN torch's fp32 -> bf16 conversion writes depends
    on whether its vectorised or its scalar loop converts the element -- 0xFFFF or 0x7FC0 -- so no payload is compared; no pick reads
    one).  -inf stays -inf, the sign never flips.  torch's DIRECT bf16
    evaluation, torch.where(s < 0, s * p, s / p) on the bf16 tensor, is compared as well: it agrees on every non-NaN pattern for
    these penalties (it rounds p to fp32 like the rule and computes in fp32), which is asserted."""
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    s = torch.from_numpy(bits.view(np.int16).copy()).view(torch.bfloat16)
    nan = np.isnan(P.bf16_value(bits))
    assert nan.sum() == 2 * 127
    for p in (0.8, 1.2, 1.5, 2.0):
        p32 = float(np.float32(p))
        got = P.penalise_bits(bits, p)
        want = torch.where(s < 0, s.float() * p32, s.float() / p32).to(torch.bfloat16)
        want = want.view(torch.int16).numpy().view(np.uint16)
        assert got[~nan].tolist() == want[~nan].tolist(), p
        assert np.isnan(P.bf16_value(got)).tolist() == nan.tolist() == np.isnan(P.bf16_value(want)).tolist()
        assert got[0xFF80] == 0xFF80 and got[0x7F80] == 0x7F80               # -inf and +inf stay
        assert ((got >> 15) == (bits >> 15))[~nan].all()
        direct = torch.where(s < 0, s * p, s / p).view(torch.int16).numpy().view(np.uint16)
        differ = np.flatnonzero((direct != got) & ~nan)
        print(f"penalty {p}: the direct bf16 evaluation differs on {differ.size} non-NaN patterns", [hex(int(b)) for b in bits[differ][:8]])
        assert differ.size == 0, p


def test_seen_sets_bitmaps_and_the_eos_rule():
    seen = P.seen_sets([[1, 5, 5, 40], [1, 33]])
    P.seen_update(seen, [7, 0], [True, False])
    assert seen == [{1, 5, 40, 7}, {1, 33}]
    bm = P.bitmap(seen, 37, 3)
    assert bm.tolist() == [[(1 << 1) | (1 << 5) | (1 << 7), 0, 0], [1 << 1, 1 << 1, 0]]          # (40 >= V is left out)
    from navillm_amd.kvcache import _seen_bitmap
    assert _seen_bitmap([[1, 5, 5, 40], [1, 33]], 37).tolist() == P.bitmap(P.seen_sets([[1, 5, 5, 40], [1, 33]]), 37, 2).tolist()
    assert 2 not in P.candidates(37, 33, 2, 2, 3, 4) and 2 in P.candidates(37, 33, 2, 2, 4, 4) and 33 not in P.candidates(37, 33, 2, 2, 4, 4)


def test_the_kernel_cases_are_what_their_descriptions_say():
    """from the reference alone: the penalty changes every winner it is said to change, and no sampled case has a nucleus boundary
    within 1e-5 (relative to the total weight W) of top_p * W"""
    for shape in P.SHAPES:
        B, V, ldl = shape
        sp0, f = P.special0(V), P.far_id(V)
        ids = P.candidates(V, sp0, P.NSPECIAL, P.EOS, 0, 0)
        rows, seen = P.greedy_case(shape)
        assert [P.greedy_reference(rows[b], ids, set(), 1.0, V) for b in range(B)] == [f, 3, 5]
        assert [P.greedy_reference(rows[b], ids, seen[b], P.PENALTY, V) for b in range(B)] == [3, f, 5]
        x = P.processed_row(rows[2], seen[2], P.PENALTY, V)
        assert x[5] == x[f] == 4.0 and f > 5
        rows, seen = P.min_new_case(shape)
        assert [P.greedy_reference(rows[b], P.candidates(V, sp0, P.NSPECIAL, P.EOS, 3, 4), seen[b], 1.0, V) for b in range(B)] == [f] * B
        assert [P.greedy_reference(rows[b], P.candidates(V, sp0, P.NSPECIAL, P.EOS, 4, 4), seen[b], 1.0, V) for b in range(B)] == [P.EOS] * B
        rows, seen = P.trie_case(shape)
        kids = [w[0] for w in P.TRIE_WORDS]
        assert [P.greedy_reference(rows[b], kids, set(), 1.0, V) for b in range(B)] == [9, 9, 9]
        assert [P.greedy_reference(rows[b], kids, seen[b], P.PENALTY, V) for b in range(B)] == [3, 17, 9]
        rows, seen = P.sample_case(shape)
        kept = set()
        for T, top_k, top_p in P.SAMPLE_SETTINGS:
            for cnt in P.SAMPLE_CNTS:
                ids = P.candidates(V, sp0, P.NSPECIAL, P.EOS, cnt, P.SAMPLE_MIN_NEW)
                for b in range(B):
                    ref = P.sampled_reference(rows[b], ids, seen[b], P.SAMPLE_PENALTY, V, T, top_k, top_p, 0.5)
                    plain = P.sampled_reference(rows[b], ids, set(), 1.0, V, T, top_k, top_p, 0.5)
                    assert not ref["ambiguous"], (shape, T, top_k, top_p, cnt, b)
                    assert cnt >= P.SAMPLE_MIN_NEW or P.EOS not in ref["ids"]
                    kept.add((b, ref["kept"], ref["ids"].tolist() != plain["ids"].tolist() or not np.array_equal(ref["w"], plain["w"])))
        # the two largest planted ids of rows 0 and 1 are seen: the penalty changes the survivors or their weights in every setting
        assert all(changed for b, _, changed in kept if b < 2) and any(changed for b, _, changed in kept if b == 2)
        assert len({k for _, k, _ in kept}) > 3


def test_procs_header_binding_and_library_agree():
    """include/navillm_hip_procs.h <-> lib.PROC_SIGNATURES <-> the built .so, symbol for symbol; the three earlier tables are disjoint
    from it and keep their sizes; every argument error of the two entries returns before any launch (no device is touched here)"""
    from navillm_amd import lib
    hdr = open(os.path.join(ROOT, "include", "navillm_hip_procs.h")).read()
    declared = set(re.findall(r"\b(nv_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(lib.PROC_SIGNATURES) == {"nv_decode_pick_proc_bf16", "nv_decoder_proc_step"}
    for table, size in ((lib.SIGNATURES, 119), (lib.TOPP_SIGNATURES, 2), (lib.OPTIM_SIGNATURES, 2)):
        assert len(table) == size and not declared & set(table)
    assert len(lib.PROC_SIGNATURES["nv_decode_pick_proc_bf16"][1]) == 28 and len(lib.PROC_SIGNATURES["nv_decoder_proc_step"][1]) == 37
    L = lib.load()                                    # binds every table: raises when the library does not export a name
    one = 1 << 12                                     # (any non-null pointer value will do: nothing is launched)
    args = dict(logits=one, ldl=1024, V=1006, special0=1000, nspecial=5, off=None, tok=None, nxt=None, n_nodes=0, node=None, sample=0,
                temperature=0.0, top_k=0, top_p=1.0, rng=None, u_out=None, kept_out=None, seen=one, seen_ld=32, pen=1.3, min_new=4, state=one,
                out=one, max_steps=4, B=3, eos=2, pad=0, stream=None)
    trie = dict(off=one, tok=one, nxt=one, n_nodes=5, node=one)
    bad = [dict(pen=v) for v in (0.0, -1.0, float("nan"), float("inf"))] + [dict(min_new=-1), dict(seen=None), dict(seen_ld=31), trie,
           dict(trie, min_new=1), dict(sample=1), dict(sample=1, rng=one, temperature=0.0), dict(sample=1, rng=one, temperature=1.0, top_p=0.0),
           dict(sample=1, rng=one, temperature=1.0, top_k=-1), dict(ldl=1000), dict(state=None), dict(off=one), dict(B=0)]
    for kw in bad:
        assert L.nv_decode_pick_proc_bf16(*dict(args, **kw).values()) == -1, kw
    step = dict(p=one, hs=one, embed=one, lm_head=one, Vp=1024, V=1006, special0=1000, nspecial=5, off=None, tok=None, nxt=None, n_nodes=0,
                node=None, sample=0, temperature=0.0, top_k=0, top_p=1.0, rng=None, seen=one, seen_ld=32, pen=1.3, min_new=4, logits=one, x=one,
                state=one, out=one, max_steps=4, kv0=one, attn=one, lse=one, B=3, cap=64, eos=2, pad=0, ws=one, ws_bytes=0, stream=None)
    for kw in [dict(pen=v) for v in (0.0, -1.0, float("nan"), float("inf"))] + [dict(min_new=-1), dict(seen=None), dict(seen_ld=31),
                                                                                 dict(trie, min_new=1), dict(sample=1), dict(p=None), dict(Vp=1000)]:
        assert L.nv_decoder_proc_step(*dict(step, **kw).values()) == -1, kw


def test_generate_refuses_bad_processor_arguments_before_any_work():
    """the check is generate()'s first act: it is reached on an object that has no buffers, no model and no device at all; values that
    pass it fail on the missing attributes instead"""
    from navillm_amd.kvcache import KVCacheLM, _check_processors
    kv = object.__new__(KVCacheLM)
    for do_sample in (False, True):
        for bad in (0, 0.0, -1.3, float("nan"), float("inf"), "1.2", True, False, 1 + 0j, [1.2], 1e-60, 1e60):
            with pytest.raises(ValueError, match="repetition_penalty"):
                KVCacheLM.generate(kv, [[1, 5]], do_sample=do_sample, repetition_penalty=bad)
        for bad in (-1, 1.0, 2.5, "4", True, False, float("nan"), [4]):
            with pytest.raises(ValueError, match="min_new_tokens"):
                KVCacheLM.generate(kv, [[1, 5]], do_sample=do_sample, min_new_tokens=bad)
        with pytest.raises(ValueError, match="trie"):
            KVCacheLM.generate(kv, [[1, 5]], do_sample=do_sample, min_new_tokens=1, trie=object())
        for good in (dict(), dict(repetition_penalty=None, min_new_tokens=None), dict(repetition_penalty=1.3, min_new_tokens=4),
                     dict(repetition_penalty=np.float32(0.8)), dict(repetition_penalty=2, min_new_tokens=np.int64(3)),
                     dict(repetition_penalty=1.3, min_new_tokens=0, trie=object())):
            with pytest.raises(AttributeError):                        # past the check
                KVCacheLM.generate(kv, [[1, 5]], do_sample=do_sample, **good)
    assert _check_processors(None, None, None) is None and _check_processors(1.0, 0, object()) is None and _check_processors(1, 0, None) is None
    assert _check_processors(1.3, None, None) == (float(np.float32(1.3)), 0) and _check_processors(None, 4, None) == (1.0, 4)


class _Recorder:
    """stands in for the library: records the name of every entry point called, answers NV_OK"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        return lambda *a: self.calls.append((name, a)) or 0


def test_processor_free_calls_take_the_old_symbols(monkeypatch):
    """`_greedy_step` without processors calls the step entry points it called before there were any, with their argument lists;
    with processors it calls nv_decoder_proc_step alone.  In the C sources the old picks and steps are calls of the new ones with
    seen = NULL, penalty 1 and min_new 0, which launch the PROC = false kernels."""
    from navillm_amd import kvcache as kvm, lib, ops
    rec = _Recorder()
    monkeypatch.setattr(ops, "_L", lambda: rec)
    t = lambda: types.SimpleNamespace(data_ptr=lambda: 4096, numel=lambda: 64, shape=(3, 8))
    model = types.SimpleNamespace(cfg=types.SimpleNamespace(special_token_ids=(250, 251), vocab_size=256),
                                  store=types.SimpleNamespace(p=lambda name: t(), lm_head_padded=t, vocab_pad=256))
    kv = types.SimpleNamespace(model=model, kv0=t(), attn=t(), lse=t(), B=3, cap=64, _ws=t())
    g = {k: t() for k in ("hs", "logits", "x", "state", "out", "rng", "node", "seen")}
    g["max_steps"] = 8
    trie = {"off": t(), "tok": t(), "nxt": t(), "n_nodes": 5}
    smp = lambda top_p: {"temperature": 0.7, "top_k": 5, "top_p": top_p}
    want = {(False, None): "nv_decoder_greedy_step", (True, None): "nv_decoder_trie_step", (False, 1.0): "nv_decoder_sample_step",
            (True, 1.0): "nv_decoder_sample_step", (False, 0.9): "nv_decoder_sample_topp_step", (True, 0.9): "nv_decoder_sample_topp_step"}
    tables = {**lib.SIGNATURES, **lib.TOPP_SIGNATURES, **lib.PROC_SIGNATURES}
    for (constrained, top_p), name in want.items():
        for procs in (None, (1.5, 0), (1.0, 4)):
            rec.calls.clear()
            kvm.KVCacheLM._greedy_step(kv, g, 2, 0, None, 4096, trie if constrained else None, None if top_p is None else smp(top_p), procs)
            (called, a), = rec.calls
            assert called == (name if procs is None else "nv_decoder_proc_step"), (constrained, top_p, procs, called)
            assert len(a) == len(tables[called][1])
    src = inspect.getsource(kvm.KVCacheLM._greedy_step)
    assert src.count("nv_decoder_proc_step(") == 1 and src.index("if procs is not None:") < src.index("nv_decoder_proc_step(") < src.index("elif sampler")
    hip = open(os.path.join(ROOT, "navillm_amd", "csrc", "decode_step.hip")).read()
    off = r"nullptr,\s*0,\s*1\.0f,\s*0,\s*state,"                       # seen, seen_ld, rep_penalty, min_new
    for old in ("nv_decode_pick_bf16", "nv_decode_pick_trie_bf16", "nv_decode_pick_sample_topp_bf16"):
        body = hip[hip.index(f"int {old}("):]
        body = body[:body.index("\n}\n")]
        assert re.search(r"return nv_decode_pick_proc_bf16\(", body) and re.search(off, body), old
    assert re.search(r"const bool proc = seen \|\| min_new > 0;", hip)
    for k in ("decode_pick_kernel", "decode_pick_trie_kernel"):
        assert re.search(rf"if \(proc\) NV_PICK_GREEDY\({k}<true>.*\n\s*else NV_PICK_GREEDY\({k}<false>", hip), k
    rt = open(os.path.join(ROOT, "navillm_amd", "csrc", "decoder_runtime.cpp")).read()
    assert rt.count("nv_decode_pick_proc_bf16(") == 1 and len(re.findall(r"return decode_step\(", rt)) == 4
    for old in ("nv_decoder_greedy_step", "nv_decoder_trie_step", "nv_decoder_sample_topp_step"):
        body = rt[rt.index(f"int {old}("):]
        body = body[:body.index("\n}\n")]
        assert re.search(r"nullptr,\s*0,\s*1\.f,\s*0,\s*logits,", body), old
