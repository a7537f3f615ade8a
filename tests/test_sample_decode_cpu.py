"""CPU: the references of sampled decoding on the device (tests/sample_ref.py: Philox4x32-10 against the Random123 known answers,
the fp64 sampler against hand-made rows) and the plumbing of `nv_decode_pick_sample_bf16` / `nv_decoder_sample_step`.  No kernel is
launched here."""
import os

import numpy as np

from sample_ref import philox4x32_10, philox_u, sample_reference, check_draw
from util import ROOT


def test_numpy_philox_reproduces_the_random123_known_answers():
    kat = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for ctr, key, want in kat:
        assert " ".join(f"{int(w):08x}" for w in philox4x32_10(ctr, key)) == want
    # vectorised == one at a time; the counter's high word and the seed's high word are used
    n = np.array([0, 1, (1 << 32) - 1, 1 << 32, (1 << 40) + 7], dtype=np.uint64)
    seed = 0x123456789abcdef1
    u = philox_u(seed, n)
    assert u.dtype == np.float32 and [float(philox_u(seed, int(k))) for k in n] == u.tolist()
    assert len(set(u.tolist())) == 5 and float(philox_u(seed & 0xffffffff, 0)) != float(u[0])
    w0 = int(philox4x32_10((0, 0, 0, 0), (0, 0))[0])
    assert float(philox_u(0, 0)) == (w0 >> 8) * 2.0 ** -24 + 2.0 ** -25
    # the range: never 0; the 25-bit sum is exact below 0.5 and rounds to even above, so the topmost cell gives 1.0 (the draw rule's
    # "past the end" case then takes the last kept candidate)
    k = np.array([0, 1, (1 << 23) - 1, 1 << 23, (1 << 23) + 1, (1 << 24) - 2, (1 << 24) - 1], dtype=np.float32)
    uk = k * np.float32(2.0 ** -24) + np.float32(2.0 ** -25)
    assert uk.dtype == np.float32 and uk[0] == 2.0 ** -25 and uk[2] == 0.5 - 2.0 ** -25 and uk[-1] == 1.0 and bool((np.diff(uk) > 0).all())


def test_sample_reference_on_hand_made_rows():
    x = np.array([1.0, 3.0, 2.0, 2.0, 2.0, 0.0, -np.inf, 5.0, np.nan])
    cand = [0, 1, 2, 3, 4, 5, 6, 8]                               # id 7 (the row's maximum) is no candidate, id 8 is a NaN
    # top_k = 2: the second largest candidate is 2.0, three candidates tie there -> all of them are kept
    r = sample_reference(x, cand, 1.0, 2, 0.5)
    assert r["ids"].tolist() == [1, 2, 3, 4]
    e = np.exp(-1.0)
    np.testing.assert_allclose(r["w"], [1.0, e, e, e], rtol=1e-15)
    np.testing.assert_allclose(r["hi"], np.cumsum([1.0, e, e, e]) / (1 + 3 * e), rtol=1e-15)
    assert r["lo"][0] == 0.0 and r["hi"][-1] == 1.0 and r["lo"][1:].tolist() == r["hi"][:-1].tolist()
    # top_k = 0 / None / >= the number of candidates (7 without the NaN): everything is kept, -inf with weight 0
    for k in (0, None, 7, 8, 1000):
        r = sample_reference(x, cand, 1.0, k, 0.5)
        assert r["ids"].tolist() == [0, 1, 2, 3, 4, 5, 6] and r["w"][6] == 0.0, k
    # a -inf candidate is never drawn, not even by the largest u; neither is a non-candidate
    for u in (2.0 ** -25, 0.3, 0.999, 1.0 - 2.0 ** -25):
        for k in (0, 3, 6, 7):
            assert sample_reference(x, cand, 0.7, k, u)["token"] in (0, 1, 2, 3, 4, 5)
    assert sample_reference(x, [6], 1.0, 0, 0.5)["token"] is None          # nothing but -inf: no token
    assert sample_reference(x, [], 1.0, 0, 0.5)["token"] is None and sample_reference(x, [8], 1.0, 0, 0.5)["token"] is None
    # T = 0.01 with a gap of one bf16 spacing at 4.0 (2^-5): the runner-up weighs exp(-3.125), nothing underflows, total >= 1
    y = np.array([4.0, 4.0 - 2.0 ** -5, 1.0])
    r = sample_reference(y, [0, 1, 2], 0.01, 0, 0.5)
    np.testing.assert_allclose(r["w"], [1.0, np.exp(-3.125), 0.0], rtol=1e-12, atol=1e-120)
    p1 = np.exp(-3.125) / (1 + np.exp(-3.125))
    assert r["token"] == 0 and sample_reference(y, [0, 1, 2], 0.01, 0, 1 - p1 / 2)["token"] == 1
    # u just below / just above a CDF boundary (weights 1, 1, 2 of 4 -> boundaries 0.25 and 0.5), ascending id order
    z = np.log(np.array([1.0, 1.0, 2.0]))
    for u, want in ((0.25 - 1e-9, 0), (0.25 + 1e-9, 1), (0.5 - 1e-9, 1), (0.5 + 1e-9, 2), (1 - 1e-9, 2), (1e-9, 0)):
        r = sample_reference(z, [2, 0, 1], 1.0, 0, u)
        assert r["token"] == want, (u, want)
        check_draw(r, want, u, 0.0)
    # check_draw refuses a neighbour beyond eps and accepts it within
    r = sample_reference(z, [0, 1, 2], 1.0, 0, 0.25 + 1e-7)
    check_draw(r, 0, 0.25 + 1e-7, 1e-5)
    for bad_tok, bad_u in ((0, 0.26), (2, 0.3), (5, 0.3)):
        try:
            check_draw(r, bad_tok, bad_u, 1e-5)
        except AssertionError:
            continue
        raise AssertionError((bad_tok, bad_u))


def test_header_and_binding_declare_the_sampled_pick_and_step():
    from navillm_amd import lib
    hdr = open(os.path.join(ROOT, "include", "navillm_hip.h")).read()
    for name in ("nv_decode_pick_sample_bf16", "nv_decoder_sample_step"):
        assert f"int {name}(" in hdr and name in lib.SIGNATURES, name
    assert len(lib.SIGNATURES) == 119
    L = lib.load()                                    # binds every declared symbol: raises when the library does not export one
    assert len(lib.SIGNATURES["nv_decode_pick_sample_bf16"][1]) == 21 and len(lib.SIGNATURES["nv_decoder_sample_step"][1]) == 31
    # argument errors return before any launch (any non-null pointer value will do)
    one = 1 << 12
    args = dict(logits=one, ldl=1024, V=1006, special0=1000, nspecial=5, off=one, tok=one, nxt=one, n_nodes=3, node=one, temperature=0.7,
                top_k=50, rng=one, u_out=None, state=one, out=one, max_steps=4, B=7, eos=2, pad=0, stream=None)
    bad = [(k, None) for k in ("logits", "rng", "state", "out", "off", "tok", "nxt", "node")]          # (a partly-null trie among them)
    bad += [("B", 0), ("V", 0), ("ldl", 1000), ("n_nodes", 0), ("max_steps", -1), ("nspecial", -1), ("top_k", -1), ("temperature", 0.0),
            ("temperature", -1.0), ("temperature", float("inf")), ("temperature", float("nan")), ("temperature", 1e-60)]
    for k, v in bad:
        a = dict(args)
        a[k] = v
        assert L.nv_decode_pick_sample_bf16(*a.values()) == -1, (k, v)
    free = dict(args, off=None, tok=None, nxt=None, n_nodes=0, node=None)
    assert L.nv_decode_pick_sample_bf16(*dict(free, n_nodes=3).values()) == -1
    assert L.nv_decode_pick_sample_bf16(*dict(free, node=one).values()) == -1
    assert L.nv_decoder_sample_step(*([None] * 4), 0, 0, 0, 0, None, None, None, 0, None, 1.0, 0, None, None, None, None, None, 0, None, None,
                                    None, 0, 0, 0, 0, None, 0, None) == -1
