"""References of sampled decoding for the tests (numpy, no GPU): Philox4x32-10 with the library's counter / key convention and an
fp64 restatement of the draw rule of `decode_pick_sample_kernel` (navillm_amd/csrc/decode_step.hip)."""
import numpy as np

_U64 = np.uint64
_MASK = _U64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: 4 words, key: 2 words (ints or equal-shaped integer arrays) -> the 4 output words as uint64 arrays < 2^32"""
    c = [np.asarray(x, dtype=_U64) & _MASK for x in counter]
    k0, k1 = (np.asarray(x, dtype=_U64) & _MASK for x in key)
    for _ in range(10):
        p0, p1 = _U64(0xD2511F53) * c[0], _U64(0xCD9E8D57) * c[2]
        c = [(p1 >> _U64(32)) ^ c[1] ^ k0, p1 & _MASK, (p0 >> _U64(32)) ^ c[3] ^ k1, p0 & _MASK]
        k0, k1 = (k0 + _U64(0x9E3779B9)) & _MASK, (k1 + _U64(0xBB67AE85)) & _MASK
    return c


def philox_u(seed, counter):
    """the uniform of 64-bit `counter` (int or array) under `seed`: c0/c1 = the counter's low/high word, c2 = c3 = 0, key = the
    seed's low/high word; u = (word0 >> 8) * 2^-24 + 2^-25 as fp32 (exact)"""
    n = np.asarray(counter, dtype=_U64)
    s = _U64(int(seed) & 0xFFFFFFFFFFFFFFFF)
    w0 = philox4x32_10((n & _MASK, n >> _U64(32), 0, 0), (s & _MASK, s >> _U64(32)))[0]
    return ((w0 >> _U64(8)).astype(np.float32) * np.float32(2.0 ** -24) + np.float32(2.0 ** -25)).astype(np.float32)


def sample_reference(logits, allowed_ids, T, top_k, u):
    """HF sample() for one row, in fp64.  `logits`: the row; `allowed_ids`: its candidates (pickable ids / pickable trie children;
    one with a NaN logit is dropped); top-k keeps every candidate >= the top_k-th largest candidate logit (ties included; None, 0 or
    >= the candidate count keeps all); w = exp((x - max) / T), 0 at -inf; the token is the kept id, in ascending order, whose
    running sum first exceeds u * total.
    -> dict(token: the id, or None when no kept candidate has weight > 0; ids: the kept ids ascending; w: their weights;
            lo, hi: their CDF intervals [lo, hi) as fractions of the total)"""
    x = np.asarray(logits, dtype=np.float64)
    ids = np.array(sorted(set(int(v) for v in allowed_ids)), dtype=np.int64)
    ids = ids[~np.isnan(x[ids])] if ids.size else ids
    if top_k and 0 < top_k < ids.size:
        kth = np.sort(x[ids])[::-1][top_k - 1]
        ids = ids[x[ids] >= kth]
    if ids.size == 0:
        return dict(token=None, ids=ids, w=np.zeros(0), lo=np.zeros(0), hi=np.zeros(0))
    xs = x[ids]
    m = xs.max()
    with np.errstate(invalid="ignore", over="ignore"):
        w = np.where(xs == -np.inf, 0.0, np.where(xs == m, 1.0, np.exp((xs - m) / float(T))))
    total = w.sum()
    if not total > 0:
        return dict(token=None, ids=ids, w=w, lo=np.zeros(ids.size), hi=np.zeros(ids.size))
    cdf = np.cumsum(w)
    hit = np.flatnonzero((cdf > float(u) * total) & (w > 0))
    j = int(hit[0]) if hit.size else int(np.flatnonzero(w > 0)[-1])
    return dict(token=int(ids[j]), ids=ids, w=w, lo=(cdf - w) / total, hi=cdf / total)


def check_draw(ref, token, u, eps):
    """what the GPU tests assert of one drawn token: a kept candidate of non-zero weight whose CDF interval, widened by eps, holds u.
    -> how far outside [lo, hi) u lies (0.0 inside): the figure eps allows for"""
    j = np.flatnonzero(ref["ids"] == token)
    assert j.size == 1, ("not a kept candidate", token)
    j = int(j[0])
    assert ref["w"][j] > 0, ("zero weight", token)
    assert ref["lo"][j] - eps <= float(u) < ref["hi"][j] + eps, (token, float(u), ref["lo"][j], ref["hi"][j], ref["token"])
    return max(ref["lo"][j] - float(u), float(u) - ref["hi"][j], 0.0)
