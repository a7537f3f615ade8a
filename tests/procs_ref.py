"""The numpy reference of the two logits processors of the decode loop (repetition penalty, minimum length) for the tests -- no GPU, no
torch arithmetic -- and the inputs that tests/test_procs_decode_gpu.py feeds the pick kernels.

The rule (DESIGN.md §4 "Logits processors"; navillm_amd/csrc/decode_step.hip): seen[b] is the set of ids in row b's own sequence (its
unpadded prompt and every token it emitted while unfinished).  With p32 = float32(penalty), a bf16 logit x of an id in seen[b] becomes
bf16_rne(float32(x) * p32) when x < 0, else bf16_rne(float32(x) / p32); -inf stays -inf, a NaN stays a NaN (written here as
0x7FC0).  While cnt < min_new, `eos` is no candidate.  Both run after the special-id mask and in front of the trie, temperature,
top-k and top-p, so the sampled picks are tests/sample_ref.py and tests/topp_ref.py on the penalised row over the remaining candidates."""
import numpy as np

from topp_ref import topp_reference


# ------------------------------------------------------------------------------------------------ the penalty on bf16 bit patterns
def bf16_bits(x):
    """fp32 array -> its bf16 patterns (uint16), round to nearest even; a NaN -> 0x7FC0"""
    x = np.asarray(x, dtype=np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    r = ((u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(np.uint16)
    return np.where(np.isnan(x), np.uint16(0x7FC0), r)


def bf16_value(bits):
    """bf16 patterns (uint16) -> fp32"""
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def penalise_bits(bits, penalty):
    """the penalty on bf16 patterns: uint16 array -> uint16 array"""
    x = bf16_value(bits)
    p32 = np.float32(penalty)
    with np.errstate(all="ignore"):
        y = np.where(x < 0, x * p32, x / p32).astype(np.float32)
    return bf16_bits(y)


# ------------------------------------------------------------------------------------------------ the seen set and its bitmap
def seen_sets(prompts):
    return [set(int(t) for t in p) for p in prompts]


def seen_update(seen, tokens, unfinished):
    """after one step: an unfinished row marks what it emitted (its `eos` too); a finished row emitted `pad` and marks nothing"""
    for s, t, live in zip(seen, tokens, unfinished):
        if live:
            s.add(int(t))


def bitmap(seen, V, ld):
    """[B, ld] uint32: bit v & 31 of word v >> 5 holds id v"""
    assert ld >= (V + 31) // 32
    bm = np.zeros((len(seen), ld), np.uint32)
    for b, s in enumerate(seen):
        for v in s:
            if 0 <= v < V:
                bm[b, v >> 5] |= np.uint32(1 << (v & 31))
    return bm


# ------------------------------------------------------------------------------------------------ the picks on a processed row
def candidates(V, sp0, nsp, eos, cnt, min_new):
    """the dense candidates: [0, V) without the special range, and without `eos` while cnt < min_new"""
    return [v for v in range(V) if not sp0 <= v < sp0 + nsp and not (cnt < min_new and v == eos)]


def processed_row(bits_row, seen_b, penalty, V):
    """row of bf16 patterns -> fp64 values with the penalty on the seen ids inside [0, V)"""
    bits = np.array(bits_row, dtype=np.uint16)
    ids = np.array(sorted(v for v in seen_b if 0 <= v < V), dtype=np.int64)
    if ids.size:
        bits[ids] = penalise_bits(bits[ids], penalty)
    return bf16_value(bits).astype(np.float64)


def greedy_reference(bits_row, ids, seen_b, penalty, V):
    """the argmax over the candidates `ids` of the processed row: the largest value, ties to the smallest id; None without candidates"""
    x = processed_row(bits_row, seen_b, penalty, V)
    ids = sorted(set(int(v) for v in ids))
    if not ids:
        return None
    xs = x[ids]
    assert not np.isnan(xs).any()
    return int(np.array(ids)[xs == xs.max()][0])


def sampled_reference(bits_row, ids, seen_b, penalty, V, T, top_k, top_p, u):
    """tests/topp_ref.topp_reference (and through it tests/sample_ref.sample_reference) on the processed row"""
    return topp_reference(processed_row(bits_row, seen_b, penalty, V), ids, T, top_k, top_p, u)


# ------------------------------------------------------------------------------------------------ the inputs of the kernel-level tests
SHAPES = ((3, 37, 37), (3, 300, 304), (3, 8205, 8208))                # (B, V, ldl): scalar loads and two bitmap words / vector loads / a
SHAPE_IDS = ("V37_scalar_loads", "V300_vector_loads", "V8205_second_trip")          # second trip of the 1024 x 8 stride
NSPECIAL, EOS, PAD = 2, 2, 0
PENALTY = 1.5


def special0(V):
    return V - 4


def far_id(V):
    """an id past the first 32 (a second bitmap word) and, at V > 8192, past the first trip of the 1024 x 8 stride"""
    return V - 5


def base_rows(shape, seed, lo):
    """[B, ldl] bf16 patterns of -|randn| + lo: everything a test plants lies above `lo`"""
    B, V, ldl = shape
    rng = np.random.RandomState(seed)
    return bf16_bits((lo - np.abs(rng.randn(B, ldl))).astype(np.float32))


def set_logits(rows, b, ids, values):
    rows[b, list(ids)] = bf16_bits(np.asarray(values, dtype=np.float32))


def greedy_case(shape):
    """rows whose winner the penalty changes -> (logit patterns [B, ldl], seen sets).
    row 0  the unpenalised maximum 8 sits at the seen id far_id: 8 / 1.5 = 5.33 < the 6 of the unseen id 3
    row 1  every logit negative; the maximum -2 at the seen id 3 becomes -3 < the -2.5 of the unseen id far_id
    row 2  the seen id 5 at 6 becomes 6 / 1.5 = 4 exactly, the 4 of the unseen id far_id: a tie the penalty made, which goes to id 5
    In every row a few ids of the base are seen as well (negative logits: multiplied), one of them in the special range."""
    B, V, ldl = shape
    rows = base_rows(shape, 11, -4.0)
    f = far_id(V)
    set_logits(rows, 0, (f, 3), (8.0, 6.0))
    set_logits(rows, 1, (3, f), (-2.0, -2.5))
    set_logits(rows, 2, (5, f), (6.0, 4.0))
    seen = [{f, 1, 7, special0(V)}, {3, 1, 9, V - 1}, {5, 1, 8, 33}]
    return rows, seen


def min_new_case(shape):
    """`eos` holds every row's maximum (10), id far_id the runner-up (9, 8, 7 by row) -> (logit patterns, seen sets: empty)"""
    B, V, ldl = shape
    rows = base_rows(shape, 12, 0.0)
    for b in range(B):
        set_logits(rows, b, (EOS, far_id(V)), (10.0, 9.0 - b))
    return rows, [set() for _ in range(B)]


TRIE_WORDS = ([3, 20], [9, 21], [17, 22], [30])                       # the root's children: 3, 9, 17, 30 (all < 37)


def trie_case(shape):
    """every row at the root.  The row maximum 20 is at id 12, no child.  Among the children: 9 holds 8 and is seen (-> 5.33), 3 holds 6,
    17 holds 5, 30 holds 2; id 12 and the child 30 are seen too -> the winner moves from 9 to 3.  Row 1: negative children, the seen
    child 9 at -2 (-> -3) loses to 17 at -2.5.  Row 2: nothing of it is seen, so 9 wins as it would without the penalty."""
    B, V, ldl = shape
    rows = base_rows(shape, 13, -6.0)
    set_logits(rows, 0, (12, 9, 3, 17, 30), (20.0, 8.0, 6.0, 5.0, 2.0))
    set_logits(rows, 1, (12, 9, 3, 17, 30), (20.0, -2.0, -4.0, -2.5, -5.0))
    set_logits(rows, 2, (12, 9, 3, 17, 30), (20.0, 8.0, 6.0, 5.0, 2.0))
    seen = [{9, 12, 30}, {9, 12}, {4}]
    return rows, seen


SAMPLE_SETTINGS = ((1.0, 0, 1.0), (0.7, 5, 0.9), (1.0, 0, 0.5), (2.0, 4, 0.8))        # (T, top_k, top_p)
SAMPLE_CNTS = (0, 2)
SAMPLE_MIN_NEW = 1                                                    # cnt 0: eos is banned; cnt 2: it is a candidate again
SAMPLE_PENALTY = 1.3


def sample_case(shape):
    """a base 20 below six planted ids per row (8, 7.5, 7, 6, 5, 4 + b/4, one of them `eos`), of which the two largest and some ids of
    the base are seen: the penalty reorders the planted ids (8 / 1.3 = 6.16, 7.5 / 1.3 = 5.77) and with them the top-k set and the
    nucleus.  Where top_k = 0 lets the base in (T <= 1) it weighs < 1e-4 of the total, so every top-p boundary falls among the planted classes."""
    B, V, ldl = shape
    rows = base_rows(shape, 14, -16.0)
    f = far_id(V)
    planted = (f, 6, EOS, 18, 35, 10)
    seen = []
    for b in range(B):
        set_logits(rows, b, planted, np.array([8.0, 7.5, 7.0, 6.0, 5.0, 4.0]) + 0.25 * b)
        seen.append({f, 6, 1, 13, special0(V), V - 1} if b != 2 else {EOS, 18, 11})
    return rows, seen
