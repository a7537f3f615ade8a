"""The fp64 reference of nucleus (top-p) sampling for the tests (numpy, no GPU), on top of tests/sample_ref.py, and the case list that
tests/test_topp_decode_cpu.py and tests/test_topp_decode_gpu.py share.

The rule (decode_pick_sample_kernel, navillm_amd/csrc/decode_step.hip): after top-k, with w = exp((x - m) / T) the survivors' weights
and W their sum, a logit value x stays iff S(x), the weight of the survivors with a STRICTLY larger logit, is < top_p * W.  Survivors
that share a logit value stay or go together; the class of the maximum always stays; the draw runs over what stayed.

BAND = 1e-5 is the bound of tests/test_sample_decode_gpu.py (EPS) for the fp32 running sums of that kernel; the sums that decide the
boundary have the same depth.  A case is AMBIGUOUS when some logit class other than the maximum's has |S - top_p * W| <= BAND * W:
fp32 may then decide that class either way.  The class of the maximum is left out of that test because it has no decision to take:
its S is 0 in any arithmetic and 0 < top_p * W."""
import functools

import numpy as np
import torch

from sample_ref import sample_reference

BAND = 1e-5


def topp_reference(logits, allowed_ids, T, top_k, top_p, u, band=BAND):
    """-> sample_reference's dict for the survivors of both warpers (token, ids ascending, w, lo, hi) plus kept: their number, 0 where
    no survivor has weight (the kernel then emits eos); ambiguous; alt: for an ambiguous case the two references with every class
    inside the band dropped / kept (each without `alt`), else ()"""
    x = np.asarray(logits, dtype=np.float64)
    base = sample_reference(x, allowed_ids, T, top_k, u)
    if base["token"] is None:
        return dict(base, kept=0, ambiguous=False, alt=())
    ids, w = base["ids"], base["w"]
    if top_p is None or top_p >= 1.0:
        return dict(base, kept=int(ids.size), ambiguous=False, alt=())
    xs, W = x[ids], w.sum()
    order = np.argsort(-xs, kind="stable")
    xo, wo = xs[order], w[order]
    before = np.cumsum(wo) - wo                                        # the weight sorted in front of each survivor ...
    first = np.r_[True, xo[1:] != xo[:-1]]
    above = np.maximum.accumulate(np.where(first, before, 0.0))        # ... at the first of a run of equal logits: the weight strictly above
    S = np.empty_like(above)
    S[order] = above
    lim = float(top_p) * W
    top = xs == xs.max()

    def side(keep):
        r = sample_reference(x, ids[keep | top], T, 0, u)
        return dict(r, kept=int(r["ids"].size), ambiguous=False, alt=())

    near = (np.abs(S - lim) <= band * W) & ~top
    ref = side(S < lim)
    if near.any():
        ref["ambiguous"] = True
        ref["alt"] = (side((S < lim) & ~near), side((S < lim) | near))
    return ref


def hf_top_p_keep(scores, top_p):
    """HF's TopPLogitsWarper.__call__ (min_tokens_to_keep = 1) restated literally on one fp64 row of already warped scores (a kept-out
    entry is -inf): ascending sort, softmax, cumulative sum, remove where cumsum <= 1 - top_p, never the last.  -> bool keep mask"""
    s = torch.as_tensor(np.asarray(scores, dtype=np.float64))[None]
    sorted_logits, sorted_indices = torch.sort(s, descending=False)
    cumulative_probs = sorted_logits.softmax(dim=-1).cumsum(dim=-1)
    sorted_indices_to_remove = cumulative_probs <= (1 - top_p)
    sorted_indices_to_remove[..., -1:] = 0
    indices_to_remove = sorted_indices_to_remove.scatter(1, sorted_indices, sorted_indices_to_remove)
    return (~indices_to_remove)[0].numpy()


# ------------------------------------------------------------------------------------------------ the cases of the kernel-level tests
SHAPES = ((7, 1006, 1024, 1000), (3, 9001, 9008, 8990), (7, 1006, 1011, 1000))      # (B, V, ldl, special0)
SHAPE_IDS = ("V1006", "V9001_several_ids_per_thread", "ldl_no_multiple_of_8")
NSPECIAL = 5
TEMPS, TOPKS, TOPPS = (0.01, 1.0, 100.0), (0, 1, 50), (1e-6, 0.5, 0.9, 0.999)
ROW_SEED, TRIE_SEED = 4, 6                                             # picked so that no case below is ambiguous
TOP, TIE3, LADDER = 700, (5, 9, 11), 60                                # ids / sizes of the planted rows below


def ladder_ids():
    return [20 + 13 * j for j in range(LADDER)]


@functools.lru_cache(maxsize=None)
def planted_rows(B, V, ldl, sp0, seed=ROW_SEED):
    """randn * 2 in bf16 with, by row % 7:
    0  the row maximum inside the special range and a larger one at an id >= V; among the candidates id TOP at 30: at T <= 1 it carries
       all but e^-20 of the weight, so every top_p here keeps it alone and it is the token for every u;
    1  id TOP at 10, the ids TIE3 (in FRONT of it) at 9, everything else 20 lower: at T = 1, top_k = 0 the weights are 1, 3 x e^-1 and
       ~1e-4 in all, so W = 2.104 and at top_p = 0.5 the limit 1.052 falls INSIDE the tie (S = 1 for the three; one of them alone
       would already pass it): all three stay, the kept count is 4, and dropping one would shift the CDF interval of TOP;
    2  a three-way tie for the maximum, at 20 (kept whole by top_k = 1 and by top_p = 1e-6);
    3  finished earlier;
    4  every candidate at -inf;
    5  a ladder of LADDER ids at 8.5, 8.375, ... (steps of 1/8, exact in bf16), everything else 20 lower.  T = 1, top_k = 50: top_p = 0.5
       keeps the 6 largest (top-p cuts inside the top-k set); top_p = 0.999 keeps 47, down to 2.75, while the top-k threshold is 2.375:
       the same high byte of the 16-bit key.  T = 100, top_k = 50: the 50 weigh about the same, so no top_p here drops any (top-k set
       smaller than the nucleus);
    6  a NaN and a -inf among ordinary candidates, one of them at 16.
    At T = 100 the weights of the randn part are nearly equal, so top_p = 0.9 puts the boundary among the negative logits.
    The maxima of rows 2 and 6 are as large as they are for the sake of T = 1, top_p = 0.999: the ~1000 (9000) randn logits form classes
    of ~1e-5 of their total weight each, finer than the band, so a boundary that falls among them is ambiguous whatever the seed; under
    these maxima they weigh < 1e-3 of W in all and the boundary stays above them.
    -> (logits [B, ldl] bf16, fin [B])"""
    g = torch.Generator().manual_seed(seed)
    lg = (torch.randn(B, ldl, generator=g) * 2).to(torch.bfloat16)
    fin = [0] * B
    for b in range(B):
        k = b % 7
        if k == 0:
            lg[b, sp0 + 1] = 50.0
            lg[b, V + 2] = 60.0
            lg[b, TOP] = 30.0
        elif k == 1:
            lg[b] = (lg[b].float() - 20.0).to(torch.bfloat16)
            lg[b, TOP] = 10.0
            lg[b, list(TIE3)] = 9.0
        elif k == 2:
            lg[b, 7] = lg[b, 300] = lg[b, V - 20] = 20.0
        elif k == 3:
            fin[b] = 1
        elif k == 4:
            lg[b, :V] = float("-inf")
            lg[b, sp0] = 3.0
        elif k == 5:
            lg[b] = (lg[b].float() - 20.0).to(torch.bfloat16)
            lg[b, ladder_ids()] = (8.5 - torch.arange(LADDER) * 0.125).to(torch.bfloat16)
        else:
            lg[b, 11] = float("nan")
            lg[b, 12] = float("-inf")
            lg[b, 13] = 16.0
    return lg, tuple(fin)


def candidates(V, sp0):
    return [v for v in range(V) if not sp0 <= v < sp0 + NSPECIAL]


_refs = {}


def case_reference(shape, b, T, top_k, top_p):
    """the reference of row b of `shape` under one setting, computed once (kept set and CDF do not depend on u)"""
    key = (shape, b, T, top_k, top_p)
    if key not in _refs:
        B, V, ldl, sp0 = shape
        lg, _ = planted_rows(B, V, ldl, sp0)
        _refs[key] = topp_reference(lg[b].double().numpy(), candidates(V, sp0), T, top_k, top_p, 0.5)
    return _refs[key]


def kernel_cases(shape):
    """every (T, top_k, top_p) of the kernel-level test of one shape"""
    return [(T, k, p) for T in TEMPS for k in TOPKS for p in TOPPS]


# ------------------------------------------------------------------------------------------------ the trie case
class _Node:
    def __init__(self):
        self.child = {}


class Trie:
    """tools/trie.py protocol (root / get_child_index / get_next_node); a token that is no child changes nothing"""

    def __init__(self, eos, words=()):
        self.root, self.eos = _Node(), eos
        for w in words:
            cur = self.root
            for c in w:
                cur = cur.child.setdefault(int(c), _Node())

    def get_child_index(self, cur):
        return [self.eos] if not cur.child else list(cur.child.keys())

    def get_next_node(self, cur, w):
        return cur.child[w] if w in cur.child else cur

    def at(self, path):
        cur = self.root
        for c in path:
            cur = cur.child[c]
        return cur


TRIE_SHAPE = (7, 1006, 1024, 1000)                                     # (B, V, ldl, special0); eos 2, pad 1005
TRIE_PATHS = ([100], [101], [102], [103], [104], [100], [105])
TRIE_FIN = (0, 0, 0, 0, 0, 1, 0)


@functools.lru_cache(maxsize=None)
def trie_case(seed=TRIE_SEED):
    """rows at nodes with 3 children, 1 child, 3 children of which one >= V, 4 of which one special and the other three tied, a leaf,
    a finished row, and 300 children.  -> (trie, logits [B, ldl] bf16, the candidates of every row)"""
    B, V, ldl, sp0 = TRIE_SHAPE
    words = [[100, 10], [100, 20], [100, 30], [101, 40], [102, 1010], [102, 50], [102, 51], [103, 1001], [103, 7], [103, 300], [103, 650], [104]]
    words += [[105, t] for t in range(0, 900, 3)]
    trie = Trie(2, words)
    g = torch.Generator().manual_seed(seed)
    lg = (torch.randn(B, ldl, generator=g) * 2).to(torch.bfloat16)
    lg[0, 500] = 50.0                                                  # the row's global maximum is no child
    lg[2, 1010] = 60.0                                                 # a child >= V
    lg[3, 1001] = 50.0                                                 # a child in the special range
    lg[3, 7] = lg[3, 300] = lg[3, 650] = 12.0                          # tied children
    lg[4, 77] = 70.0                                                   # a leaf emits eos whatever the logits say
    lg[5, 20] = 55.0                                                   # finished earlier: pad, the node stays
    special = range(sp0, sp0 + NSPECIAL)
    cands = tuple(tuple(t for t in trie.get_child_index(trie.at(p)) if t < V and t not in special) for p in TRIE_PATHS)
    assert [len(c) for c in cands] == [3, 1, 2, 3, 1, 3, 300]
    return trie, lg, cands


def trie_reference(b, T, top_k, top_p):
    key = ("trie", b, T, top_k, top_p)
    if key not in _refs:
        _, lg, cands = trie_case()
        _refs[key] = topp_reference(lg[b].double().numpy(), cands[b], T, top_k, top_p, 0.5)
    return _refs[key]


# ------------------------------------------------------------------------------------------------ the frequency case
FREQ_IDS, FREQ_LOGITS, FREQ_TOPK, FREQ_TOPP = (17, 100, 333, 640, 900, 1005), (3.0, 2.5, 2.0, 1.5, 1.0, 0.0), 6, 0.8


@functools.lru_cache(maxsize=None)
def freq_case():
    """one row (V = 1006 of 1024, special 1000..1004, T = 1) whose top_k = 6 survivors weigh 1, e^-.5, e^-1, ... (W = 2.383): top_p = 0.8 puts
    the limit at 1.906, between S = 1.607 (id 333, stays) and S = 1.975 (id 640, goes).  -> (row [1024] fp32, the reference)"""
    row = torch.full((1024,), -5.0)
    row[list(FREQ_IDS)] = torch.tensor(FREQ_LOGITS)
    ref = topp_reference(row.double().numpy(), candidates(1006, 1000), 1.0, FREQ_TOPK, FREQ_TOPP, 0.5)
    return row, ref


def all_references():
    """the reference of every case the kernel-level GPU tests check"""
    for shape in SHAPES:
        fin = planted_rows(*shape)[1]
        for T, k, p in kernel_cases(shape):
            for b in range(shape[0]):
                if not fin[b]:
                    yield ("rows", shape, b, T, k, p), case_reference(shape, b, T, k, p)
    for T, k, p in kernel_cases(TRIE_SHAPE):
        for b in range(TRIE_SHAPE[0]):
            if not TRIE_FIN[b]:
                yield ("trie", b, T, k, p), trie_reference(b, T, k, p)
    yield ("freq",), freq_case()[1]
