"""CPU: the host half of trie-constrained decoding on the device -- `kvcache.flatten_trie` (the trie as three int32 arrays, built
through the tools/trie.py protocol alone) and the argument checks of `nv_decode_pick_trie_bf16`.  No kernel is launched here."""
from collections import defaultdict

import numpy as np

from util import gold, meta_of, tiny_cfg


class _Node:
    def __init__(self):
        self.child = {}


class _WordTrie:
    """tools/trie.py protocol over a word list, without side effects (like test_oracle_golden._GoldTrie)"""

    def __init__(self, words, eos):
        self.root, self.eos = _Node(), eos
        for w in words:
            cur = self.root
            for c in w:
                cur = cur.child.setdefault(int(c), _Node())

    def get_child_index(self, cur):
        return [self.eos] if not cur.child else list(cur.child.keys())

    def get_next_node(self, cur, w):
        return cur if not cur.child else cur.child[int(w)]


class _InsertingNode:
    def __init__(self):
        self.child = defaultdict(_InsertingNode)


class _InsertingTrie:
    """the reference's tools/trie.py behaviour: `get_next_node` INSERTS a node when the token is no child"""

    def __init__(self, words, eos):
        self.root, self.eos = _InsertingNode(), eos
        for w in words:
            cur = self.root
            for c in w:
                cur = cur.child[int(c)]

    def get_child_index(self, cur):
        return [self.eos] if len(cur.child) == 0 else list(cur.child.keys())

    def get_next_node(self, cur, w):
        return cur if len(cur.child) == 0 else cur.child[w]


def _count(node):
    return 1 + sum(_count(c) for c in node.child.values())


def _check_walk(trie, eos, V, special):
    """the table, walked from node 0 alongside the trie, says what the protocol says at every reachable node"""
    from navillm_amd.kvcache import flatten_trie
    off, tok, nxt, eligible = flatten_trie(trie, eos, V, special)
    assert off.dtype == tok.dtype == nxt.dtype == np.int32
    N = off.size - 1
    assert off[0] == 0 and off[-1] == tok.size == nxt.size and bool((np.diff(off) >= 1).all())
    assert bool(((nxt >= 0) & (nxt < N)).all())
    seen, todo = {0: trie.root}, [0]
    while todo:
        n = todo.pop()
        node = seen[n]
        e0, e1 = int(off[n]), int(off[n + 1])
        kids = tok[e0:e1].tolist()
        assert kids == sorted(set(trie.get_child_index(node))), n           # the node's children, sorted by token id
        if not node.child:                                                  # a leaf: the one edge eos -> itself
            assert kids == [eos] and nxt[e0] == n
        for e in range(e0, e1):
            child = trie.get_next_node(node, int(tok[e]))
            j = int(nxt[e])
            if j in seen:
                assert seen[j] is child
            else:
                seen[j] = child
                todo.append(j)
    assert len(seen) == N == _count(trie.root)                              # every node of the table is reachable, none is missing
    return off, tok, nxt, eligible


def test_flatten_trie_walk_reproduces_the_protocol_on_the_g9_trie_and_a_random_trie():
    z = gold("g9_generate_bf16.npz")
    m = meta_of(z)
    cfg = tiny_cfg("bf16")
    words = [[int(c) for c in row if c >= 0] for row in z["trie_words"]]
    *_, eligible = _check_walk(_WordTrie(words, m["eos"]), m["eos"], cfg.vocab_size, cfg.special_token_ids)
    assert eligible                                   # the G9 summarization trie may take the device loop (the GPU pin relies on it)
    # random: shared prefixes, words that are prefixes of other words, words ending in an explicit eos
    rng = np.random.RandomState(5)
    eos, V, special = 2, 200, range(190, 195)
    words = []
    for _ in range(60):
        w = rng.randint(3, 40, size=rng.randint(1, 7)).tolist()
        if words and rng.rand() < 0.5:
            p = words[rng.randint(len(words))]
            w = [t for t in p if t != eos][:rng.randint(1, 6)] + w[:rng.randint(0, 3)]       # shares a prefix / IS a prefix
        if rng.rand() < 0.4:
            w = w + [eos]
        words.append(w)
    words.append(words[0][:1])
    off, tok, nxt, eligible = _check_walk(_WordTrie(words, eos), eos, V, special)
    assert eligible and off.size - 1 > 60


def test_flatten_trie_leaves_an_inserting_trie_with_the_nodes_it_had():
    from navillm_amd.kvcache import flatten_trie
    eos = 2
    words = [[5, 6, 7], [5, 6, 8, eos], [5, 9], [11], [11, 12]]
    trie = _InsertingTrie(words, eos)
    before = _count(trie.root)
    off, tok, nxt, eligible = flatten_trie(trie, eos, 100, range(90, 95))
    assert _count(trie.root) == before == off.size - 1 and eligible
    _check_walk(trie, eos, 100, range(90, 95))
    assert _count(trie.root) == before
    # (and a miss really inserts: the protection is in the flattening, not in the trie)
    trie.get_next_node(trie.root, 77)
    assert _count(trie.root) == before + 1


def test_flatten_trie_eligibility():
    """a node whose children are ALL special or >= V has no pickable child: such a trie keeps the host loop"""
    from navillm_amd.kvcache import flatten_trie
    eos, V, special = 2, 100, range(90, 95)
    good = [[5, 6], [5, 7, eos], [8, 91], [8, 9], [10, 120], [10, 11]]       # special / out-of-vocabulary children NEXT TO pickable ones
    assert flatten_trie(_WordTrie(good, eos), eos, V, special)[3] is True
    bad = [4, 92, 13]                                                       # node [4]: the only child is special
    assert flatten_trie(_WordTrie(good + [bad], eos), eos, V, special)[3] is False
    bad2 = [4, 100]                                                         # ... the only child is >= V
    assert flatten_trie(_WordTrie(good + [bad2], eos), eos, V, special)[3] is False
    assert flatten_trie(_WordTrie(good + [bad2, [4, 92], [4, 93]], eos), eos, V, special)[3] is False
    assert flatten_trie(_WordTrie(good + [[4, 92], [4, 14]], eos), eos, V, special)[3] is True
    # eos itself outside the pickable set makes every leaf ineligible
    assert flatten_trie(_WordTrie(good, 93), 93, V, special)[3] is False


def test_trie_pick_refuses_bad_arguments_before_any_launch():
    from navillm_amd import lib
    L = lib.load()
    one = 1 << 12                                     # any non-null pointer value: an argument error returns before it is used
    args = dict(logits=one, ldl=1024, V=1006, special0=1000, nspecial=5, off=one, tok=one, nxt=one, n_nodes=3, node=one, state=one, out=one,
                max_steps=4, B=7, eos=2, pad=0, stream=None)
    for k in ("logits", "off", "tok", "nxt", "node", "state", "out"):
        a = dict(args)
        a[k] = None
        assert L.nv_decode_pick_trie_bf16(*a.values()) == -1, k
    for k, v in (("B", 0), ("B", -2), ("V", 0), ("ldl", 1000), ("n_nodes", 0), ("max_steps", -1), ("nspecial", -1)):
        a = dict(args)
        a[k] = v
        assert L.nv_decode_pick_trie_bf16(*a.values()) == -1, (k, v)
    assert L.nv_decode_pick_trie_bf16(None, 0, 0, 0, 0, None, None, None, 0, None, None, None, 0, 0, 0, 0, None) == -1
    assert L.nv_decoder_trie_step(*([None] * 4), 0, 0, 0, 0, None, None, None, 0, None, None, None, None, None, 0, None, None, None,
                                  0, 0, 0, 0, None, 0, None) == -1
