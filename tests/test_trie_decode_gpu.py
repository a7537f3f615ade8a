"""Trie-constrained greedy decoding with the loop on the device: `decode_pick_trie_kernel` against torch + a Python trie walk, the
device loop (eager and replayed from a hipGraph) against the host loop token for token, the reference's own trie-constrained
generate() output (fixture G9) through the device loop, and the cases that keep the host loop."""
import functools
import types

import numpy as np
import pytest
import torch

from util import gold, T, tiny_cfg, meta_of, hist_lists, GOLDEN_SEED

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


class _Node:
    def __init__(self):
        self.child = {}


class _Trie:
    """tools/trie.py protocol (root / get_child_index / get_next_node); a token that is no child changes nothing"""

    def __init__(self, eos, words=()):
        self.root, self.eos = _Node(), eos
        for w in words:
            self.insert(w)

    def insert(self, word):
        cur = self.root
        for c in word:
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


def _table_walk(off, tok, nxt, path):
    """node id reached from the root along `path` in the flattened table"""
    n = 0
    for c in path:
        e = [e for e in range(off[n], off[n + 1]) if tok[e] == c]
        assert len(e) == 1, (path, c)
        n = int(nxt[e[0]])
    return n


def test_trie_pick_kernel_vs_torch_and_a_python_trie_walk():
    """nv_decode_pick_trie_bf16: the masked argmax of nv_decode_pick_bf16 over the children of each row's node only, the row's move
    along the picked edge, and HF's finished/pad bookkeeping -- against torch.argmax on the CPU over the logits masked by a Python
    walk of the same trie."""
    from navillm_amd import ops, lib
    from navillm_amd.kvcache import flatten_trie
    L = ops._L()
    B, V, Vp, eos, pad = 7, 1006, 1024, 2, 1005
    sp0, nsp = 1000, 5
    special = range(sp0, sp0 + nsp)
    words = [[100, 10], [100, 20], [100, 30],                   # row 0 / row 5: plain children
             [101, 1001], [101, 40], [101, 41],                 # row 1: one child is a special id
             [102, 1010], [102, 50], [102, 51],                 # row 2: one child lies beyond the vocabulary
             [103, 7], [103, 300], [103, 650], [103, 9],        # row 3: three children tie
             [104]]                                             # row 4: a leaf
    words += [[105, t] for t in range(3000)]                    # row 6: 3 000 children (those >= V can never be picked)
    trie = _Trie(eos, words)
    off, tok, nxt, eligible = flatten_trie(trie, eos, V, special)
    assert eligible and off[_table_walk(off, tok, nxt, [105]) + 1] - off[_table_walk(off, tok, nxt, [105])] == 3000
    paths = [[100], [101], [102], [103], [104], [100], [105]]
    g = torch.Generator().manual_seed(3)
    lg = (torch.randn(B, Vp, generator=g) * 2).to(torch.bfloat16)
    lg[0, 500] = 50.0                         # the row's global maximum is no child
    lg[1, 1001] = 50.0                        # a child in the special range holds the maximum of the children: skipped
    lg[2, 1010] = 60.0                        # a child >= V: skipped
    lg[3, 7] = lg[3, 300] = lg[3, 650] = 40.0   # ties -> smallest id
    lg[3, 9] = 39.0
    lg[4, 77] = 70.0                          # a leaf emits eos whatever the logits say
    lg[5, 20] = 55.0                          # finished earlier: pad, the node stays
    lg[6, 767] = 45.0                         # edge 767 of 3 000: the last lane of the last wave, on its third trip through the stride loop
    lg[6, 1001] = 80.0
    lg[6, 2] = -30.0
    n_state = L.nv_decode_state_ints(B)
    node0 = [_table_walk(off, tok, nxt, p) for p in paths]
    # reference: torch on the CPU + the trie itself
    want_tok, want_node, want_fin = [], [], []
    for b in range(B):
        if b == 5:
            want_tok.append(pad), want_node.append(node0[b]), want_fin.append(1)
            continue
        cur = trie.at(paths[b])
        kids = [t for t in trie.get_child_index(cur) if t < V]
        ref = lg[b, :V].float().clone()
        ref[sp0:sp0 + nsp] = float("-inf")
        masked = torch.full_like(ref, float("-inf"))
        masked[kids] = ref[kids]
        t = int(masked.argmax())
        want_tok.append(t)
        want_node.append(_table_walk(off, tok, nxt, paths[b] + [t]) if cur.child else node0[b])
        want_fin.append(int(t == eos))
    assert want_tok[:5] == [int(max((10, 20, 30), key=lambda t: float(lg[0, t]))), int(max((40, 41), key=lambda t: float(lg[1, t]))),
                            int(max((50, 51), key=lambda t: float(lg[2, t]))), 7, eos] and want_tok[6] == 767
    lgd = lg.to(DEV)

    def run(tables, cnt, max_steps, nodes, fin5=1):
        off_d, tok_d, nxt_d = (torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in tables)
        st = torch.zeros(n_state, dtype=torch.int32)
        st[B + 5] = fin5
        st[7 * B + 2] = cnt
        std = st.to(DEV)
        node = torch.tensor(nodes, dtype=torch.int32, device=DEV)
        out = torch.full((4, B), -1, dtype=torch.int32, device=DEV)
        lib.check(L.nv_decode_pick_trie_bf16(lgd.data_ptr(), Vp, V, sp0, nsp, off_d.data_ptr(), tok_d.data_ptr(), nxt_d.data_ptr(),
                                             tables[0].size - 1, node.data_ptr(), std.data_ptr(), out.data_ptr(), max_steps, B, eos, pad,
                                             ops._st()), "pick_trie")
        torch.cuda.synchronize()
        return std.cpu(), node.cpu().tolist(), out.cpu()

    s, node, out = run((off, tok, nxt), 1, 4, node0)
    assert s[:B].tolist() == want_tok and s[B:2 * B].tolist() == want_fin and node == want_node
    assert out[1].tolist() == want_tok and bool((out[[0, 2, 3]] == -1).all())
    assert s[2 * B:].tolist() == [0] * (5 * B + 2) + [1, 0]          # nothing else of the state moves
    # cnt == max_steps: the token still reaches tok[], nothing is written to out
    s, node, out = run((off, tok, nxt), 4, 4, node0)
    assert s[:B].tolist() == want_tok and node == want_node and bool((out == -1).all())
    # a node without a pickable child (kvcache.py never sends one): `eos`, the row finishes, the node stays; so does a node id
    # outside the table -- and neither reads or writes out of bounds
    t2 = _Trie(eos, [[5, 1002], [5, 1003], [6, 8]])
    off2, tok2, nxt2, ok2 = flatten_trie(t2, eos, V, special)
    assert not ok2
    dead = _table_walk(off2, tok2, nxt2, [5])
    nodes2 = [dead, off2.size - 1, -3, 0, 0, 0, 0]
    s, node, out = run((off2, tok2, nxt2), 0, 4, nodes2, fin5=0)
    assert s[:3].tolist() == [eos] * 3 and s[B:B + 3].tolist() == [1, 1, 1] and node[:3] == nodes2[:3]
    assert s[3:B].tolist() == [max((5, 6), key=lambda t: float(lg[b, t])) for b in range(3, B)]


def _mid_cfg(layers, heads):
    from navillm_amd import config as nvcfg
    return nvcfg.NavConfig(hidden_size=512, num_layers=layers, num_heads=heads, intermediate_size=1408, base_vocab_size=1000,
                           enc_hidden_size=256, enc_num_heads=4, enc_intermediate_size=512, image_feat_size=768)


@functools.lru_cache(maxsize=None)
def _model(heads):
    from navillm_amd.nav_model import NavModel
    m = NavModel(nav_config=_mid_cfg(3, heads), device=torch.device(DEV), seed=11)
    m.eval()
    return m


@functools.lru_cache(maxsize=None)
def _case(heads, B=4):
    """the model, prompts of different lengths with <cand> / <hist> tokens and their visual rows (test_kvcache_gpu._gen_case)"""
    m = _model(heads)
    cfg = m.cfg
    g = torch.Generator().manual_seed(321)
    ids_l, n_c, n_h = [], 0, 0
    for b in range(B):
        ids = torch.randint(3, cfg.base_vocab_size, (40 + 17 * b,), generator=g).tolist()
        ids[0] = 1
        for j in (5, 9 + b):
            ids[j] = cfg.cand_token_id
            n_c += 1
        ids[20] = cfg.hist_token_id
        n_h += 1
        ids_l.append(ids)
    S = max(len(x) for x in ids_l)
    ids_t = torch.full((B, S), cfg.pad_token_id, dtype=torch.int64)
    am = torch.zeros((B, S), dtype=torch.int64)
    for b, x in enumerate(ids_l):
        ids_t[b, S - len(x):] = torch.tensor(x)
        am[b, S - len(x):] = 1
    cand = torch.randn(n_c, cfg.hidden_size, generator=g) * 0.5
    hist = torch.randn(n_h, cfg.hidden_size, generator=g) * 0.5
    ids_l, vix_l, vis_all, _ = m._vis_layout(ids_t, am, cand.to(DEV), hist.to(DEV), None)
    return m, ids_l, vix_l, vis_all


def _words(n, seed, vocab, eos):
    """n random words of 1-6 tokens: about half of them continue a prefix of an earlier word, a third end in an explicit eos"""
    rng = np.random.RandomState(seed)
    words = []
    for _ in range(n):
        w = rng.randint(3, vocab, size=rng.randint(1, 7)).tolist()
        if words and rng.rand() < 0.5:
            p = [t for t in words[rng.randint(len(words))] if t != eos]
            w = (p[:rng.randint(1, 6)] + w)[:6]
        if rng.rand() < 0.33:
            w = w[:5] + [eos]
        words.append(w)
    return words


def _assert_paths(trie, rows, eos, pad):
    for b, row in enumerate(rows):
        node, done = trie.root, False
        for t in row:
            if done:
                assert t == pad, (b, row)
                continue
            assert t in trie.get_child_index(node), (b, t, row)
            if t == eos:
                done = True
            else:
                node = trie.get_next_node(node, t)


EOS, PAD = 2, 0


@pytest.mark.parametrize("heads", [4, 8])            # head_dim 128 and 64
def test_trie_device_loop_equals_host_loop(monkeypatch, heads):
    """trie-constrained greedy decoding with the pick, the trie walk and the bookkeeping on the device (eager, and replayed from a
    hipGraph) == the host loop, token for token, rows that finish at different steps included; a repeated call replays the graph; a
    larger trie (the device tables are reallocated) and an unconstrained call on the same KVCacheLM equal their host results; the
    cache bookkeeping stays consistent."""
    import navillm_amd.kvcache as kvm
    from navillm_amd.kvcache import KVCacheLM
    m, ids_l, vix_l, vis_all = _case(heads)
    cfg = m.cfg
    B = len(ids_l)
    trie = _Trie(EOS, _words(40, 7, cfg.base_vocab_size, EOS))
    big = _Trie(EOS, _words(600, 8, cfg.base_vocab_size, EOS))
    runs = {}
    for tag, dev_loop, graph in (("host", False, False), ("device", True, False), ("graph", True, True)):
        monkeypatch.setattr(kvm, "DEVICE_GREEDY", dev_loop)
        monkeypatch.setattr(kvm, "USE_HIP_GRAPH", graph)
        loop = "device" if dev_loop else "host"
        kv = KVCacheLM(m, B, capacity=256)
        gen = lambda t, n=12, eos=EOS: kv.generate(ids_l, vix_l, vis_all, max_new_tokens=n, eos_token_id=eos, pad_token_id=PAD, trie=t)
        a = gen(trie)
        assert kv.last_generate == {"loop": loop, "trie": True}
        b = gen(trie)                                              # graph reuse
        assert a == b and kv.last_generate == {"loop": loop, "trie": True}
        _assert_paths(trie, a, EOS, PAD)
        tables = None if not dev_loop else (kv._trie_dev["off"].data_ptr(), kv._trie_dev["tok"].data_ptr())
        c = gen(big)                                               # more nodes and edges than the tables hold: they are reallocated
        assert kv.last_generate == {"loop": loop, "trie": True}
        _assert_paths(big, c, EOS, PAD)
        if dev_loop:
            assert tables != (kv._trie_dev["off"].data_ptr(), kv._trie_dev["tok"].data_ptr())
        a2 = gen(trie)                                             # back to the first trie, now in the larger tables
        assert a2 == a
        f = gen(None, 5, -7)                                       # unconstrained, on the same object: its own graph
        assert kv.last_generate == {"loop": loop, "trie": False} and all(len(x) == 5 for x in f)
        a3 = gen(trie)                                             # ... and the trie graph is still the trie graph
        assert a3 == a
        f2 = gen(None, 5, -7)
        assert f2 == f
        runs[tag] = (a, c, f)
        # the cache bookkeeping stays consistent: a following extend() of prompt + generated tokens reuses everything but the last token
        seqs = [list(ids_l[i]) + f[i] for i in range(B)]
        vix = [list(vix_l[i]) + [-1] * len(f[i]) for i in range(B)]
        keys = [("gen", r) for r in range(vis_all.shape[0])]
        kv.extend(seqs, vix, vis_all, keys)
        if dev_loop:
            assert kv.last_stats["new"] == [1] * B, kv.last_stats
    print("host  :", runs["host"][0])
    print("graph :", runs["graph"][0])
    assert runs["host"] == runs["device"] == runs["graph"]
    ends = [[row.index(EOS) for row in runs["host"][k]] for k in (0, 1)]
    assert len(set(ends[0])) > 1 or len(set(ends[1])) > 1, ends   # rows finish at different steps: the earlier ones go on with pad


def test_g9_trie_generation_runs_the_device_loop_and_matches_the_reference():
    """fixture G9: `model("summarization", batch, training=False, trie=trie)` returns the token ids the reference's own
    trie-constrained generate() returned -- through the device loop (the G9 trie is eligible: tests/test_trie_decode_cpu.py)."""
    from navillm_amd.nav_model import NavModel
    z = gold("g9_generate_bf16.npz")
    m = NavModel(nav_config=tiny_cfg("bf16"), device=torch.device(DEV), seed=GOLDEN_SEED)
    m.eval()
    meta = meta_of(z)
    words = [[int(c) for c in row if c >= 0] for row in z["trie_words"]]
    trie = _Trie(meta["eos"], words)
    m.lang_model.tokenizer = types.SimpleNamespace(eos_token_id=meta["eos"], unk_token_id=meta["pad"])   # ids only: prompts are pre-tokenised
    dev = lambda x: T(x).to(DEV)
    B = z["sum_input_ids"].shape[0]
    m.enable_kv_cache(B, capacity=(z["sum_input_ids"].shape[1] + 50 + 127) // 128 * 128)
    with torch.no_grad():
        ps = m("panorama", dict(view_img_fts=dev(z["sum_view_img_fts"]), view_lens=dev(z["sum_view_lens"]), loc_fts=dev(z["sum_loc_fts"]),
                                nav_types=dev(z["sum_nav_types"])))
        vp = torch.cat([torch.zeros_like(ps["pano_embeds"][:, :1]), ps["pano_embeds"]], 1)
        hv = hist_lists(dev(z["sum_hist_vis_flat"]), meta["hist_t"])
        sm = m("summarization", dict(vp_img_embeds=vp, vp_nav_masks=T(z["sum_vp_nav_masks"]), instruction=["x"] * B, answer=[""] * B,
                                     hist_vis=hv, data_type=["r2r"] * B, input_ids=T(z["sum_input_ids"]),
                                     attention_mask=T(z["sum_attention_mask"])), training=False, trie=trie)
    assert sm["generated_ids"] == z["sum_new_ids"].tolist(), (sm["generated_ids"], z["sum_new_ids"].tolist())
    assert m.kv.last_generate == {"loop": "device", "trie": True}


def test_trie_calls_that_keep_the_host_loop(monkeypatch):
    """an ineligible trie (a node whose only child is a special id), do_sample=True and prompt + max_new_tokens > capacity report
    the host loop, with the output of the host loop"""
    import navillm_amd.kvcache as kvm
    from navillm_amd.kvcache import KVCacheLM
    m, ids_l, vix_l, vis_all = _case(4)
    cfg = m.cfg
    B = len(ids_l)
    words = _words(40, 7, cfg.base_vocab_size, EOS)
    trie = _Trie(EOS, words)
    bad = _Trie(EOS, words + [[999, cfg.special_token_ids[0]]])
    cases = {"ineligible": (256, dict(trie=bad)), "sample": (256, dict(trie=trie, do_sample=True, temperature=0.7)),
             "capacity": (100, dict(trie=trie))}
    got = {}
    for dev_loop in (False, True):
        monkeypatch.setattr(kvm, "DEVICE_GREEDY", dev_loop)
        for name, (cap, kw) in cases.items():
            kv = KVCacheLM(m, B, capacity=cap)
            torch.manual_seed(5)
            got[name, dev_loop] = kv.generate(ids_l, vix_l, vis_all, max_new_tokens=12, eos_token_id=EOS, pad_token_id=PAD, **kw)
            assert kv.last_generate == {"loop": "host", "trie": True}, (name, dev_loop)
            _assert_paths(kw["trie"], got[name, dev_loop], EOS, PAD)
    for name in cases:
        assert got[name, False] == got[name, True], name
    # (the same calls minus what sends them to the host loop DO run on the device)
    kv = KVCacheLM(m, B, capacity=256)
    _assert_paths(trie, kv.generate(ids_l, vix_l, vis_all, max_new_tokens=12, eos_token_id=EOS, pad_token_id=PAD, trie=trie), EOS, PAD)
    assert kv.last_generate == {"loop": "device", "trie": True}
