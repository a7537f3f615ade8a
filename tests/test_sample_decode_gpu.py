"""Temperature / top-k sampled decoding with the loop on the device: `decode_pick_sample_kernel` (unconstrained and over the
children of a trie node) against the fp64 reference and the numpy Philox of tests/sample_ref.py, the frequencies of 4 096 draws,
`KVCacheLM.generate(do_sample=True)` under NAVILLM_DEVICE_SAMPLE end to end (eager and replayed from a hipGraph), and the calls that
keep the host loop.

EPS = 1e-5 is the allowance of the CDF check for the kernel's fp32 sums (at most 32 sequential adds per thread, a 1024-wide scan,
expf): an fp32 emulation of that order against fp64 gave at most 7.3e-7."""
import functools

import numpy as np
import pytest
import torch

from sample_ref import philox_u, sample_reference, check_draw

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-5
SEED, OFFSET = 0x123456789abcdef1, (1 << 32) - 5          # the counter crosses into its high word within the first rows
TEMPS, TOPKS, CNTS = (0.01, 0.7, 1.0), (0, 1, 50, None), (0, 3)       # top_k None: V + 5
MAX_STEPS = 4


class _Node:
    def __init__(self):
        self.child = {}


class _Trie:
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


def _table_walk(off, tok, nxt, path):
    n = 0
    for c in path:
        e = [e for e in range(off[n], off[n + 1]) if tok[e] == c]
        assert len(e) == 1, (path, c)
        n = int(nxt[e[0]])
    return n


def _launch(lgd, ldl, V, sp0, nsp, tables, nodes, T, top_k, cnt, fin, eos, pad, max_steps=MAX_STEPS, seed=SEED, offset=OFFSET,
            out=None, u_out=None):
    """one nv_decode_pick_sample_bf16 launch on a fresh state -> (state, node, out, u_out) on the host"""
    from navillm_amd import ops, lib
    L = ops._L()
    B = lgd.shape[0]
    st = torch.zeros(L.nv_decode_state_ints(B), dtype=torch.int32)
    st[B:2 * B] = torch.tensor(fin, dtype=torch.int32)
    st[7 * B + 2] = cnt
    std = st.to(DEV)
    rng = torch.from_numpy(np.array([seed, offset], dtype=np.uint64).view(np.int64)).to(DEV)
    out = torch.full((max_steps, B), -1, dtype=torch.int32, device=DEV) if out is None else out
    u_out = torch.full((max_steps * B,), -1.0, dtype=torch.float32, device=DEV) if u_out is None else u_out
    tr, node = (None, None, None, 0, None), None
    if tables is not None:
        td = [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in tables]
        node = torch.tensor(nodes, dtype=torch.int32, device=DEV)
        tr = (td[0].data_ptr(), td[1].data_ptr(), td[2].data_ptr(), tables[0].size - 1, node.data_ptr())
    lib.check(L.nv_decode_pick_sample_bf16(lgd.data_ptr(), ldl, V, sp0, nsp, *tr, T, top_k, rng.data_ptr(), u_out.data_ptr(), std.data_ptr(),
                                           out.data_ptr(), max_steps, B, eos, pad, ops._st()), "pick_sample")
    torch.cuda.synchronize()
    return std.cpu(), (None if node is None else node.cpu().tolist()), out.cpu(), u_out.cpu().numpy()


def _check_launch(res, lg64, cands, T, top_k, cnt, fin, eos, pad, refs):
    """the assertions shared by the unconstrained and the trie test; -> the tokens.  `refs` caches the reference's kept set and CDF
    per (row, T, top_k): they do not depend on u"""
    s, _, out, u_out = res
    B = lg64.shape[0]
    u = philox_u(SEED, OFFSET + cnt * B + np.arange(B))
    if cnt < MAX_STEPS:
        assert u_out[cnt * B:(cnt + 1) * B].view(np.uint32).tolist() == u.view(np.uint32).tolist()       # bit for bit
        assert bool((np.delete(u_out, np.arange(cnt * B, (cnt + 1) * B)) == -1.0).all())
    else:
        assert bool((u_out == -1.0).all())
    toks = s[:B].tolist()
    worst = 0.0
    for b in range(B):
        if fin[b]:
            assert toks[b] == pad and s[B + b] == 1, b
            continue
        key = (b, T, top_k)
        if key not in refs:
            refs[key] = sample_reference(lg64[b], cands[b], T, top_k, 0.5)
        ref = refs[key]
        if ref["token"] is None:
            assert toks[b] == eos and s[B + b] == 1, (b, toks[b])
            continue
        worst = max(worst, check_draw(ref, toks[b], u[b], EPS))
        assert s[B + b] == int(toks[b] == eos), b
    assert s[2 * B:].tolist() == [0] * (5 * B + 2) + [cnt, 0]              # nothing else of the state moves
    if cnt < MAX_STEPS:
        assert out[cnt].tolist() == toks and bool((np.delete(out.numpy(), cnt, axis=0) == -1).all())
    else:
        assert bool((out == -1).all())
    if worst > 0:
        print(f"u outside the token's fp64 CDF interval by {worst:.2e} (T={T}, top_k={top_k}, cnt={cnt})")
    return toks


def _planted_rows(B, V, ldl, sp0, nsp, seed):
    """randn * 2 in bf16 with, by row % 7: 0 the row maximum inside the special range; 1 the row maximum at an id >= V; 2 48 distinct
    large values and a three-way tie right below them (the 49th..51st largest: the tie sits exactly at top_k = 50), the tied ids in
    front so that dropping one would shift every CDF interval behind it; 3 finished earlier; 4 every candidate at -inf; 5 a three-way
    tie for the maximum (the tie at top_k = 1); 6 a NaN and a -inf among ordinary candidates"""
    g = torch.Generator().manual_seed(seed)
    lg = (torch.randn(B, ldl, generator=g) * 2).to(torch.bfloat16)
    fin = [0] * B
    for b in range(B):
        k = b % 7
        if k == 0:
            lg[b, sp0 + 1] = 50.0
        elif k == 1:
            lg[b, V + 2] = 60.0
        elif k == 2:
            lg[b, 5] = lg[b, 9] = lg[b, V - 1] = 12.0
            lg[b, torch.arange(48) * 17 + 40] = 12.0 + (torch.arange(48) + 1).to(torch.bfloat16) * 0.0625      # 12.0625 .. 15.0, exact in bf16
        elif k == 3:
            fin[b] = 1
        elif k == 4:
            lg[b, :V] = float("-inf")
            lg[b, sp0] = 3.0
        elif k == 5:
            lg[b, 7] = lg[b, 300] = lg[b, V - 20] = 14.0               # (V - 20 lies below both special ranges)
        else:
            lg[b, 11] = float("nan")
            lg[b, 12] = float("-inf")
            lg[b, 13] = 9.0
    return lg, fin


@pytest.mark.parametrize("B,V,ldl,sp0", [(7, 1006, 1024, 1000), (3, 9001, 9008, 8990), (7, 1006, 1011, 1000)],
                         ids=["V1006", "V9001_several_ids_per_thread", "ldl_no_multiple_of_8"])
def test_sample_pick_kernel_vs_the_fp64_reference(B, V, ldl, sp0):
    """nv_decode_pick_sample_bf16 without a trie: the uniform equals the numpy Philox bit for bit, the token is a kept candidate of
    non-zero weight whose fp64 CDF interval holds u (within EPS), finished rows emit pad, a row of -inf candidates emits eos, the rest
    of the state does not move, and nothing reaches `out` at cnt == max_steps."""
    nsp, eos, pad = 5, 2, V - 1
    lg, fin = _planted_rows(B, V, ldl, sp0, nsp, 3)
    lg64 = lg.double().numpy()
    cands = [[v for v in range(V) if not sp0 <= v < sp0 + nsp]] * B
    lgd = lg.to(DEV)
    refs, seen = {}, set()
    for T in TEMPS:
        for k in TOPKS:
            top_k = V + 5 if k is None else k
            for cnt in CNTS:
                res = _launch(lgd, ldl, V, sp0, nsp, None, None, T, top_k, cnt, fin, eos, pad)
                toks = _check_launch(res, lg64, cands, T, top_k, cnt, fin, eos, pad, refs)
                seen.update((b, t) for b, t in enumerate(toks))
    assert len(refs[2, 1.0, 50]["ids"]) == 51 and len(refs[2, 1.0, 1]["ids"]) == 1         # the planted tie at the 50th value is kept whole
    if B > 5:
        assert len(refs[5, 1.0, 1]["ids"]) == 3 and refs[4, 1.0, 0]["token"] is None and 11 not in refs[6, 1.0, 0]["ids"]
        assert len({t for b, t in seen if b == 5}) > 1                                   # the tied maxima are drawn, not only the first
    assert all(t != sp0 + 1 for b, t in seen if b == 0) and all(t < V for _, t in seen)
    # cnt == max_steps: the token still reaches tok[], nothing is written to out or u_out
    res = _launch(lgd, ldl, V, sp0, nsp, None, None, 0.7, 50, MAX_STEPS, fin, eos, pad)
    _check_launch(res, lg64, cands, 0.7, 50, MAX_STEPS, fin, eos, pad, refs)
    # equal (logits, rng, cnt) give equal tokens; another offset gives other uniforms
    a = _launch(lgd, ldl, V, sp0, nsp, None, None, 1.0, 0, 1, fin, eos, pad)
    b = _launch(lgd, ldl, V, sp0, nsp, None, None, 1.0, 0, 1, fin, eos, pad)
    c = _launch(lgd, ldl, V, sp0, nsp, None, None, 1.0, 0, 1, fin, eos, pad, offset=OFFSET + 1000)
    assert a[0].tolist() == b[0].tolist() and a[3].tolist() == b[3].tolist() and a[3].tolist() != c[3].tolist()


def test_sample_pick_kernel_with_a_trie():
    """the same over the children of each row's trie node (the trie of test_trie_pick_kernel_vs_torch_and_a_python_trie_walk): a special
    child, a child >= V, tied children, a leaf, a finished row, the 3 000-child node; the node moves along the picked edge, a
    finished row's node stays; a dead node and a node id outside the table emit eos."""
    from navillm_amd.kvcache import flatten_trie
    B, V, Vp, eos, pad = 7, 1006, 1024, 2, 1005
    sp0, nsp = 1000, 5
    special = range(sp0, sp0 + nsp)
    words = [[100, 10], [100, 20], [100, 30], [101, 1001], [101, 40], [101, 41], [102, 1010], [102, 50], [102, 51],
             [103, 7], [103, 300], [103, 650], [103, 9], [104]]
    words += [[105, t] for t in range(3000)]
    trie = _Trie(eos, words)
    off, tok, nxt, eligible = flatten_trie(trie, eos, V, special)
    assert eligible
    paths = [[100], [101], [102], [103], [104], [100], [105]]
    fin = [0, 0, 0, 0, 0, 1, 0]
    g = torch.Generator().manual_seed(3)
    lg = (torch.randn(B, Vp, generator=g) * 2).to(torch.bfloat16)
    lg[0, 500] = 50.0                         # the row's global maximum is no child
    lg[1, 1001] = 50.0                        # a child in the special range
    lg[2, 1010] = 60.0                        # a child >= V
    lg[3, 7] = lg[3, 300] = lg[3, 650] = 40.0   # tied children (kept together by top_k = 1)
    lg[3, 9] = 39.0
    lg[4, 77] = 70.0                          # a leaf emits eos whatever the logits say
    lg[5, 20] = 55.0                          # finished earlier: pad, the node stays
    lg[6, 1001] = 80.0
    lg[6, 2] = -30.0
    lg64 = lg.double().numpy()
    node0 = [_table_walk(off, tok, nxt, p) for p in paths]
    cands = [[t for t in trie.get_child_index(trie.at(p)) if t < V and t not in special] for p in paths]
    assert [len(c) for c in cands] == [3, 2, 2, 4, 1, 3, 1001]
    lgd = lg.to(DEV)
    refs, seen = {}, set()
    for T in TEMPS:
        for k in TOPKS:
            top_k = V + 5 if k is None else k
            for cnt in CNTS:
                res = _launch(lgd, Vp, V, sp0, nsp, (off, tok, nxt), node0, T, top_k, cnt, fin, eos, pad)
                toks = _check_launch(res, lg64, cands, T, top_k, cnt, fin, eos, pad, refs)
                want = [node0[b] if (fin[b] or not trie.at(paths[b]).child) else _table_walk(off, tok, nxt, paths[b] + [toks[b]]) for b in range(B)]
                assert res[1] == want, (T, top_k, cnt)
                assert toks[4] == eos and toks[5] == pad
                seen.update((b, t) for b, t in enumerate(toks))
    assert len(refs[3, 1.0, 1]["ids"]) == 3 and len({t for b, t in seen if b == 3}) > 1
    assert len({t for b, t in seen if b == 6}) > 3                       # the 3 000-child node: several different draws
    res = _launch(lgd, Vp, V, sp0, nsp, (off, tok, nxt), node0, 0.7, 50, MAX_STEPS, fin, eos, pad)
    _check_launch(res, lg64, cands, 0.7, 50, MAX_STEPS, fin, eos, pad, refs)
    # a node without a pickable child (kvcache.py never sends one) and node ids outside the table: eos, the row finishes, the node stays
    t2 = _Trie(eos, [[5, 1002], [5, 1003], [6, 8]])
    off2, tok2, nxt2, ok2 = flatten_trie(t2, eos, V, special)
    assert not ok2
    dead = _table_walk(off2, tok2, nxt2, [5])
    nodes2 = [dead, off2.size - 1, -3, 0, 0, 0, 0]
    s, node, out, _ = _launch(lgd, Vp, V, sp0, nsp, (off2, tok2, nxt2), nodes2, 1.0, 0, 0, [0] * B, eos, pad)
    assert s[:3].tolist() == [eos] * 3 and s[B:B + 3].tolist() == [1, 1, 1] and node[:3] == nodes2[:3]
    assert all(t in (5, 6) for t in s[3:B].tolist()) and s[2 * B:].tolist() == [0] * (5 * B + 2) + [0, 0]
    assert node[3:] == [_table_walk(off2, tok2, nxt2, [t]) for t in s[3:B].tolist()]


def test_sample_draw_frequencies():
    """64 identical rows with six kept candidates (top_k = 6) of known probabilities, drawn at cnt = 0..63: every one of the 4 096
    uniforms is another one (counters are not reused: with this seed the numpy Philox says so too -- 24-bit uniforms of a seed picked
    at random collide with probability 0.4), and every frequency lies within 5 sigma of its binomial expectation."""
    from navillm_amd import ops
    B, V, Vp, eos, pad, steps = 64, 1006, 1024, 2, 0, 64
    seed = 20243
    ids = [17, 100, 333, 640, 900, 1005]
    row = torch.full((Vp,), -5.0)
    row[ids] = torch.tensor([3.0, 2.5, 2.0, 1.5, 1.0, 0.0])
    lgd = row.to(torch.bfloat16).repeat(B, 1).contiguous().to(DEV)
    ref = sample_reference(row.double().numpy(), [v for v in range(V) if not 1000 <= v < 1005], 1.0, 6, 0.5)
    assert ref["ids"].tolist() == ids
    p = ref["w"] / ref["w"].sum()
    out = torch.full((steps, B), -1, dtype=torch.int32, device=DEV)
    u_out = torch.full((steps * B,), -1.0, dtype=torch.float32, device=DEV)
    for cnt in range(steps):
        _launch(lgd, Vp, V, 1000, 5, None, None, 1.0, 6, cnt, [0] * B, eos, pad, max_steps=steps, seed=seed, offset=0, out=out, u_out=u_out)
    u = u_out.cpu().numpy()
    assert u.view(np.uint32).tolist() == philox_u(seed, np.arange(steps * B)).view(np.uint32).tolist()
    assert len(set(u.tolist())) == steps * B
    toks = out.cpu().numpy().reshape(-1)
    n = toks.size
    freq = np.array([(toks == v).sum() for v in ids])
    print("frequencies", freq.tolist(), "expected", (n * p).round(1).tolist())
    assert freq.sum() == n
    assert bool((np.abs(freq - n * p) <= 5 * np.sqrt(n * p * (1 - p))).all()), (freq, n * p)
    for j in range(n):                                              # ... and every single draw is the reference's (within EPS)
        check_draw(ref, int(toks[j]), u[j], EPS)


# ---------------------------------------------------------------------------------------------------------------- generate()
def _mid_cfg(layers, heads):
    from navillm_amd import config as nvcfg
    return nvcfg.NavConfig(hidden_size=512, num_layers=layers, num_heads=heads, intermediate_size=1408, base_vocab_size=1000,
                           enc_hidden_size=256, enc_num_heads=4, enc_intermediate_size=512, image_feat_size=768)


@functools.lru_cache(maxsize=None)
def _case(B=4):
    """a small model and prompts of different lengths (plain tokens)"""
    from navillm_amd.nav_model import NavModel
    m = NavModel(nav_config=_mid_cfg(3, 4), device=torch.device(DEV), seed=11)
    m.eval()
    g = torch.Generator().manual_seed(321)
    ids_l = [[1] + torch.randint(3, m.cfg.base_vocab_size, (39 + 17 * b,), generator=g).tolist() for b in range(B)]
    return m, ids_l


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


@pytest.mark.parametrize("constrained", [False, True], ids=["free", "trie"])
def test_generate_samples_on_the_device(monkeypatch, constrained):
    """generate(do_sample=True) under DEVICE_SAMPLE: reproducible from torch.manual_seed, eager == hipGraph, other seeds give other
    tokens, tokens are pickable ids (with a trie: paths of the trie, then eos, then pad), `last_sample` records the Philox key,
    outputs of 1, 2 and 3 new tokens under one seed are prefixes of each other and each call's last token is the reference's draw
    from the logits that step saw; temperature 1e-4 gives the greedy tokens (wherever the row maximum is untied)."""
    import navillm_amd.kvcache as kvm
    from navillm_amd.kvcache import KVCacheLM
    m, ids_l = _case()
    cfg = m.cfg
    B, V = len(ids_l), cfg.vocab_size
    special = set(cfg.special_token_ids)
    trie = _Trie(EOS, _words(300, 7, cfg.base_vocab_size, EOS)) if constrained else None
    monkeypatch.setattr(kvm, "DEVICE_SAMPLE", True)
    T, top_k, n_new = 0.9, 40, 8
    runs = {}
    for graph in (False, True):
        monkeypatch.setattr(kvm, "USE_HIP_GRAPH", graph)
        kv = KVCacheLM(m, B, capacity=256)
        gen = lambda n=n_new, **kw: kv.generate(ids_l, max_new_tokens=n, eos_token_id=EOS, pad_token_id=PAD, trie=trie,
                                                **{**dict(do_sample=True, temperature=T, top_k=top_k), **kw})
        outs = []
        for seed in (5, 5, 6, 7):
            torch.manual_seed(seed)
            outs.append(gen())
            assert kv.last_generate == {"loop": "device", "trie": constrained}
            assert kv.last_sample == {"seed": seed, "offset": 0, "temperature": T, "top_k": top_k}
        follow = gen()                                                      # no re-seed: the next B * n_new counters
        assert kv.last_sample["offset"] == B * n_new and kv.last_sample["seed"] == 7
        assert outs[0] == outs[1] and (outs[2] != outs[0] or outs[3] != outs[0])
        for rows in outs + [follow]:
            assert all(0 <= t < V and t not in special for row in rows for t in row)
            if constrained:
                _assert_paths(trie, rows, EOS, PAD)
        # 1, 2, 3 new tokens under one seed: the longer output starts with the shorter, and the token of each call's last step is the
        # reference's draw from the loop's own logits buffer -- the logits that step picked from
        def cands(prefix):
            if not constrained:
                return [v for v in range(V) if v not in special]
            node = trie.root
            for t in prefix:
                node = trie.get_next_node(node, t)
            return [t for t in trie.get_child_index(node) if t < V and t not in special]

        prev = None
        for n in (1, 2, 3):
            torch.manual_seed(9)
            rows = gen(n)
            if prev is not None:
                assert all(r[:len(p)] == p for r, p in zip(rows, prev)), (n, rows, prev)
            prev = rows
            if len(rows[0]) < n:
                continue                                                    # (every row had finished: HF stops, the trimmed step drew pad)
            lg64 = kv._greedy["logits"].double().cpu().numpy()
            u = philox_u(9, kv.last_sample["offset"] + (n - 1) * B + np.arange(B))
            assert kv.last_sample["offset"] == 0
            for b in range(B):
                if EOS in rows[b][:n - 1]:
                    assert rows[b][n - 1] == PAD
                    continue
                check_draw(sample_reference(lg64[b], cands(rows[b][:n - 1]), T, top_k, u[b]), rows[b][n - 1], u[b], EPS)
        # a tiny temperature is greedy decoding.  Checked step by step, so that it needs no lucky input: two of ~1000 bf16 logits share
        # the row maximum in several percent of all rows, and there the draw may take either while the argmax takes the smaller id.
        # While a row's tokens agree, the cold token is the reference's draw at T = 1e-4 from the logits that step saw, the greedy token
        # is the smallest id at the maximum, and the two are EQUAL wherever the maximum is untied and carries the whole weight.
        alive, exact = [True] * B, 0
        for n in (1, 2, 3):
            torch.manual_seed(3)
            cold = gen(n, temperature=1e-4)
            assert kv.last_generate["loop"] == "device" and kv.last_sample["temperature"] == 1e-4
            lg64 = kv._greedy["logits"].double().cpu().numpy()              # (the greedy call below overwrites the buffer)
            greedy = gen(n, do_sample=False)
            assert kv.last_sample is None and kv.last_generate == {"loop": "device", "trie": constrained}
            u = philox_u(3, (n - 1) * B + np.arange(B))
            for b in range(B):
                if not alive[b] or min(len(cold[b]), len(greedy[b])) < n or EOS in cold[b][:n - 1]:
                    continue
                assert cold[b][:n - 1] == greedy[b][:n - 1]
                cand = cands(cold[b][:n - 1])
                ref = sample_reference(lg64[b], cand, 1e-4, top_k, u[b])
                check_draw(ref, cold[b][n - 1], u[b], EPS)
                top = lg64[b][cand].max()
                tied = [c for c in cand if lg64[b][c] == top]
                assert greedy[b][n - 1] == min(tied)
                if len(tied) == 1 and ref["w"].sum() - 1.0 < 1e-6:
                    assert cold[b][n - 1] == greedy[b][n - 1], (n, b)
                    exact += 1
                alive[b] = cold[b][n - 1] == greedy[b][n - 1]
        assert exact >= B, exact
        torch.manual_seed(5)
        assert gen() == outs[0]                                             # ... and the sampling graph is still the sampling graph
        runs[graph] = (outs, prev, cold, greedy)
    assert runs[False] == runs[True]


def test_sampled_calls_that_keep_the_host_loop(monkeypatch):
    """DEVICE_SAMPLE on: temperature 0, a negative top_k, an ineligible trie and prompt + max_new_tokens beyond the capacity run the
    host loop (last_sample is None).  DEVICE_SAMPLE off (the default): do_sample=True is the host loop, restated here from extend()
    and logits_last() and compared token for token under torch.manual_seed(5).  Greedy calls do not look at the flag."""
    import navillm_amd.kvcache as kvm
    from navillm_amd.kvcache import KVCacheLM
    m, ids_l = _case()
    cfg = m.cfg
    B = len(ids_l)
    assert kvm.DEVICE_SAMPLE is False                                       # opt-in
    words = _words(40, 7, cfg.base_vocab_size, EOS)
    trie = _Trie(EOS, words)
    bad = _Trie(EOS, words + [[999, cfg.special_token_ids[0]]])
    call = lambda kv, **kw: kv.generate(ids_l, max_new_tokens=6, eos_token_id=EOS, pad_token_id=PAD, **kw)
    monkeypatch.setattr(kvm, "DEVICE_SAMPLE", True)

    class _HostLoop(Exception):
        pass

    def stop(*a, **k):                                                      # the host loop's first act is an extend()
        raise _HostLoop

    # only the routing is looked at: what the host loop makes of a zero temperature or a negative top_k is not this test's business
    cases = {"temperature 0": (256, dict(temperature=0.0, top_k=1)), "temperature nan": (256, dict(temperature=float("nan"))),
             "temperature inf": (256, dict(temperature=float("inf"))), "temperature below fp32": (256, dict(temperature=1e-60)),
             "top_k < 0": (256, dict(temperature=0.7, top_k=-1)), "top_k no int": (256, dict(temperature=0.7, top_k=2.5)),
             "ineligible trie": (256, dict(temperature=0.7, trie=bad)), "capacity": (96, dict(temperature=0.7))}
    for name, (cap, kw) in cases.items():
        kv = KVCacheLM(m, B, capacity=cap)
        seen = []
        monkeypatch.setattr(kv, "_generate_on_device", lambda *a, **k: seen.append(1))
        monkeypatch.setattr(kv, "extend", stop)
        with pytest.raises(_HostLoop):
            call(kv, do_sample=True, **kw)
        assert not seen and kv.last_generate == {"loop": "host", "trie": "trie" in kw} and kv.last_sample is None, name
    # the same call minus what sends it to the host loop does run on the device
    kv = KVCacheLM(m, B, capacity=256)
    _assert_paths(trie, call(kv, do_sample=True, temperature=0.7, trie=trie), EOS, PAD)
    assert kv.last_generate == {"loop": "device", "trie": True} and kv.last_sample["top_k"] == 50
    call(kv, do_sample=True, temperature=0.7, top_k=None)
    assert kv.last_generate["loop"] == "device" and kv.last_sample["top_k"] == 0
    greedy_on = call(kv)
    assert kv.last_generate == {"loop": "device", "trie": False} and kv.last_sample is None

    # the switch off: today's host loop, restated
    monkeypatch.setattr(kvm, "DEVICE_SAMPLE", False)
    kv = KVCacheLM(m, B, capacity=256)
    torch.manual_seed(5)
    got = call(kv, do_sample=True, temperature=0.7, top_k=50)
    assert kv.last_generate == {"loop": "host", "trie": False} and kv.last_sample is None
    kv2 = KVCacheLM(m, B, capacity=256)
    torch.manual_seed(5)
    seqs, want, live = [list(x) for x in ids_l], [[] for _ in range(B)], [True] * B
    for _ in range(6):
        lg = kv2.logits_last(kv2.extend(seqs)) / 0.7
        kth = torch.topk(lg, 50, dim=-1).values[:, -1:]
        nxt = torch.multinomial(torch.softmax(lg.masked_fill(lg < kth, float("-inf")), dim=-1), 1).view(-1).tolist()
        for b in range(B):
            t = nxt[b] if live[b] else PAD
            want[b].append(t)
            seqs[b].append(t)
            live[b] = live[b] and t != EOS
        if not any(live):
            break
    assert got == want
    assert call(kv) == greedy_on and kv.last_generate == {"loop": "device", "trie": False}
