"""Nucleus (top-p) sampling in the device-side decode loop: `nv_decode_pick_sample_topp_bf16` (unconstrained and over the children of a
trie node) against the fp64 reference of tests/topp_ref.py -- the uniform bit for bit, the kept count through `kept_out`, the token
inside its CDF interval over the survivors -- the frequencies of 4 096 draws, and `KVCacheLM.generate(do_sample=True, top_p=...)`
under NAVILLM_DEVICE_SAMPLE end to end (eager and replayed from a hipGraph), on the host loop and through NavModel.

EPS = 1e-5 is the allowance of tests/test_sample_decode_gpu.py for the kernel's fp32 sums; the same figure is the band inside which
the reference calls a nucleus boundary ambiguous (tests/topp_ref.py: there the kernel may decide either way; the case list has no
such case, tests/test_topp_decode_cpu.py says so, and the cap asserted here is 2 %).  The boundary itself is decided on integer
masses (weights truncated to 2^-40: < V * 2^-40 = 1e-8 of a total >= 1), far inside the band."""
import functools

import numpy as np
import pytest
import torch

import topp_ref as R
from sample_ref import philox_u, check_draw

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-5
SEED, OFFSET = 0x123456789abcdef1, (1 << 32) - 5          # the counter crosses into its high word within the first rows
MAX_STEPS = 4
CNTS = (0, 3, MAX_STEPS)                                   # at and past max_steps: the last one writes no out / u_out / kept_out
NV_ERR_ARG = -1
SENT = -7                                                  # sentinel of kept_out (out: -1, u_out: -1.0)


def _table_walk(off, tok, nxt, path):
    n = 0
    for c in path:
        e = [e for e in range(off[n], off[n + 1]) if tok[e] == c]
        assert len(e) == 1, (path, c)
        n = int(nxt[e[0]])
    return n


def _launch(lgd, ldl, V, sp0, nsp, tables, nodes, T, top_k, top_p, cnt, fin, eos, pad, max_steps=MAX_STEPS, seed=SEED, offset=OFFSET,
            bufs=None, entry="topp", expect=0):
    """one pick launch on a fresh state -> (state, node, out, u_out, kept_out) on the host.  entry "topp": the new symbol; "old":
    nv_decode_pick_sample_bf16 (no top_p, no kept_out)"""
    from navillm_amd import ops
    L = ops._L()
    B = lgd.shape[0]
    st = torch.zeros(L.nv_decode_state_ints(B), dtype=torch.int32)
    st[B:2 * B] = torch.tensor(fin, dtype=torch.int32)
    st[7 * B + 2] = cnt
    std = st.to(DEV)
    rng = torch.from_numpy(np.array([seed, offset], dtype=np.uint64).view(np.int64)).to(DEV)
    if bufs is None:
        bufs = (torch.full((max_steps, B), -1, dtype=torch.int32, device=DEV), torch.full((max_steps * B,), -1.0, dtype=torch.float32, device=DEV),
                torch.full((max_steps * B,), SENT, dtype=torch.int32, device=DEV))
    out, u_out, kept = bufs
    tr, node = (None, None, None, 0, None), None
    if tables is not None:
        td = [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in tables]
        node = torch.tensor(nodes, dtype=torch.int32, device=DEV)
        tr = (td[0].data_ptr(), td[1].data_ptr(), td[2].data_ptr(), tables[0].size - 1, node.data_ptr())
    head = (lgd.data_ptr(), ldl, V, sp0, nsp, *tr, T, top_k)
    tail = (std.data_ptr(), out.data_ptr(), max_steps, B, eos, pad, ops._st())
    if entry == "topp":
        rc = L.nv_decode_pick_sample_topp_bf16(*head, top_p, rng.data_ptr(), u_out.data_ptr(), kept.data_ptr(), *tail)
    else:
        rc = L.nv_decode_pick_sample_bf16(*head, rng.data_ptr(), u_out.data_ptr(), *tail)
    assert rc == expect, rc
    torch.cuda.synchronize()
    return std.cpu(), (None if node is None else node.cpu().tolist()), out.cpu(), u_out.cpu().numpy(), kept.cpu().numpy()


def _check_launch(res, ref_of, cnt, fin, eos, pad, tally):
    """the assertions shared by the unconstrained and the trie test; -> the tokens.  `ref_of(b)`: the reference of row b under the
    launch's settings; `tally`: [cases, ambiguous cases]"""
    s, _, out, u_out, kept = res
    B = len(fin)
    u = philox_u(SEED, OFFSET + cnt * B + np.arange(B))
    mine = np.arange(cnt * B, (cnt + 1) * B)
    if cnt < MAX_STEPS:
        assert u_out[mine].view(np.uint32).tolist() == u.view(np.uint32).tolist()       # bit for bit
        assert bool((np.delete(u_out, mine) == -1.0).all()) and bool((np.delete(kept, mine) == SENT).all())
    else:
        assert bool((u_out == -1.0).all()) and bool((kept == SENT).all())
    toks = s[:B].tolist()
    worst = 0.0
    for b in range(B):
        if fin[b]:
            assert toks[b] == pad and s[B + b] == 1, b
            assert cnt >= MAX_STEPS or kept[cnt * B + b] == SENT                        # a finished row writes no count
            continue
        ref = ref_of(b)
        tally[0] += 1
        tally[1] += bool(ref["ambiguous"])
        if cnt < MAX_STEPS:
            got = int(kept[cnt * B + b])
            if ref["ambiguous"]:
                sides = [a for a in ref["alt"] if a["kept"] == got]
                assert sides, (b, got, [a["kept"] for a in ref["alt"]])
                ref = sides[0]
            assert got == ref["kept"], (b, got, ref["kept"])
        if ref["token"] is None:
            assert toks[b] == eos and s[B + b] == 1, (b, toks[b])
            continue
        if ref["ambiguous"]:                                                            # (past max_steps no count tells the side)
            sides = [a for a in ref["alt"] if toks[b] in a["ids"]]
            assert sides, (b, toks[b])
            ref = sides[0]
        worst = max(worst, check_draw(ref, toks[b], u[b], EPS))
        assert s[B + b] == int(toks[b] == eos), b
    assert s[2 * B:].tolist() == [0] * (5 * B + 2) + [cnt, 0]              # nothing else of the state moves
    if cnt < MAX_STEPS:
        assert out[cnt].tolist() == toks and bool((np.delete(out.numpy(), cnt, axis=0) == -1).all())
    else:
        assert bool((out == -1).all())
    if worst > 0:
        print(f"u outside the token's fp64 CDF interval by {worst:.2e} (cnt={cnt})")
    return toks


@pytest.mark.parametrize("shape", R.SHAPES, ids=R.SHAPE_IDS)
def test_topp_pick_kernel_vs_the_fp64_reference(shape):
    """nv_decode_pick_sample_topp_bf16 without a trie over T x top_k x top_p x cnt on the planted rows of topp_ref.planted_rows: the
    uniform equals the numpy Philox bit for bit, kept_out equals the reference's count, the token is a survivor whose fp64 CDF
    interval holds u (within EPS), finished rows emit pad and write no count, a row of -inf candidates emits eos with count 0, nothing
    else of state / out / u_out / kept_out moves; top_p = 1 through the new entry is the old entry bit for bit; bad top_p is refused."""
    B, V, ldl, sp0 = shape
    nsp, eos, pad = R.NSPECIAL, 2, V - 1
    lg, fin = R.planted_rows(*shape)
    lgd = lg.to(DEV)
    tally, seen = [0, 0], {}
    for T, top_k, top_p in R.kernel_cases(shape):
        for cnt in CNTS:
            res = _launch(lgd, ldl, V, sp0, nsp, None, None, T, top_k, top_p, cnt, fin, eos, pad)
            toks = _check_launch(res, lambda b: R.case_reference(shape, b, T, top_k, top_p), cnt, fin, eos, pad, tally)
            for b, t in enumerate(toks):
                seen.setdefault((b, T, top_k, top_p), set()).add(t)
    print(f"{tally[0]} cases, {tally[1]} ambiguous")
    assert tally[1] <= 0.02 * tally[0]
    # the planted rows (tests/test_topp_decode_cpu.py checks what the reference says of them; here: what the kernel drew)
    for T in (0.01, 1.0):
        assert all(seen[0, T, k, p] == {R.TOP} for k in R.TOPKS for p in R.TOPPS)          # the argmax for every u
    assert R.case_reference(shape, 1, 1.0, 0, 0.5)["kept"] == 4 and seen[1, 1.0, 0, 0.5] <= set(R.TIE3) | {R.TOP}
    assert all(seen[2, T, k, 1e-6] <= {7, 300, V - 20} for T in R.TEMPS for k in R.TOPKS)
    assert len(set().union(*(seen[2, T, k, 1e-6] for T in R.TEMPS for k in R.TOPKS))) > 1   # the tied maxima are drawn, not only the first
    assert all(t != sp0 + 1 and t < V for ts in seen.values() for t in ts)
    if B > 5:
        assert seen[5, 1.0, 50, 0.5] <= set(R.ladder_ids()[:6]) and all(ts == {eos} for (b, *_), ts in seen.items() if b == 4)
    # top_p = 1.0f through the new entry == the old entry, bit for bit in token, state, out and u (and it reports the top-k count)
    for T, top_k, cnt in ((0.7, 50, 1), (1.0, 0, 3), (0.01, 1, MAX_STEPS)):
        a = _launch(lgd, ldl, V, sp0, nsp, None, None, T, top_k, 1.0, cnt, fin, eos, pad)
        b = _launch(lgd, ldl, V, sp0, nsp, None, None, T, top_k, None, cnt, fin, eos, pad, entry="old")
        assert a[0].tolist() == b[0].tolist() and a[2].tolist() == b[2].tolist()
        assert a[3].view(np.uint32).tolist() == b[3].view(np.uint32).tolist() and bool((b[4] == SENT).all())
        _check_launch(a, lambda r: R.topp_reference(lg[r].double().numpy(), R.candidates(V, sp0), T, top_k, 1.0, 0.5), cnt, fin, eos, pad, [0, 0])
    # equal (logits, rng, cnt, settings) give equal tokens and counts
    a = _launch(lgd, ldl, V, sp0, nsp, None, None, 100.0, 0, 0.9, 1, fin, eos, pad)
    b = _launch(lgd, ldl, V, sp0, nsp, None, None, 100.0, 0, 0.9, 1, fin, eos, pad)
    assert a[0].tolist() == b[0].tolist() and a[4].tolist() == b[4].tolist()
    # refusals: NV_ERR_ARG before any launch, nothing written
    for bad in (0.0, -0.1, 1.5, float("nan")):
        s, _, out, u_out, kept = _launch(lgd, ldl, V, sp0, nsp, None, None, 1.0, 50, bad, 0, fin, eos, pad, expect=NV_ERR_ARG)
        assert s.tolist() == [0] * B + list(fin) + [0] * (5 * B + 4)
        assert bool((out == -1).all()) and bool((u_out == -1.0).all()) and bool((kept == SENT).all())


def test_topp_pick_kernel_with_a_trie():
    """the same over the children of each row's trie node (topp_ref.trie_case: nodes with 3, 1, 2 pickable of 3, 3 tied of 4, a leaf,
    a finished row, 300 children); the node moves along the picked edge, a finished row's node stays."""
    from navillm_amd.kvcache import flatten_trie
    B, V, ldl, sp0 = R.TRIE_SHAPE
    nsp, eos, pad = R.NSPECIAL, 2, 1005
    trie, lg, cands = R.trie_case()
    off, tok, nxt, eligible = flatten_trie(trie, eos, V, range(sp0, sp0 + nsp))
    assert eligible
    paths, fin = [list(p) for p in R.TRIE_PATHS], list(R.TRIE_FIN)
    node0 = [_table_walk(off, tok, nxt, p) for p in paths]
    lgd = lg.to(DEV)
    tally, seen = [0, 0], {}
    for T, top_k, top_p in R.kernel_cases(R.TRIE_SHAPE):
        for cnt in CNTS:
            res = _launch(lgd, ldl, V, sp0, nsp, (off, tok, nxt), node0, T, top_k, top_p, cnt, fin, eos, pad)
            toks = _check_launch(res, lambda b: R.trie_reference(b, T, top_k, top_p), cnt, fin, eos, pad, tally)
            want = [node0[b] if (fin[b] or not trie.at(paths[b]).child) else _table_walk(off, tok, nxt, paths[b] + [toks[b]]) for b in range(B)]
            assert res[1] == want, (T, top_k, top_p, cnt)
            assert toks[1] == 40 and toks[4] == eos and toks[5] == pad
            for b, t in enumerate(toks):
                seen.setdefault((b, T, top_k, top_p), set()).add(t)
    print(f"{tally[0]} cases, {tally[1]} ambiguous")
    assert tally[1] <= 0.02 * tally[0]
    assert all(seen[3, T, k, p] <= {7, 300, 650} for T in (0.01, 1.0) for k in R.TOPKS for p in R.TOPPS)      # the tied children, never 1001
    assert len(set().union(*(ts for (b, *_), ts in seen.items() if b == 3))) > 1
    assert R.trie_reference(6, 100.0, 0, 0.5)["kept"] < 300 and len(set().union(*(ts for (b, *_), ts in seen.items() if b == 6))) > 3
    a = _launch(lgd, ldl, V, sp0, nsp, (off, tok, nxt), node0, 0.7, 50, 1.0, 1, fin, eos, pad)
    b = _launch(lgd, ldl, V, sp0, nsp, (off, tok, nxt), node0, 0.7, 50, None, 1, fin, eos, pad, entry="old")
    assert a[0].tolist() == b[0].tolist() and a[1] == b[1] and a[2].tolist() == b[2].tolist() and a[3].view(np.uint32).tolist() == b[3].view(np.uint32).tolist()


def test_topp_draw_frequencies():
    """64 identical rows whose six top-k survivors have known weights, top_p = 0.8 keeping three of them (topp_ref.freq_case), drawn at
    cnt = 0..63: none of the 4 096 draws leaves the nucleus, every count says 3, and every frequency lies within 5 sigma of its
    renormalised probability."""
    B, V, Vp, eos, pad, steps = 64, 1006, 1024, 2, 0, 64
    seed = 20243
    row, ref = R.freq_case()
    assert ref["ids"].tolist() == [17, 100, 333] and not ref["ambiguous"]
    p = ref["w"] / ref["w"].sum()
    lgd = row.to(torch.bfloat16).repeat(B, 1).contiguous().to(DEV)
    bufs = (torch.full((steps, B), -1, dtype=torch.int32, device=DEV), torch.full((steps * B,), -1.0, dtype=torch.float32, device=DEV),
            torch.full((steps * B,), SENT, dtype=torch.int32, device=DEV))
    for cnt in range(steps):
        _launch(lgd, Vp, V, 1000, 5, None, None, 1.0, R.FREQ_TOPK, R.FREQ_TOPP, cnt, [0] * B, eos, pad, max_steps=steps, seed=seed, offset=0, bufs=bufs)
    u = bufs[1].cpu().numpy()
    assert u.view(np.uint32).tolist() == philox_u(seed, np.arange(steps * B)).view(np.uint32).tolist()
    assert bool((bufs[2].cpu().numpy() == 3).all())
    toks = bufs[0].cpu().numpy().reshape(-1)
    n = toks.size
    freq = np.array([(toks == v).sum() for v in ref["ids"]])
    print("frequencies", freq.tolist(), "expected", (n * p).round(1).tolist())
    assert freq.sum() == n                                            # no token outside the nucleus
    assert bool((np.abs(freq - n * p) <= 5 * np.sqrt(n * p * (1 - p))).all()), (freq, n * p)
    for j in range(n):
        check_draw(ref, int(toks[j]), u[j], EPS)


# ---------------------------------------------------------------------------------------------------------------- generate()
MODEL_SEED = 12                                            # with it no step of the greedy sequences below has a tie at the maximum
EOS, PAD = 2, 0


def _mid_cfg(layers, heads):
    from navillm_amd import config as nvcfg
    return nvcfg.NavConfig(hidden_size=512, num_layers=layers, num_heads=heads, intermediate_size=1408, base_vocab_size=1000,
                           enc_hidden_size=256, enc_num_heads=4, enc_intermediate_size=512, image_feat_size=768)


@functools.lru_cache(maxsize=None)
def _case(B=4, seed=MODEL_SEED):
    """a small model and prompts of different lengths (plain tokens)"""
    from navillm_amd.nav_model import NavModel
    m = NavModel(nav_config=_mid_cfg(3, 4), device=torch.device(DEV), seed=seed)
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


def host_steps(m, ids_l, rows, trie):
    """the host's view of a produced sequence: step by step `extend` + `logits_last` on a cache of its own, fed the tokens of `rows`
    -> per step (logits [B, V] fp64, the candidates of every row, which rows were still unfinished)"""
    from navillm_amd.kvcache import KVCacheLM
    cfg = m.cfg
    V, special = cfg.vocab_size, set(cfg.special_token_ids)
    B = len(ids_l)
    kv = KVCacheLM(m, B, capacity=256)
    seqs, live = [list(x) for x in ids_l], [True] * B
    nodes = [trie.root] * B if trie is not None else None
    free = [v for v in range(V) if v not in special]
    steps = []
    for t in range(max(len(r) for r in rows)):
        lg = kv.logits_last(kv.extend(seqs)).double().cpu().numpy()
        cands = [free if trie is None else [c for c in trie.get_child_index(nodes[b]) if c < V and c not in special] for b in range(B)]
        steps.append((lg, cands, list(live)))
        for b in range(B):
            tk = rows[b][t]
            seqs[b].append(tk)
            if trie is not None and live[b]:
                nodes[b] = trie.get_next_node(nodes[b], tk)
            live[b] = live[b] and tk != EOS
    return steps


def max_ties(m, ids_l, rows, trie):
    """how many (step, unfinished row) pairs of a sequence have more than one candidate at the row maximum"""
    n = 0
    for lg, cands, live in host_steps(m, ids_l, rows, trie):
        for b in range(len(rows)):
            if live[b]:
                x = lg[b][cands[b]]
                n += int((x == x.max()).sum() > 1)
    return n


@pytest.mark.parametrize("constrained", [False, True], ids=["free", "trie"])
def test_generate_with_top_p_on_the_device(monkeypatch, constrained):
    """generate(do_sample=True, top_p=...) under DEVICE_SAMPLE: the device loop, last_sample records top_p, reproducible from
    torch.manual_seed, eager == hipGraph; another top_p re-captures the graph and every token lies in that step's nucleus (the logits
    recomputed by the host); top_p = 1.0 is the call without top_p; top_p = 1e-6 with top_k = 0 is greedy decoding."""
    import navillm_amd.kvcache as kvm
    from navillm_amd.kvcache import KVCacheLM
    m, ids_l = _case()
    cfg = m.cfg
    B = len(ids_l)
    trie = R.Trie(EOS, _words(300, 7, cfg.base_vocab_size, EOS)) if constrained else None
    monkeypatch.setattr(kvm, "DEVICE_SAMPLE", True)
    T, top_k, n_new = 0.9, 40, 8
    runs = {}
    for graph in (False, True):
        monkeypatch.setattr(kvm, "USE_HIP_GRAPH", graph)
        kv = KVCacheLM(m, B, capacity=256)
        gen = lambda **kw: kv.generate(ids_l, eos_token_id=EOS, pad_token_id=PAD, trie=trie,
                                       **{**dict(max_new_tokens=n_new, do_sample=True, temperature=T, top_k=top_k), **kw})
        outs = []
        for seed in (5, 5, 6):
            torch.manual_seed(seed)
            outs.append(gen(top_p=0.8))
            assert kv.last_generate == {"loop": "device", "trie": constrained}
            assert kv.last_sample == {"seed": seed, "offset": 0, "temperature": T, "top_k": top_k, "top_p": 0.8}
        assert outs[0] == outs[1]
        kind = ("sample", constrained)
        first = kv._greedy["graphs"].get(kind)
        # another top_p on the same object: a new graph, and tokens from the 0.3-nucleus of the logits of their step
        torch.manual_seed(5)
        tight = gen(top_p=0.3)
        assert kv.last_sample["top_p"] == 0.3
        if graph:
            second = kv._greedy["graphs"][kind]
            assert second[0] != first[0] and second[1] is not first[1]
        for t, (lg, cands, live) in enumerate(host_steps(m, ids_l, tight, trie)):
            for b in range(B):
                if live[b]:
                    ref = R.topp_reference(lg[b], cands[b], T, top_k, 0.3, 0.5)
                    ok = ref["ids"].tolist() if not ref["ambiguous"] else ref["alt"][1]["ids"].tolist()
                    assert tight[b][t] in ok, (t, b, tight[b][t], ok)
                else:
                    assert tight[b][t] == PAD
        # top_p = 1.0 and no top_p: the same tokens, the same (top-p free) record
        torch.manual_seed(5)
        one = gen(top_p=1.0)
        assert kv.last_sample == {"seed": 5, "offset": 0, "temperature": T, "top_k": top_k}
        torch.manual_seed(5)
        assert gen() == one and kv.last_sample == {"seed": 5, "offset": 0, "temperature": T, "top_k": top_k}
        # top_p = 1e-6 keeps the class of the maximum alone: greedy decoding wherever that class is one token
        greedy = gen(do_sample=False)
        assert kv.last_sample is None
        assert max_ties(m, ids_l, greedy, trie) == 0
        torch.manual_seed(3)
        assert gen(top_p=1e-6, top_k=0) == greedy
        assert kv.last_generate["loop"] == "device" and kv.last_sample["top_p"] == 1e-6
        torch.manual_seed(5)
        assert gen(top_p=0.8) == outs[0]                                   # ... and the 0.8 graph comes back
        runs[graph] = (outs, tight, one, greedy)
    assert runs[False] == runs[True]


def test_generate_with_top_p_on_the_host_loop_and_through_navmodel(monkeypatch):
    """DEVICE_SAMPLE off (the default): the host loop honours top_p (1e-6 with top_k = 0 gives the greedy tokens) and refuses a bad one
    before any work, as the device loop does; model('3dqa', ..., top_p=...) hands the value to generate()."""
    import navillm_amd.kvcache as kvm
    from navillm_amd.kvcache import KVCacheLM
    from navillm_amd.nav_model import NavModel
    m, ids_l = _case()
    B = len(ids_l)
    assert kvm.DEVICE_SAMPLE is False
    kv = KVCacheLM(m, B, capacity=256)
    call = lambda **kw: kv.generate(ids_l, max_new_tokens=6, eos_token_id=EOS, pad_token_id=PAD, **kw)
    greedy = call()
    assert max_ties(m, ids_l, greedy, None) == 0
    assert call(do_sample=True, top_k=0, top_p=1e-6) == greedy
    assert kv.last_generate == {"loop": "host", "trie": False} and kv.last_sample is None
    assert call(do_sample=True, temperature=3.0, top_p=1e-6) == greedy        # ... after temperature and the default top-k as well
    for flag in (False, True):
        monkeypatch.setattr(kvm, "DEVICE_SAMPLE", flag)
        monkeypatch.setattr(kv, "extend", lambda *a, **k: pytest.fail("work before the check"))
        for bad in (0.0, -0.1, 1.5, float("nan"), "0.5"):
            with pytest.raises(ValueError, match="top_p"):
                call(do_sample=True, top_p=bad)
        monkeypatch.undo()
    # through NavModel: the keyword reaches KVCacheLM.generate (and its check)
    cfg = _mid_cfg(1, 4)
    nm = NavModel(nav_config=cfg, device=torch.device(DEV), seed=3)
    nm.eval()
    g = torch.Generator().manual_seed(0)
    feats = [torch.randn(5, cfg.image_feat_size, generator=g), torch.randn(3, cfg.image_feat_size, generator=g)]
    ids2 = []
    for b, f in enumerate(feats):
        ids = [1] + torch.randint(3, cfg.base_vocab_size, (12 + b,), generator=g).tolist()
        for j in range(f.shape[0]):
            ids[2 + j] = cfg.cand_token_id
        ids2.append(ids)
    S = max(len(x) for x in ids2)
    ids_t = torch.full((2, S), cfg.pad_token_id, dtype=torch.int64)
    am = torch.zeros((2, S), dtype=torch.int64)
    for b, x in enumerate(ids2):
        ids_t[b, S - len(x):] = torch.tensor(x)
        am[b, S - len(x):] = 1
    batch = {"features": feats, "question": ["q"] * 2, "input_ids": ids_t, "attention_mask": am}
    got = []
    real = KVCacheLM.generate

    def spy(self, *a, **kw):
        got.append(kw.get("top_p", "absent"))
        return real(self, *a, **kw)

    monkeypatch.setattr(KVCacheLM, "generate", spy)
    out = nm("3dqa", batch, training=False, max_new_tokens=4, do_sample=True, top_p=0.25)
    assert got == [0.25] and len(out["generated_ids"]) == 2
    nm("3dqa", batch, training=False, max_new_tokens=4, do_sample=True)
    assert got[-1] == 1.0
    with pytest.raises(ValueError, match="top_p"):
        nm("3dqa", batch, training=False, max_new_tokens=4, do_sample=True, top_p=1.5)
