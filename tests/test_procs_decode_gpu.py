"""HF's repetition penalty and minimum length in the decode loop: `nv_decode_pick_proc_bf16` (greedy, over a trie node's children and
sampled) against the numpy reference of tests/procs_ref.py, one pick launch per case, and `KVCacheLM.generate(repetition_penalty=...,
min_new_tokens=...)` end to end -- device loop (eager and replayed from a hipGraph) against the host loop, with the processors off, and
through NavModel.

EPS = 1e-5 is the allowance of tests/test_topp_decode_gpu.py for the kernel's fp32 sums; the sampled inputs have no nucleus boundary
inside that band (asserted below from the reference alone), so every kept count is compared exactly."""
import functools

import numpy as np
import pytest
import torch

import procs_ref as P
from sample_ref import philox_u, check_draw
from topp_ref import Trie

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-5
SEED, OFFSET = 0x123456789abcdef1, (1 << 32) - 5
MAX_STEPS = 6
NV_ERR_ARG = -1
SENT, GUARD = -7, 0x5A5A5A5A                               # sentinel of kept_out (out: -1, u_out: -1.0); the words around the bitmap


def _dev_rows(rows):
    return torch.from_numpy(rows.view(np.int16).copy()).view(torch.bfloat16).to(DEV)


def _launch(shape, rows, seen, penalty, min_new, cnt, fin=None, tables=None, sample=None, seen_ld=None, null_seen=False, expect=0):
    """one launch of nv_decode_pick_proc_bf16 on a fresh state.  The bitmap lives in rows 1..B of a [B + 2, width] buffer whose rows 0
    and B + 1 and whose last column hold GUARD; the buffer's width (two words more than the ids need) is the seen_ld handed over unless
    one is given.  `sample`: (T, top_k, top_p) or None (the argmax)
    -> dict(state, tok, fin, node, out, u, kept, bitmap: the whole guarded buffer after, before: the same before)"""
    from navillm_amd import ops
    L = ops._L()
    B, V, ldl = shape
    sp0 = P.special0(V)
    fin = [0] * B if fin is None else list(fin)
    st = torch.zeros(L.nv_decode_state_ints(B), dtype=torch.int32)
    st[B:2 * B] = torch.tensor(fin, dtype=torch.int32)
    st[7 * B + 2] = cnt
    std = st.to(DEV)
    lgd = _dev_rows(rows)
    need = (V + 31) // 32
    ld = need + 1 if seen_ld is None else seen_ld
    width = max(ld, need) + 1
    before = np.full((B + 2, width), GUARD, np.uint32)
    before[1:B + 1, :max(ld, need)] = 0
    before[1:B + 1, :need] = P.bitmap(seen, V, need)
    buf = torch.from_numpy(before.view(np.int32).copy()).to(DEV)
    seen_ptr = None if null_seen else buf.data_ptr() + 4 * width
    rng = torch.from_numpy(np.array([SEED, OFFSET], dtype=np.uint64).view(np.int64)).to(DEV)
    out = torch.full((MAX_STEPS, B), -1, dtype=torch.int32, device=DEV)
    u_out = torch.full((MAX_STEPS * B,), -1.0, dtype=torch.float32, device=DEV)
    kept = torch.full((MAX_STEPS * B,), SENT, dtype=torch.int32, device=DEV)
    tr, node = (None, None, None, 0, None), None
    if tables is not None:
        td = [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in tables]
        node = torch.zeros((B,), dtype=torch.int32, device=DEV)          # every row at the root
        tr = (td[0].data_ptr(), td[1].data_ptr(), td[2].data_ptr(), tables[0].size - 1, node.data_ptr())
    smp = (0, 0.0, 0, 1.0, None, None, None) if sample is None else (1, *sample, rng.data_ptr(), u_out.data_ptr(), kept.data_ptr())
    rc = L.nv_decode_pick_proc_bf16(lgd.data_ptr(), ldl, V, sp0, P.NSPECIAL, *tr, *smp, seen_ptr, width if seen_ld is None else seen_ld, penalty,
                                    min_new, std.data_ptr(), out.data_ptr(), MAX_STEPS, B, P.EOS, P.PAD, ops._st())
    assert rc == expect, rc
    torch.cuda.synchronize()
    s = std.cpu()
    return dict(state=s, tok=s[:B].tolist(), fin=s[B:2 * B].tolist(), node=None if node is None else node.cpu().tolist(), out=out.cpu(),
                u=u_out.cpu().numpy(), kept=kept.cpu().numpy(), bitmap=buf.cpu().numpy().view(np.uint32), before=before)


def _check_books(shape, res, toks, cnt, was_fin):
    """what every pick leaves behind: tok, fin, out[cnt], nothing else of the state; in the guarded bitmap exactly the emitted token's
    bit of every row that was unfinished, nothing for a finished row (which emits pad)"""
    B, V, ldl = shape
    assert res["tok"] == toks, (res["tok"], toks)
    assert res["fin"] == [int(bool(f) or t == P.EOS) for f, t in zip(was_fin, toks)]
    assert res["state"][2 * B:].tolist() == [0] * (5 * B + 2) + [cnt, 0]
    assert res["out"][cnt].tolist() == toks and bool((np.delete(res["out"].numpy(), cnt, axis=0) == -1).all())
    want = res["before"].copy()
    for b, t in enumerate(toks):
        if not was_fin[b]:
            want[b + 1, t >> 5] |= np.uint32(1 << (t & 31))
        else:
            assert t == P.PAD
    assert np.array_equal(res["bitmap"], want)


@pytest.mark.parametrize("shape", P.SHAPES, ids=P.SHAPE_IDS)
def test_greedy_pick_with_the_repetition_penalty(shape):
    """the penalty changes the winner (a positive maximum divided, a negative one multiplied), a tie it creates goes to the smaller id;
    with penalty 1 over the same bitmap the unpenalised winners come back; an unfinished row sets exactly its token's bit, a finished
    row emits pad and sets none"""
    B, V, ldl = shape
    rows, seen = P.greedy_case(shape)
    ids = P.candidates(V, P.special0(V), P.NSPECIAL, P.EOS, 0, 0)
    want = [P.greedy_reference(rows[b], ids, seen[b], P.PENALTY, V) for b in range(B)]
    plain = [P.greedy_reference(rows[b], ids, set(), 1.0, V) for b in range(B)]
    assert want != plain and want[2] == 5 < P.far_id(V)
    _check_books(shape, _launch(shape, rows, seen, P.PENALTY, 0, 1), want, 1, [0] * B)
    _check_books(shape, _launch(shape, rows, seen, 1.0, 0, 1), plain, 1, [0] * B)
    fin = [0, 1, 0]
    _check_books(shape, _launch(shape, rows, seen, P.PENALTY, 0, 3, fin=fin), [want[0], P.PAD, want[2]], 3, fin)


@pytest.mark.parametrize("shape", P.SHAPES, ids=P.SHAPE_IDS)
@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
def test_minimum_length_bans_eos(shape, sampled):
    """eos holds every row's maximum: at cnt = min_new - 1 the runner-up is picked, at cnt = min_new eos is, and the row finishes
    (the sampled pick at T = 0.01, where the maximum carries all but e^-100 of the weight)"""
    B, V, ldl = shape
    rows, seen = P.min_new_case(shape)
    sample = (0.01, 0, 1.0) if sampled else None
    res = _launch(shape, rows, seen, 1.0, 4, 3, sample=sample)
    _check_books(shape, res, [P.far_id(V)] * B, 3, [0] * B)
    res = _launch(shape, rows, seen, 1.0, 4, 4, sample=sample)
    _check_books(shape, res, [P.EOS] * B, 4, [0] * B)
    assert res["fin"] == [1] * B


@pytest.mark.parametrize("shape", P.SHAPES, ids=P.SHAPE_IDS)
def test_trie_pick_with_the_repetition_penalty(shape):
    """the penalty over the children of the row's node only: the row maximum (seen, no child) stays out, the seen child loses to an
    unseen one, the node moves along the picked edge"""
    from navillm_amd.kvcache import flatten_trie
    B, V, ldl = shape
    rows, seen = P.trie_case(shape)
    trie = Trie(P.EOS, P.TRIE_WORDS)
    off, tok, nxt, eligible = flatten_trie(trie, P.EOS, V, range(P.special0(V), P.special0(V) + P.NSPECIAL))
    assert eligible
    kids = [w[0] for w in P.TRIE_WORDS]
    want = [P.greedy_reference(rows[b], kids, seen[b], P.PENALTY, V) for b in range(B)]
    assert want == [3, 17, 9]
    res = _launch(shape, rows, seen, P.PENALTY, 0, 2, tables=(off, tok, nxt))
    _check_books(shape, res, want, 2, [0] * B)
    edge = {int(tok[e]): int(nxt[e]) for e in range(off[0], off[1])}
    assert res["node"] == [edge[t] for t in want]


@pytest.mark.parametrize("shape", P.SHAPES, ids=P.SHAPE_IDS)
def test_sampled_pick_with_the_processors(shape):
    """the uniforms equal the numpy Philox bit for bit, kept_out equals the reference's count on the penalised row (eos banned at
    cnt 0), every token lies in its fp64 CDF interval over the survivors within EPS; no case has a nucleus boundary inside the band"""
    B, V, ldl = shape
    rows, seen = P.sample_case(shape)
    for T, top_k, top_p in P.SAMPLE_SETTINGS:
        for cnt in P.SAMPLE_CNTS:
            ids = P.candidates(V, P.special0(V), P.NSPECIAL, P.EOS, cnt, P.SAMPLE_MIN_NEW)
            refs = [P.sampled_reference(rows[b], ids, seen[b], P.SAMPLE_PENALTY, V, T, top_k, top_p, 0.5) for b in range(B)]
            assert not any(r["ambiguous"] for r in refs), (T, top_k, top_p, cnt)
            res = _launch(shape, rows, seen, P.SAMPLE_PENALTY, P.SAMPLE_MIN_NEW, cnt, sample=(T, top_k, top_p))
            u = philox_u(SEED, OFFSET + cnt * B + np.arange(B))
            mine = np.arange(cnt * B, (cnt + 1) * B)
            assert res["u"][mine].view(np.uint32).tolist() == u.view(np.uint32).tolist()
            assert bool((np.delete(res["u"], mine) == -1.0).all()) and bool((np.delete(res["kept"], mine) == SENT).all())
            assert res["kept"][mine].tolist() == [r["kept"] for r in refs], (T, top_k, top_p, cnt)
            worst = max(check_draw(refs[b], res["tok"][b], u[b], EPS) for b in range(B))
            if worst > 0:
                print(f"u outside the token's fp64 CDF interval by {worst:.2e} (T={T}, top_k={top_k}, top_p={top_p}, cnt={cnt})")
            _check_books(shape, res, res["tok"], cnt, [0] * B)


def test_refusals_leave_everything_untouched():
    """every NV_ERR_ARG the processors add comes back before any launch: state, out, u_out, kept_out and the bitmap keep their bits"""
    from navillm_amd.kvcache import flatten_trie
    shape = P.SHAPES[1]
    B, V, ldl = shape
    rows, seen = P.greedy_case(shape)
    off, tok, nxt, _ = flatten_trie(Trie(P.EOS, P.TRIE_WORDS), P.EOS, V, range(P.special0(V), P.special0(V) + P.NSPECIAL))
    need = (V + 31) // 32
    cases = [dict(penalty=v, min_new=0) for v in (0.0, -1.5, float("nan"), float("inf"))]
    cases += [dict(penalty=1.5, min_new=-1), dict(penalty=1.5, min_new=0, null_seen=True), dict(penalty=1.5, min_new=0, seen_ld=need - 1),
              dict(penalty=1.5, min_new=1, tables=(off, tok, nxt)), dict(penalty=1.0, min_new=1, tables=(off, tok, nxt), null_seen=True)]
    for sample in (None, (0.7, 5, 0.9)):
        for kw in cases:
            res = _launch(shape, rows, seen, cnt=1, fin=[0, 1, 0], sample=sample, expect=NV_ERR_ARG, **kw)
            assert res["state"].tolist() == [0] * B + [0, 1, 0] + [0] * (5 * B + 2) + [1, 0], kw
            assert bool((res["out"] == -1).all()) and bool((res["u"] == -1.0).all()) and bool((res["kept"] == SENT).all()), kw
            assert np.array_equal(res["bitmap"], res["before"]) and (res["node"] is None or res["node"] == [0] * B), kw


# ---------------------------------------------------------------------------------------------------------------- generate()
EOS, PAD = 2, 0
N_NEW, PENALTY, MIN_NEW = 12, 1.3, 4


@functools.lru_cache(maxsize=None)
def _model(which):
    from navillm_amd import config as nvcfg
    from navillm_amd.nav_model import NavModel
    from util import tiny_cfg, GOLDEN_SEED
    cfg = tiny_cfg("bf16") if which == "tiny" else nvcfg.gpt2_small_shaped(num_layers=2)
    m = NavModel(nav_config=cfg, device=torch.device(DEV), seed=GOLDEN_SEED)
    m.eval()
    g = torch.Generator().manual_seed(77)
    ids_l = [[1] + torch.randint(3, cfg.base_vocab_size, (9 + 7 * b,), generator=g).tolist() for b in range(3)]      # ragged prompts
    return m, ids_l


def _words(n, seed, ids_l, vocab):
    """n random words of 2-8 tokens, drawn half from the prompts' own tokens (seen from the first step on) and half from the vocabulary"""
    rng = np.random.RandomState(seed)
    own = sorted(set(t for x in ids_l for t in x if t > 2))
    return [[int(rng.choice(own)) if rng.rand() < 0.5 else int(rng.randint(3, vocab)) for _ in range(rng.randint(2, 9))] for _ in range(n)]


def _host_reference(m, ids_l, out, penalty, min_new, trie):
    """the greedy sequences recomputed step by step from the host's logits and tests/procs_ref.py: the argmax set of every step (all
    ids at the maximum of the processed row) -> how many steps had a tie at the maximum"""
    from navillm_amd.kvcache import KVCacheLM
    cfg = m.cfg
    V, special = cfg.vocab_size, set(cfg.special_token_ids)
    B = len(ids_l)
    kv = KVCacheLM(m, B, capacity=256)
    seqs, live = [list(x) for x in ids_l], [True] * B
    seen = P.seen_sets(ids_l)
    nodes = [trie.root] * B if trie is not None else None
    ties = 0
    for t in range(len(out[0])):
        lg = kv.logits_last(kv.extend(seqs)).to(torch.bfloat16).view(torch.int16).cpu().numpy().view(np.uint16)
        for b in range(B):
            tk = out[b][t]
            if not live[b]:
                assert tk == PAD
                continue
            ids = [v for v in (range(V) if trie is None else trie.get_child_index(nodes[b])) if v < V and v not in special]
            ids = [v for v in ids if not (t < min_new and v == EOS)]
            x = P.processed_row(lg[b], seen[b], penalty, V)[ids]
            top = [v for v, xv in zip(ids, x) if xv == x.max()]
            ties += len(top) > 1
            assert tk == top[0], (t, b, tk, top)
        P.seen_update(seen, [out[b][t] for b in range(B)], live)
        for b in range(B):
            seqs[b].append(out[b][t])
            if trie is not None and live[b]:
                nodes[b] = trie.get_next_node(nodes[b], out[b][t])
            live[b] = live[b] and out[b][t] != EOS
    return ties


@pytest.mark.parametrize("which", ["tiny", "gpt2_small_2_layers"])
def test_device_loop_equals_host_loop_with_the_processors(monkeypatch, which):
    """greedy with both processors and trie-greedy with the penalty: device loop (eager, hipGraph) == host loop, token for token, and
    both are what tests/procs_ref.py picks from the host's logits; the penalised output differs from the unpenalised one; no eos in
    the first MIN_NEW tokens; last_generate records the processors"""
    import navillm_amd.kvcache as kvm
    from navillm_amd.kvcache import KVCacheLM
    m, ids_l = _model(which)
    B = len(ids_l)
    trie = Trie(EOS, _words(200, 5, ids_l, m.cfg.base_vocab_size))
    runs = {}
    for tag, dev_loop, graph in (("host", False, False), ("device", True, False), ("graph", True, True)):
        monkeypatch.setattr(kvm, "DEVICE_GREEDY", dev_loop)
        monkeypatch.setattr(kvm, "USE_HIP_GRAPH", graph)
        kv = KVCacheLM(m, B, capacity=256)
        gen = lambda **kw: kv.generate(ids_l, max_new_tokens=N_NEW, eos_token_id=EOS, pad_token_id=PAD, **kw)
        free = gen(repetition_penalty=PENALTY, min_new_tokens=MIN_NEW)
        assert kv.last_generate == {"loop": "device" if dev_loop else "host", "trie": False,
                                    "processors": {"repetition_penalty": PENALTY, "min_new_tokens": MIN_NEW}}
        assert gen(repetition_penalty=PENALTY, min_new_tokens=MIN_NEW) == free                 # (a replay of the captured graph)
        tr = gen(repetition_penalty=PENALTY, trie=trie)
        assert kv.last_generate["trie"] and kv.last_generate["processors"] == {"repetition_penalty": PENALTY, "min_new_tokens": 0}
        only_min = gen(min_new_tokens=MIN_NEW)
        runs[tag] = (free, tr, only_min, gen(), gen(trie=trie))
    print("host  :", runs["host"][0])
    print("graph :", runs["graph"][0])
    assert runs["host"] == runs["device"] == runs["graph"]
    free, tr, only_min, plain, plain_trie = runs["host"]
    assert free != plain
    print("the penalty changes the trie-constrained output:", tr != plain_trie)
    assert all(EOS not in row[:MIN_NEW] for row in free + only_min) and all(len(row) >= MIN_NEW for row in free)
    ties = _host_reference(m, ids_l, free, PENALTY, MIN_NEW, None) + _host_reference(m, ids_l, tr, PENALTY, 0, trie)
    ties += _host_reference(m, ids_l, only_min, 1.0, MIN_NEW, None)
    print("steps with a tie at the maximum:", ties)


def test_sampled_device_loop_with_the_processors_eager_equals_graph(monkeypatch):
    """NAVILLM_DEVICE_SAMPLE: the sampled device loop with both processors and top-p draws the same tokens eager and replayed, for one
    seed; no eos in the first MIN_NEW tokens"""
    import navillm_amd.kvcache as kvm
    from navillm_amd.kvcache import KVCacheLM
    m, ids_l = _model("tiny")
    monkeypatch.setattr(kvm, "DEVICE_SAMPLE", True)
    runs = []
    for graph in (False, True):
        monkeypatch.setattr(kvm, "USE_HIP_GRAPH", graph)
        kv = KVCacheLM(m, len(ids_l), capacity=256)
        torch.manual_seed(5)
        runs.append(kv.generate(ids_l, max_new_tokens=N_NEW, eos_token_id=EOS, pad_token_id=PAD, do_sample=True, temperature=0.9, top_k=40,
                                top_p=0.8, repetition_penalty=PENALTY, min_new_tokens=MIN_NEW))
        assert kv.last_generate["loop"] == "device" and kv.last_sample["seed"] == 5 and "processors" in kv.last_generate
        if graph:
            assert set(kv._greedy["graphs"]) == {("proc", ("sample", False))}
    assert runs[0] == runs[1] and all(EOS not in row[:MIN_NEW] for row in runs[0])


def test_processors_off_replays_the_plain_graph():
    """1.0 / None / 0 are off: the call replays the graph object a processor-free call captured, the `graphs` dict gains no kind, and
    last_generate has no "processors"; a processor-on call in between captures a kind of its own and leaves the plain one alone"""
    import navillm_amd.kvcache as kvm
    from navillm_amd.kvcache import KVCacheLM
    assert kvm.DEVICE_GREEDY and kvm.USE_HIP_GRAPH
    m, ids_l = _model("tiny")
    kv = KVCacheLM(m, len(ids_l), capacity=256)
    gen = lambda **kw: kv.generate(ids_l, max_new_tokens=N_NEW, eos_token_id=EOS, pad_token_id=PAD, **kw)
    plain = gen()
    first = kv._greedy["graphs"][False]
    assert set(kv._greedy["graphs"]) == {False} and kv.last_generate == {"loop": "device", "trie": False}
    on = gen(repetition_penalty=PENALTY, min_new_tokens=MIN_NEW)
    assert set(kv._greedy["graphs"]) == {False, ("proc", False)} and on != plain
    for off in (dict(repetition_penalty=1.0, min_new_tokens=0), dict(repetition_penalty=None, min_new_tokens=None), dict(repetition_penalty=1)):
        assert gen(**off) == plain
        assert kv.last_generate == {"loop": "device", "trie": False}
        assert set(kv._greedy["graphs"]) == {False, ("proc", False)} and kv._greedy["graphs"][False][1] is first[1]


def test_navmodel_forwards_the_processors():
    """model('3dqa', batch, training=False, repetition_penalty=..., min_new_tokens=..., max_new_tokens=...) returns what
    KVCacheLM.generate returns with those settings on the same prompts, which is not what it returns without them"""
    from navillm_amd.kvcache import KVCacheLM
    from navillm_amd.nav_model import NavModel
    from util import tiny_cfg, GOLDEN_SEED
    cfg = tiny_cfg("bf16")
    nm = NavModel(nav_config=cfg, device=torch.device(DEV), seed=GOLDEN_SEED)
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
    seen_args = []
    real = KVCacheLM.generate

    def spy(self, ids_l, vix_l, vis_all, **kw):
        seen_args.append(([list(x) for x in ids_l], [list(v) for v in vix_l], vis_all.clone(), kw))
        return real(self, ids_l, vix_l, vis_all, **kw)

    mp = pytest.MonkeyPatch()
    try:
        mp.setattr(KVCacheLM, "generate", spy)
        out = nm("3dqa", batch, training=False, repetition_penalty=PENALTY, min_new_tokens=MIN_NEW, max_new_tokens=N_NEW)
        plain = nm("3dqa", batch, training=False, max_new_tokens=N_NEW)
    finally:
        mp.undo()
    ids_l, vix_l, vis_all, kw = seen_args[0]
    assert kw["repetition_penalty"] == PENALTY and kw["min_new_tokens"] == MIN_NEW and kw["max_new_tokens"] == N_NEW
    kv = KVCacheLM(nm, 2, capacity=(S + N_NEW + 127) // 128 * 128)          # (the capacity NavModel gives its own)
    direct = kv.generate(ids_l, vix_l, vis_all, **kw)
    assert kv.last_generate["processors"] == {"repetition_penalty": PENALTY, "min_new_tokens": MIN_NEW}
    assert out["generated_ids"] == direct and out["generated_ids"] != plain["generated_ids"]
    assert all(EOS not in row[:MIN_NEW] for row in direct)
