"""Inference-only incremental LM over a per-layer K/V cache in HBM.

Two callers:

* **prefix reuse across navigation steps** (`NavModel.enable_kv_cache`): the prompt of step t+1 repeats the prompt
  of step t up to the last `<hist>` token (tasks/datasets/r2r.py:18-22; history embeddings are detached constants,
  tasks/agents/mp3d_agent.py:778), so only the new suffix (~100 tokens instead of ~650) goes through the decoder.
* **greedy generation** (`KVCacheLM.generate`): HF `generate(do_sample=False)` as the reference calls it
  (models/nav_model.py:324-341,388-402; models/modified_lm.py:184-199) with the special-id logit mask
  (modified_lm.py:122-124) and the trie-constrained decoding of modified_lm.py:10-30.
  `do_sample=True` (tasks/agents/llava.py:58-62) samples instead: on the host loop, or -- NAVILLM_DEVICE_SAMPLE=1 -- in the same device loop.

Layout: one packed post-RoPE `qkv` buffer per decoder layer, `[B*capacity (+1 junk row), 3d]` bf16 (7B, B=8,
capacity 1024: 201 MB per layer, 6.4 GB in all -- nothing next to 288 GB).  Samples are LEFT-aligned (token j of
sample b lives at row b*capacity + j, position j): appending never moves cached rows, and the positions are the
`position_ids = cumsum(attention_mask)-1` HF's generation path uses.  The training/prefill path of the reference
numbers positions over the left padding instead; RoPE scores depend on position differences only, so the two frames
agree up to bf16 rounding of the rotated q/k (tests/test_kvcache_gpu.py bounds it against full recompute).

Everything arithmetic is a launch of the same HIP kernels as the training path (plus `nv_rope_rows_bf16` and
`nv_attn_fwd_strided_bf16`); there is no autograd here.
"""
import ctypes
import math
import numbers
import os

import numpy as np
import torch

from . import lib as _lib
from . import ops
from . import debug as _debug
from . import functions as _fn

BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32
DEVICE_GREEDY = os.environ.get("NAVILLM_DEVICE_GREEDY", "1") != "0"      # greedy decoding (free or trie-constrained) with the loop on the device
USE_HIP_GRAPH = os.environ.get("NAVILLM_DECODE_GRAPH", "1") != "0"       # ... replayed from a captured hipGraph
# do_sample=True with the loop on the device as well.  Opt-in: the draws then come from the library's own Philox4x32-10 (keyed from
# torch's CUDA generator like the dropout kernels), which cannot reproduce torch.multinomial's stream draw for draw.
DEVICE_SAMPLE = os.environ.get("NAVILLM_DEVICE_SAMPLE", "0") != "0"


def flatten_trie(trie, eos, V, special_ids):
    """A trie of the tools/trie.py protocol as three int32 arrays (what `decode_pick_trie_kernel` walks): node n owns the edges
    [off[n], off[n+1]), edge e carries token tok[e] and leads to node nxt[e].  Node 0 is the root, a node's edges are sorted by token
    id, and a leaf is the one edge `eos -> itself` -- which is what the protocol says about it (get_child_index = [eos],
    get_next_node = the node).  Built through `.root`, `.get_child_index(node)` and `.get_next_node(node, w)` alone, nodes told
    apart by identity; get_next_node only ever sees tokens get_child_index just returned, so a trie that inserts on a miss
    (the reference's defaultdict) keeps exactly the nodes it had.
    -> (off [N+1], tok [E], nxt [E], eligible); eligible is False when some node has no pickable child (every child >= V or a
    special id): what the host loop answers there is torch.argmax over an all -inf row, and such a trie stays on the host loop."""
    special = set(int(t) for t in special_ids)
    nodes, index = [trie.root], {id(trie.root): 0}                      # `nodes` keeps every node alive: ids stay unique
    off, tok, nxt = [0], [], []
    eligible = True
    n = 0
    while n < len(nodes):
        cur = nodes[n]
        n += 1
        kids = sorted(set(int(w) for w in trie.get_child_index(cur)))
        for w in kids:
            child = trie.get_next_node(cur, w)
            j = index.get(id(child))
            if j is None:
                j = index[id(child)] = len(nodes)
                nodes.append(child)
            tok.append(w)
            nxt.append(j)
        off.append(len(tok))
        if not any(0 <= w < V and w not in special for w in kids):
            eligible = False
    return np.asarray(off, np.int32), np.asarray(tok, np.int32), np.asarray(nxt, np.int32), eligible


def _top_p_warp(lg, top_p):
    """HF's TopPLogitsWarper (min_tokens_to_keep = 1) on fp32 logits [B, V], by the rule of `decode_pick_sample_kernel`: a logit value
    stays iff the softmax weight of the STRICTLY larger logits is < top_p; equal logits stay or go together (HF breaks an exact tie
    at the boundary by sort order); the maximum stays.  -> the logits with what goes at -inf"""
    xs, order = torch.sort(lg, dim=-1, descending=True)
    p = torch.softmax(xs, dim=-1)
    before = torch.cumsum(p, dim=-1) - p                                # the weight sorted in front of each entry ...
    first = torch.ones_like(xs, dtype=torch.bool)
    first[:, 1:] = xs[:, 1:] != xs[:, :-1]                              # ... which at the first entry of a run of equal logits is the
    above = torch.cummax(torch.where(first, before, torch.zeros_like(before)), dim=-1).values       # weight strictly above the run
    drop = above >= top_p
    drop[:, 0] = False
    return lg.masked_fill(torch.zeros_like(drop).scatter(1, order, drop), float("-inf"))


def _check_processors(repetition_penalty, min_new_tokens, trie):
    """the arguments of the two logits processors as generate() takes them -> (p32, min_new), or None when both are off.  p32 is the
    penalty as the fp32 every implementation of the rule multiplies and divides by (DESIGN.md §4 "Logits processors"); off is p32 == 1
    with min_new == 0.  Raises ValueError for anything but None or a finite real > 0 (as an fp32 too) / None or an int >= 0, bools
    excluded, and for a minimum length under a trie."""
    p = 1.0 if repetition_penalty is None else repetition_penalty
    if isinstance(p, bool) or not isinstance(p, numbers.Real) or not 0.0 < float(p) < math.inf:           # (a NaN fails the comparison)
        raise ValueError(f"KVCacheLM.generate: repetition_penalty must be None or a finite real number > 0, not {repetition_penalty!r}")
    with np.errstate(over="ignore", under="ignore"):
        p32 = float(np.float32(p))
    if not 0.0 < p32 < math.inf:
        raise ValueError(f"KVCacheLM.generate: repetition_penalty {repetition_penalty!r} is not a finite number > 0 in fp32")
    n = 0 if min_new_tokens is None else min_new_tokens
    if isinstance(n, bool) or not isinstance(n, numbers.Integral) or n < 0:
        raise ValueError(f"KVCacheLM.generate: min_new_tokens must be None or an int >= 0, not {min_new_tokens!r}")
    n = min(int(n), 2 ** 31 - 1)
    if n > 0 and trie is not None:
        raise ValueError("KVCacheLM.generate: min_new_tokens > 0 cannot be combined with a trie (a trie leaf allows eos alone: the trie "
                         "decides where an answer ends)")
    return None if (p32 == 1.0 and n == 0) else (p32, n)


def _seen_bitmap(seqs, V):
    """the kernel's `seen` bitmap of the prompts: [B, ceil(V / 32)] uint32, bit v & 31 of word v >> 5 of row b set for every id v of
    seqs[b] inside [0, V)"""
    bm = np.zeros((len(seqs), (V + 31) // 32), np.uint32)
    for b, x in enumerate(seqs):
        ids = np.unique(np.asarray(x, dtype=np.int64))
        ids = ids[(ids >= 0) & (ids < V)]
        np.bitwise_or.at(bm[b], ids >> 5, np.uint32(1) << (ids & 31).astype(np.uint32))
    return bm


def _penalise_seen(lg, seen, p32):
    """the repetition penalty on fp32 logits [B, V] that hold bf16 values, in place: the entries of row b at the ids of seen[b] become
    bf16(x * p32) when x < 0, else bf16(x / p32), widened again.  Computed on the CPU on the few seen entries alone: torch's CPU fp32
    divide is the correctly rounded one of the rule (a GPU divide by a scalar may multiply by the reciprocal instead)."""
    V = lg.shape[1]
    rows = np.concatenate([np.full(len(s), b, np.int64) for b, s in enumerate(seen)])
    cols = np.concatenate([np.fromiter(s, np.int64, len(s)) for s in seen])
    ok = (cols >= 0) & (cols < V)
    if not ok.any():
        return lg
    idx = ops.h2d(torch.from_numpy(np.stack([rows[ok], cols[ok]])), lg.device)
    x = lg[idx[0], idx[1]].cpu()
    x = torch.where(x < 0, x * p32, x / p32).to(BF16).float()
    lg[idx[0], idx[1]] = ops.h2d(x, lg.device)
    return lg


class KVCacheLM:
    def __init__(self, model, batch_size, capacity=1024):
        cfg = model.cfg
        self.model, self.B, self.cap = model, batch_size, capacity
        d = cfg.hidden_size
        dev = model.device
        rows = batch_size * capacity + 1                      # + one junk row that padding rows of a block scatter into
        self.qkv = [torch.zeros((rows, 3 * d), dtype=BF16, device=dev) for _ in range(cfg.num_layers)]
        self.attn = torch.zeros((batch_size * capacity, d), dtype=BF16, device=dev)
        self.lse = torch.empty((batch_size, cfg.num_heads, capacity), dtype=F32, device=dev)
        self.kv0 = torch.zeros((batch_size,), dtype=I32, device=dev)
        self._dec, self._dec_key, self._ws = None, None, None
        self._greedy = None                                    # device-side decode loop: buffers + captured hipGraphs
        self._trie_host, self._trie_dev = None, None           # the flattened trie of the last constrained call, host and device
        self.last_generate = None                              # {"loop": "device" | "host", "trie": bool} of the last generate()
        self.last_sample = None                                # {"seed", "offset", "temperature", "top_k"} of a device-sampled generate(), + "top_p" when < 1
        self._key_ids = {}                                     # reuse key (hashable) -> small int
        self.reset()

    def __del__(self):
        d, self._dec = getattr(self, "_dec", None), None
        if d:
            try:
                ops._L().nv_decoder_destroy(d)
            except Exception:
                pass

    def reset(self, b=None):
        """forget the cached tokens (of sample b, or of every sample) -- e.g. at an episode boundary"""
        empty = (np.zeros(0, np.int64), np.zeros(0, np.int64))
        if b is None:
            self.state = [empty for _ in range(self.B)]
            self._key_ids.clear()
            if _debug.POISON:                      # NAVILLM_POISON=1: nothing of the forgotten prompts may be read again
                for t in self.qkv + [self.attn]:
                    _debug.poison_(t, masked_reads=True)
                _debug.poison_(self.lse)
        else:
            self.state[b] = empty

    # compatibility views (tests / callers read the cached ids)
    @property
    def ids(self):
        return [s[0].tolist() for s in self.state]

    # ------------------------------------------------------------------ the native layer loop (navillm_amd/csrc/decoder_runtime.cpp)
    def _decoder(self):
        m, cfg, st = self.model, self.model.cfg, self.model.store
        st.wait_params()           # the native layer loop reads the weights through raw pointers: behind a pending optimizer update
        # keyed by what the layer table POINTS AT, not by the stream (with the stream in the key the decoder was torn
        # down and rebuilt -- ~200 ctypes calls and a fresh split-K workspace allocation + memset -- INSIDE the hipGraph capture of
        # the greedy step, which runs on a side stream).  The split-K workspace handed to the decoder is only touched by the tile
        # GEMMs of prefill-sized steps (M > 16), which always run on the stream the decoder was created on; the captured decode
        # step (M = B <= 16) runs the weight streamers and never reads it.
        key = (id(m.fp8), m.fp8 is not None and m.fp8.resident is not None, m.store.param["lm"].data_ptr(),
               m.fp8 is not None and m.fp8.overlap)
        if self._dec is not None and self._dec_key == key:
            return self._dec
        L = ops._L()
        if self._dec is not None:
            L.nv_decoder_destroy(self._dec)
        dec = ctypes.c_void_p(L.nv_decoder_create(cfg.num_layers, cfg.hidden_size, cfg.num_heads, cfg.head_dim, cfg.intermediate_size,
                                                  cfg.rms_norm_eps))
        if not dec:
            raise _lib.NaviLLMHipError("nv_decoder_create failed")
        kinds = ("qkv", "o", "gate_up", "down")
        for i in range(cfg.num_layers):
            p = f"lang_model.model.layers.{i}."
            _lib.check(L.nv_decoder_set_layer(dec, i, st.p(p + "input_layernorm.weight").data_ptr(),
                                              st.p(p + "post_attention_layernorm.weight").data_ptr(), self.qkv[i].data_ptr()), "nv_decoder_set_layer")
            for k, kind in enumerate(kinds):
                if m.fp8 is not None:
                    wb = m.fp8.resident[i][kind].data_ptr() if m.fp8.resident is not None else None      # bf16(s*q) kept resident
                    rc = L.nv_decoder_set_weight(dec, i, k, wb, m.fp8.codes[i][kind].data_ptr(), m.fp8.scales[i][kind].data_ptr())
                else:
                    rc = L.nv_decoder_set_weight(dec, i, k, m.lm_w(i, kind).data_ptr(), None, None)
                _lib.check(rc, "nv_decoder_set_weight")
        scratch = m.fp8._scratch.data_ptr() if (m.fp8 is not None and m.fp8._scratch is not None) else None
        if m.fp8 is not None:
            _lib.check(L.nv_decoder_set_fp8_gemm_mode(dec, int(m.fp8.gemm_mode)), "nv_decoder_set_fp8_gemm_mode")
        _lib.check(L.nv_decoder_set_shared(dec, m.rope_cos.data_ptr(), m.rope_sin.data_ptr(), st.p("lang_model.model.norm.weight").data_ptr(),
                                           ops._gemm_ws(m.device) if ops.SPLITK_TAIL else None, scratch), "nv_decoder_set_shared")
        if m.fp8 is not None and m.fp8.overlap:
            pa, pb, side = m.fp8.pipe()
            _lib.check(L.nv_decoder_set_fp8_overlap(dec, pa.data_ptr(), pb.data_ptr(), side.cuda_stream), "nv_decoder_set_fp8_overlap")
        self._dec, self._dec_key = dec, key
        return dec

    def _key_codes(self, vis_idx, vis_keys):
        """per-token reuse code: 0 = plain token, -1 = visual row that must be recomputed, > 0 = interned key of a constant row"""
        vi = np.asarray(vis_idx, dtype=np.int64)
        codes = np.zeros(vi.size, dtype=np.int64)
        for j in np.flatnonzero(vi >= 0):                  # the few visual tokens only (a Python loop over all ~650 tokens of all
            k = False if vis_keys is None else vis_keys[int(vi[j])]     # 8 prompts was 1 ms of host time per step)
            codes[j] = -1 if k is False else self._key_ids.setdefault(k, len(self._key_ids) + 1)
        return codes

    @torch.no_grad()
    def extend(self, ids_list, vis_idx_list=None, vis_all=None, vis_keys=None, return_rows="last"):
        """Bring the cache to the prompts `ids_list` (B python lists of token ids, no padding) and return the final-norm
        hidden state of each sample's LAST token, [B, d] bf16.

        (return_rows="all": the hidden states of all new rows, packed sample after sample, with their offsets.)
        vis_idx_list[b][j] = row of `vis_all` ([R, d] fp32, device) added to token j's embedding, or -1;
        vis_keys[r] identifies row r across calls: equal keys = the same constant embedding (a `<hist>` token of an
        earlier step), `False` = never reusable (candidates change every step).  Tokens are reused from the cache while
        ids and keys match; the rest is recomputed.  The decoder layers run as ONE native call (nv_decoder_extend)."""
        m, cfg = self.model, self.model.cfg
        st, dev = m.store, m.device
        B, cap, H, d = self.B, self.cap, cfg.num_heads, cfg.hidden_size
        assert len(ids_list) == B
        new_state, P, n = [], [], []
        for b in range(B):
            ids = np.asarray(ids_list[b], dtype=np.int64)
            Lb = ids.size
            assert 0 < Lb <= cap, f"prompt of {Lb} tokens does not fit the cache capacity {cap}"
            codes = np.zeros(Lb, np.int64) if vis_idx_list is None else self._key_codes(vis_idx_list[b], vis_keys)
            old_i, old_c = self.state[b]
            k = min(old_i.size, Lb - 1)                        # keep >= 1 new token: its hidden state is the output
            diff = np.flatnonzero((old_i[:k] != ids[:k]) | (old_c[:k] != codes[:k]) | (codes[:k] < 0))
            P.append(int(diff[0]) if diff.size else k)
            n.append(Lb - P[-1])
            new_state.append((ids, codes))
        # the new rows, PACKED sample after sample (no padding to the longest suffix: every kernel of the step is row-wise, and at
        # ~100 new tokens per sample the padded block layout cost a whole extra 256-row GEMM tile row on a typical step)
        off = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
        M = int(off[-1])
        ids_new = np.empty(M, np.int32)
        vix_new = np.full(M, -1, np.int32)
        pos_new = np.empty(M, np.int32)
        crow = np.empty(M, np.int32)                           # cache row each new row scatters to ...
        last = np.zeros(B, np.int32)
        for b in range(B):
            s, e = int(off[b]), int(off[b + 1])
            ids_new[s:e] = new_state[b][0][P[b]:]
            if vis_idx_list is not None:
                vix_new[s:e] = vis_idx_list[b][P[b]:]
            ar = np.arange(P[b], P[b] + n[b], dtype=np.int32)
            pos_new[s:e] = ar
            crow[s:e] = b * cap + ar
            last[b] = e - 1
        grow = crow                                            # ... and reads its attention output back from
        # one pinned staging buffer, one H2D copy for all six index arrays
        packed = np.concatenate([ids_new, vix_new, pos_new, crow, grow, last])
        idx = ops.h2d(torch.from_numpy(packed), dev)
        ids_d, vix_d, pos_d, crow_d, grow_d = (idx[k * M:(k + 1) * M] for k in range(5))
        last_d = idx[5 * M:5 * M + B]
        Lmax = max(s[0].size for s in new_state)
        qmin = (min(P) // 128) * 128

        x = ops.embed_vis(st.p("lang_model.model.embed_tokens.weight"), ids_d, vix_d, vis_all)
        dec = self._decoder()
        L = ops._L()
        need = L.nv_decoder_workspace_bytes(dec, M)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty((need,), dtype=torch.uint8, device=dev)
        want_all = return_rows == "all"
        hs = torch.empty((B, d), dtype=BF16, device=dev)
        hs_all = torch.empty((M, d), dtype=BF16, device=dev) if want_all else None
        rc = L.nv_decoder_extend(dec, x.data_ptr(), pos_d.data_ptr(), crow_d.data_ptr(), grow_d.data_ptr(), self.kv0.data_ptr(),
                                 self.attn.data_ptr(), self.lse.data_ptr(), last_d.data_ptr(), hs.data_ptr(), ops._p(hs_all), M, B, Lmax, cap,
                                 qmin, None, self._ws.data_ptr(), self._ws.numel(), ops._st())
        _lib.check(rc, "nv_decoder_extend")
        if m.fp8 is not None and M > 16:
            m.fp8.invalidate()             # the layer loop's overlapped pre-pass wrote the two de-quantisation panels
        self.state = new_state
        self.last_stats = {"prefix": P, "new": n, "block_rows": M}
        if want_all:
            return hs_all, (off, n)
        return hs

    # ------------------------------------------------------------------ generation
    @torch.no_grad()
    def logits_last(self, Hs_last):
        """lm_head on [B, d] -> fp32 [B, V] with the special ids at -inf (modified_lm.py:119-124)."""
        cfg, st = self.model.cfg, self.model.store
        lg = ops.gemm_bf16(ops.NT, Hs_last, st.lm_head_padded())[:, :cfg.vocab_size].float()
        lg[:, list(cfg.special_token_ids)] = float("-inf")
        return lg

    @torch.no_grad()
    def generate(self, ids_list, vis_idx_list=None, vis_all=None, max_new_tokens=50, eos_token_id=2, pad_token_id=0,
                 trie=None, do_sample=False, temperature=1.0, top_k=50, top_p=1.0, repetition_penalty=1.0, min_new_tokens=0):
        """Greedy decoding with HF's bookkeeping (`generate(do_sample=False)`): finished rows emit `pad_token_id`, the
        loop ends when every row has produced `eos_token_id` or after `max_new_tokens`.  `trie` (tools/trie.py protocol:
        `.root`, `.get_child_index(node)`, `.get_next_node(node, w)`) constrains each step like TrieLogitsProcessor.
        do_sample=True (tasks/agents/llava.py:58-62 forwards `--do_sample --temperature`): HF's `sample()` -- after the mask and
        the trie, logits / temperature, the default top-k (50) warper, the top-p warper, softmax, one multinomial draw per row from
        torch's CUDA generator (same distribution as the reference; the streams of two RNG implementations cannot be compared draw by
        draw).  top_p (None or 1.0: off; else a real number in (0, 1), anything else raises ValueError): HF's TopPLogitsWarper -- with W
        the total softmax weight of the top-k survivors, a logit value stays iff the weight of the survivors with a strictly larger
        logit is < top_p * W; equal logits stay or go together (HF breaks an exact tie at the boundary by sort order), the maximum
        always stays.  do_sample=False ignores it, as HF does.
        With NAVILLM_DEVICE_SAMPLE=1 a sampled call runs the device loop too (temperature finite and > 0, top_k None or an int >= 0,
        room in the cache, an eligible trie; anything else keeps the host loop): the same distribution, drawn by
        `decode_pick_sample_kernel` from Philox counters taken from torch's CUDA generator (`torch.manual_seed` makes a run
        reproducible); `last_sample` then records the seed, the offset, temperature and top_k, and top_p when the warper is on.
        repetition_penalty (None or 1.0: off; else a finite real > 0) and min_new_tokens (None or 0: off; else an int > 0, not with a
        trie) are HF's RepetitionPenaltyLogitsProcessor and MinNewTokensLengthLogitsProcessor by the rule of DESIGN.md §4 "Logits
        processors", after the special-id mask and in front of the trie and the warpers, in every kind of decoding and on both loops;
        anything else raises ValueError.  With one of them on, `last_generate` gains "processors"; with both off the call is the call
        without them.
        Returns B lists with the new tokens only."""
        procs = _check_processors(repetition_penalty, min_new_tokens, trie)          # (checked before any work, whichever loop will run)
        if do_sample:                                              # (checked before any work, whichever loop will run)
            if top_p is None:
                top_p = 1.0
            if isinstance(top_p, bool) or not isinstance(top_p, numbers.Real) or not 0.0 < top_p <= 1.0:       # (a NaN fails the comparison)
                raise ValueError(f"KVCacheLM.generate: top_p must be None, 1.0 or a real number in (0, 1), not {top_p!r}")
            top_p = float(top_p)
        B = self.B
        self.reset()
        seqs = [list(x) for x in ids_list]
        vix = None if vis_idx_list is None else [list(v) for v in vis_idx_list]
        keys = None if vis_all is None else [("gen", r) for r in range(vis_all.shape[0])]   # constant within one call
        self.last_generate = {"loop": "host", "trie": trie is not None}
        if procs is not None:
            self.last_generate["processors"] = {"repetition_penalty": float(1.0 if repetition_penalty is None else repetition_penalty),
                                                "min_new_tokens": procs[1]}
        self.last_sample = None
        if do_sample:
            on_device = (DEVICE_SAMPLE and isinstance(temperature, (int, float)) and math.isfinite(temperature)
                         and 0.0 < float(np.float32(temperature)) < math.inf                   # (what the kernel is handed is an fp32)
                         and (top_k is None or (isinstance(top_k, int) and top_k >= 0)))
        else:
            on_device = DEVICE_GREEDY
        if on_device and max_new_tokens > 0 and max(len(x) for x in seqs) + max_new_tokens <= self.cap:
            tables = None if trie is None else self._trie_tables(trie, eos_token_id)
            if trie is None or tables is not None:                 # (an ineligible trie keeps the host loop)
                self.last_generate["loop"] = "device"
                sampler = None
                if do_sample:                                      # one Philox counter per draw, accounted like the attention-probability dropout
                    seed, offset = _fn._philox_take(self.model.device, 4 * B * max_new_tokens)
                    sampler = {"seed": int(seed), "offset": int(offset), "temperature": float(temperature),
                               "top_k": min(int(top_k or 0), 2 ** 31 - 1), "top_p": top_p}
                    self.last_sample = {k: v for k, v in sampler.items() if k != "top_p" or top_p < 1.0}
                return self._generate_on_device(seqs, vix, vis_all, keys, max_new_tokens, eos_token_id, pad_token_id, tables, sampler, procs)
        out = [[] for _ in range(B)]
        unfinished = [True] * B
        seen = None if procs is None or procs[0] == 1.0 else [set(x) for x in seqs]      # each row's own ids: no padding is ever part of a row
        nodes = [trie.root for _ in range(B)] if trie is not None else None
        for step in range(max_new_tokens):
            Hs = self.extend(seqs, vix, vis_all, keys)
            lg = self.logits_last(Hs)
            if seen is not None:
                lg = _penalise_seen(lg, seen, procs[0])
            if procs is not None and step < procs[1] and 0 <= eos_token_id < lg.shape[1]:
                lg[:, eos_token_id] = float("-inf")
            if trie is not None:
                if step > 0:
                    nodes = [trie.get_next_node(nodes[b], seqs[b][-1]) for b in range(B)]
                allow = torch.zeros(lg.shape, dtype=torch.bool)
                for b in range(B):
                    allow[b, trie.get_child_index(nodes[b])] = True
                lg = lg.masked_fill(ops.h2d(allow.logical_not(), lg.device), float("-inf"))
            if do_sample:
                if temperature != 1.0:
                    lg = lg / temperature
                if top_k and top_k < lg.shape[-1]:
                    kth = torch.topk(lg, top_k, dim=-1).values[:, -1:]
                    lg = lg.masked_fill(lg < kth, float("-inf"))
                if top_p < 1.0:
                    lg = _top_p_warp(lg, top_p)
                nxt = torch.multinomial(torch.softmax(lg, dim=-1), 1).view(-1).tolist()
            else:
                nxt = torch.argmax(lg, dim=-1).tolist()
            for b in range(B):
                t = nxt[b] if unfinished[b] else pad_token_id
                out[b].append(t)
                seqs[b].append(t)
                if vix is not None:
                    vix[b].append(-1)
                if seen is not None and unfinished[b]:
                    seen[b].add(t)                             # (a finished row's `pad` marks nothing)
                if unfinished[b] and t == eos_token_id:
                    unfinished[b] = False
            if not any(unfinished):
                break
        return out

    # ------------------------------------------------------------------ decoding (greedy or sampled) with the loop on the device
    def _trie_tables(self, trie, eos):
        """the device copy of `trie`, flattened; None when the trie is not eligible for the device loop.  The trie is mutable, so it is
        flattened on every call, but uploaded only when the arrays differ from the last call's.  The device buffers persist (fixed
        addresses under the captured graph) and grow by reallocation, which changes the graph key."""
        cfg, dev = self.model.cfg, self.model.device
        off, tok, nxt, eligible = flatten_trie(trie, eos, cfg.vocab_size, cfg.special_token_ids)
        if not eligible:
            return None
        host = (off, tok, nxt)
        same = self._trie_host is not None and all(a.shape == b.shape and np.array_equal(a, b) for a, b in zip(host, self._trie_host))
        if not same:
            t = self._trie_dev
            if t is None or t["off"].numel() < off.size or t["tok"].numel() < tok.size:
                grow = lambda k: max(1024, 2 * k)
                t = {"off": torch.zeros((grow(off.size),), dtype=I32, device=dev), "tok": torch.zeros((grow(tok.size),), dtype=I32, device=dev),
                     "nxt": torch.zeros((grow(tok.size),), dtype=I32, device=dev)}
            up = ops.h2d(torch.from_numpy(np.concatenate(host)), dev)               # one staging buffer, one H2D copy
            t["off"][:off.size].copy_(up[:off.size])
            t["tok"][:tok.size].copy_(up[off.size:off.size + tok.size])
            t["nxt"][:nxt.size].copy_(up[off.size + tok.size:])
            t["n_nodes"] = int(off.size - 1)
            self._trie_host, self._trie_dev = host, t
        return self._trie_dev

    def _greedy_state(self, max_steps):
        """persistent buffers of the device loop (fixed addresses: the step is replayed from a hipGraph)"""
        g = self._greedy
        if g is not None and g["max_steps"] >= max_steps:
            return g
        m, cfg, dev, B = self.model, self.model.cfg, self.model.device, self.B
        L = ops._L()
        n = L.nv_decode_state_ints(B)
        vp = m.store.vocab_pad
        g = {"max_steps": max(max_steps, 64), "graphs": {},        # which pick (free / trie) -> (key, captured hipGraph)
             "node": torch.zeros((B,), dtype=I32, device=dev),     # each sample's trie node (the trie pick only)
             "rng": torch.zeros((2,), dtype=torch.int64, device=dev),   # {seed, offset} of the sampled pick: changes per call, so not a launch argument
             "state": torch.zeros((n,), dtype=I32, device=dev), "hs": torch.zeros((B, cfg.hidden_size), dtype=BF16, device=dev),
             "x": torch.zeros((B, cfg.hidden_size), dtype=BF16, device=dev), "logits": torch.zeros((B, vp), dtype=BF16, device=dev),
             "seen": torch.zeros((B, (cfg.vocab_size + 31) // 32), dtype=I32, device=dev),   # each row's seen-id bitmap (the processors only)
             "fin_host": [torch.zeros((B,), dtype=I32).pin_memory() for _ in range(3)]}     # landing buffers of the lagging `fin` poll
        g["out"] = torch.zeros((g["max_steps"], B), dtype=I32, device=dev)
        self._greedy = g
        return g

    def _greedy_step(self, g, eos, pad, stream, dec, trie=None, sampler=None, procs=None):
        """`dec`: the native decoder, resolved by the caller BEFORE any stream capture (nothing here may allocate or rebuild);
        `trie`: the device tables of `_trie_tables` -> the step picks among the children of g["node"];
        `sampler`: temperature, top_k and top_p -> the step draws its token, keyed by the two words in g["rng"];
        `procs`: (p32, min_new) of `_check_processors` -> nv_decoder_proc_step, the same step with the processors over g["seen"];
        None takes the symbols the call took before there were processors"""
        m, cfg, st = self.model, self.model.cfg, self.model.store
        sp = cfg.special_token_ids
        head = (dec, g["hs"].data_ptr(), st.p("lang_model.model.embed_tokens.weight").data_ptr(), st.lm_head_padded().data_ptr(), st.vocab_pad,
                cfg.vocab_size, sp[0], len(sp))
        tail = (g["logits"].data_ptr(), g["x"].data_ptr(), g["state"].data_ptr(), g["out"].data_ptr(), g["max_steps"], self.kv0.data_ptr(),
                self.attn.data_ptr(), self.lse.data_ptr(), self.B, self.cap, eos, pad, self._ws.data_ptr(), self._ws.numel(), stream)
        tr = (None, None, None, 0, None) if trie is None else (trie["off"].data_ptr(), trie["tok"].data_ptr(), trie["nxt"].data_ptr(),
                                                               trie["n_nodes"], g["node"].data_ptr())
        if procs is not None:
            smp = (0, 0.0, 0, 1.0, None)
            if sampler is not None:
                smp = (1, sampler["temperature"], sampler["top_k"], min(max(float(np.float32(sampler["top_p"])), float(np.finfo(np.float32).tiny)), 1.0),
                       g["rng"].data_ptr())
            _lib.check(ops._L().nv_decoder_proc_step(*head, *tr, *smp, g["seen"].data_ptr(), g["seen"].shape[1], procs[0], procs[1], *tail),
                       "nv_decoder_proc_step")
        elif sampler is not None:
            # what the kernel is handed is an fp32: a top_p that rounds to 1 is off, one that rounds to 0 keeps the maximum alone either way
            p32 = max(float(np.float32(sampler["top_p"])), float(np.finfo(np.float32).tiny))
            if p32 < 1.0:
                _lib.check(ops._L().nv_decoder_sample_topp_step(*head, *tr, sampler["temperature"], sampler["top_k"], p32, g["rng"].data_ptr(),
                                                                *tail), "nv_decoder_sample_topp_step")
            else:
                _lib.check(ops._L().nv_decoder_sample_step(*head, *tr, sampler["temperature"], sampler["top_k"], g["rng"].data_ptr(), *tail),
                           "nv_decoder_sample_step")
        elif trie is None:
            _lib.check(ops._L().nv_decoder_greedy_step(*head, *tail), "nv_decoder_greedy_step")
        else:
            _lib.check(ops._L().nv_decoder_trie_step(*head, *tr, *tail), "nv_decoder_trie_step")

    @torch.no_grad()
    def _generate_on_device(self, seqs, vix, vis_all, keys, max_new_tokens, eos, pad, trie=None, sampler=None, procs=None):
        """prefill through `extend` (host-built indices, once), then max_new_tokens replays of ONE captured step
        (nv_decoder_greedy_step: lm_head -> masked argmax + finished/pad bookkeeping -> cache indices -> embedding -> decoder layers;
        with `trie`, the device tables of `_trie_tables`: nv_decoder_trie_step, the argmax over the children of each row's trie node;
        with `sampler`: nv_decoder_sample_step / nv_decoder_sample_topp_step, a draw among the same candidates;
        with `procs`: nv_decoder_proc_step, any of these with the repetition penalty and the minimum length).
        The host never waits for a token: it polls the `fin` flags two steps behind and trims the output where HF would have stopped."""
        B, dev = self.B, self.model.device
        g = self._greedy_state(max_new_tokens)
        L = ops._L()
        dec = self._decoder()
        need = L.nv_decoder_workspace_bytes(dec, B)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty((need,), dtype=torch.uint8, device=dev)
        kind = trie is not None                                # which captured graph: free / trie, and ("sample", free / trie)
        if sampler is not None:
            kind = ("sample", kind)
        if procs is not None:                                  # processor-on graphs are kinds of their own: the plain ones stay captured
            kind = ("proc", kind)
        if USE_HIP_GRAPH and kind not in g["graphs"]:
            # one eager step on a scratch state BEFORE the prefill: the kernels' first-use initialisation (hipFuncSetAttribute, device
            # queries) must not happen inside a stream capture.  It writes cache row 0 of every sample, which the prefill rewrites.
            g["state"].zero_()
            if trie is not None:
                g["node"].zero_()
            if procs is not None:
                g["seen"].zero_()                              # the scratch step marks what it emits; the upload below resets every word
            self._greedy_step(g, eos, pad, ops._st(), dec, trie, sampler, procs)
        Hs = self.extend(seqs, vix, vis_all, keys)
        assert self._decoder() is dec, "the decoder table changed between prefill and decode"
        n = g["state"].numel()
        init = np.zeros(n, np.int32)
        init[2 * B:3 * B] = [len(x) for x in seqs]
        if procs is None:
            g["state"].copy_(ops.h2d(torch.from_numpy(init), dev))
        else:                                                  # the prompts' bitmap rides on the same H2D copy
            bm = _seen_bitmap(seqs, self.model.cfg.vocab_size) if procs[0] != 1.0 else np.zeros(tuple(g["seen"].shape), np.uint32)
            up = ops.h2d(torch.from_numpy(np.concatenate([init, bm.view(np.int32).reshape(-1)])), dev)
            g["state"].copy_(up[:n])
            g["seen"].copy_(up[n:].view(g["seen"].shape))
        g["hs"].copy_(Hs)
        key = (self._dec_key, self._ws.data_ptr(), eos, pad, g["out"].data_ptr())
        if trie is not None:                                   # the tables' addresses and the node count are frozen launch arguments too
            g["node"].zero_()                                  # every row starts at the root
            key += (trie["off"].data_ptr(), trie["tok"].data_ptr(), trie["nxt"].data_ptr(), trie["n_nodes"], g["node"].data_ptr())
        if sampler is not None:                                # so are the three settings; the seed and the offset travel through g["rng"]
            key += (sampler["temperature"], sampler["top_k"], sampler["top_p"], g["rng"].data_ptr())
            words = np.array([sampler["seed"], sampler["offset"]], dtype=np.uint64).view(np.int64)
            g["rng"].copy_(ops.h2d(torch.from_numpy(words), dev))
        if procs is not None:                                  # and the processors' two settings and the bitmap's address
            key += (procs[0], procs[1], g["seen"].data_ptr())
        if USE_HIP_GRAPH and g["graphs"].get(kind, (None, None))[0] != key:
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream())
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                self._greedy_step(g, eos, pad, torch.cuda.current_stream().cuda_stream, dec, trie, sampler, procs)
            g["graphs"][kind] = (key, graph)                   # capture enqueues nothing: the first replay is step 0
        events = []
        steps = 0
        for t in range(max_new_tokens):
            if USE_HIP_GRAPH:
                g["graphs"][kind][1].replay()
            else:
                self._greedy_step(g, eos, pad, ops._st(), dec, trie, sampler, procs)
            steps += 1
            if len(events) >= 2:                               # flags as of two steps ago: the host stays ahead of the GPU
                ev, snap = events.pop(0)
                ev.synchronize()
                if bool(snap.all()):
                    break
            snap = g["fin_host"][t % 3]                        # at most two polls are outstanding
            snap.copy_(g["state"][B:2 * B], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            events.append((ev, snap))
        toks = g["out"][:steps].cpu().numpy()                  # [steps, B]; syncs
        if int(g["state"][7 * B + 3].item()):
            raise RuntimeError("KVCacheLM.generate: a sample's K/V cache filled up during decoding (prompt length + max_new_tokens > capacity)")
        # HF stops after the step in which the last unfinished row emitted eos: trim the steps the lagging poll let through
        fin = np.zeros(B, bool)
        keep = steps
        for t in range(steps):
            fin |= toks[t] == eos
            if fin.all():
                keep = t + 1
                break
        toks = toks[:keep]
        lens = g["state"][2 * B:3 * B].cpu().numpy()
        # the cache now also holds the generated tokens (all `steps` of them): record it so a later extend() reuses / overwrites correctly
        full = g["out"][:steps].cpu().numpy()
        self.state = [(np.concatenate([np.asarray(seqs[b], np.int64), full[:, b].astype(np.int64)])[:int(lens[b])],
                       np.concatenate([self.state[b][1], np.zeros(steps, np.int64)])[:int(lens[b])]) for b in range(B)]
        return [toks[:, b].tolist() for b in range(B)]
