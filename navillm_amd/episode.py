"""Training with the prompt's static prefix computed ONCE per episode (an MI355X-first restructuring of the rollout's
training loop; no counterpart in the reference).

The reference re-runs the whole ~650-token prompt through the LM forward AND backward at every navigation step
(tasks/agents/mp3d_agent.py:726,756), although
  * ~530 of those tokens -- everything up to "### History:" (instruction + fixed template text) -- are identical at every
    step of an episode, and
  * the weights do not change inside an episode: `optimizer.step()` runs only between episodes (train.py:86-89), the per-step
    `backward()`s just accumulate into `.grad`.
So the prefix's hidden states, K and V are the same tensors at every step, and the episode's gradient
  sum_t dL_t/dW  =  sum_t [suffix_t part]  +  backprop_prefix( sum_t dL_t/d(K,V of the prefix) )
because backpropagation is linear in the upstream gradient.  This module does exactly that:
  begin()   prefix forward once (activations kept; post-RoPE K/V written into a per-layer cache in HBM);
  step      only the step's suffix rows (history entries, candidates, hints, <cls_1>: ~60-130 tokens) go through the layers,
            attending to the cached prefix; the K/V gradients they send into the prefix rows are summed in fp32 per layer (by the
            step's own backward, or -- default -- by finish());
  finish()  ONE backward through the prefix with the accumulated K/V gradients injected at every layer (default: through every
            token row of the episode, see "Round 3b" below).
Per episode of 6 steps: 530 + 6*120 token-rows forward and backward instead of 6*650 -- about a third of the GEMM work --
at the price of keeping the prefix activations and caches resident (288 GB of HBM make that a non-issue: 17 GB at 7B, B=8).

Exactness: same function, same weights, same rounding points per op; what differs from the per-step recompute is (a) RoPE
positions are counted from each sample's first token instead of over the batch's left padding (scores depend on position
differences only: identical up to bf16 rounding of the rotated q/k, as in navillm_amd/kvcache.py), (b) summation order of
the prefix's weight gradients (one GEMM over the summed upstream gradient instead of six accumulations).  Parity against the
per-step recompute is asserted in tests/test_episode_gpu.py (logits per step, every gradient buffer after the episode).

Weight gradients are DEFERRED (round 3, `NAVILLM_EPISODE_DEFER=wgrad`; `none` restores the per-step form): a suffix step has only
~500-900 token rows, so its four weight-gradient GEMMs per layer contract over 8-14 K-tiles -- three rounds of 256x256 output
tiles that are all prologue, epilogue and a read-modify-write of the 400 MB gradient slice.  With 288 GB of HBM the GEMM
operands can simply stay: every step leaves its Linear inputs (n1, attn, n2, h) and output gradients (dqkv, dx1, dgu, dx) in
per-layer episode buffers behind the prefix's rows (131 KB per token row and layer: ~33 GB at 7B for a 6-step episode of B=8),
and `finish()` runs ONE weight-gradient GEMM per weight over all rows of the episode -- fp32 accumulation across the whole
episode and a single bf16 rounding, where the per-step form (and the reference's autograd) round after every step.

Round 3b: the WHOLE backward of the suffix steps is deferred too (`NAVILLM_EPISODE_DEFER=all`, the default).  A step's
`backward()` then only records the gradient of its B output rows; `finish()` walks the layers ONCE for every token row of the
episode -- prefix rows and all steps' blocks side by side, ~7 700 rows -- so the four dgrad GEMMs per layer and the row kernels
run at large-M efficiency instead of six times at M ~ 600, the attention backward of ALL steps is one launch per kernel over
these row buffers (nv_attn_bwd_episode_bf16; `NAVILLM_EPISODE_ATTN_BWD=steps`: one strided backward per step over the K/V
cache), the prefix's own causal attention separately, and each step's visual-token gradient is then sent into that step's
scene-encoder / fusion graph, which was kept alive (the step's forward hands the LM a detached copy).  Nothing reads `.grad`
between the steps of an episode -- `optimizer.step()` only runs after it (train.py:86-89) -- so the result is the same sum of
gradients.  What is kept per token row and layer: x, n1, qkv, attn, x1, n2, gu, h (131 KB at 7B) + the per-step lse.  A step's
rows are packed sample after sample (no padding to the longest suffix).

`NavModel.begin_episode` / `finish_episode` switch it on per episode; `bench.py` measures it by default (`--mode prefix_reuse`)
and the reference's per-step recompute beside it (`--mode recompute`).  Its gradients are pinned to the reference's own run of a
3-step episode by fixture G12 (tests/test_parity_gpu.py).
"""
import os

import numpy as np
import torch

from . import debug
from . import layer
from . import ops

BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32


def prefix_ids_from_prompts(tokenizer, prompts):
    """For callers that hold prompt STRINGS (the reference's agents): token ids of each prompt's static prefix = the longest common
    prefix of tokenise(prompt) and tokenise(text up to "### History:") -- the LCP guards against a sub-word merge across the cut."""
    from .prompts import static_prefix
    out = []
    for p in prompts:
        full = tokenizer(p, add_special_tokens=True)["input_ids"]
        head = tokenizer(static_prefix(p), add_special_tokens=True)["input_ids"]
        n = 0
        while n < min(len(full), len(head)) and full[n] == head[n]:
            n += 1
        out.append(list(full[:n]))
    return out


class _SuffixLM(torch.autograd.Function):
    """the step's suffix rows through the decoder over the cached prefix -> final-norm hidden state of each sample's last token.
    mode "all": `vis_all` arrives detached (the live tensor, with its encoder / fusion graph, waits in step["vis_live"]), the backward
    only records dH; finish() does the rest."""

    @staticmethod
    def forward(ctx, vis_all, anchor, ep, step):
        Hs, saved = ep._step_forward(step, vis_all if step.get("vis_live") is None else step["vis_live"].detach())
        ctx.ep, ctx.saved, ctx.has_vis = ep, saved, vis_all is not None
        return Hs

    @staticmethod
    def backward(ctx, dH):
        if ctx.saved.get("batched"):
            # accumulate: a second backward through the same step (retain_graph, two losses on one output) adds, as autograd would
            ctx.saved["dH"] = dH.contiguous().clone() if ctx.saved["dH"] is None else ctx.saved["dH"] + dH
            return None, None, None, None
        dvis = ctx.ep._step_backward(ctx.saved, dH.contiguous())
        return (dvis if ctx.has_vis else None), None, None, None


class PrefixEpisode:
    def __init__(self, model, batch_size, capacity=1024, max_length=1024, samples_per_episode=None):
        cfg = model.cfg
        self.m, self.B, self.cap = model, batch_size, capacity
        # round 5, accumulation window (`begin(..., window=True)`): `batch_size` prefix slots hold the samples of SEVERAL successive
        # episodes of `samples_per_episode` prompts each -- see `_begin_window`
        self.Bs = int(samples_per_episode or batch_size)
        assert self.B % self.Bs == 0
        # the tokenizer's `max_length` (modified_lm.py:57,77-87: left truncation at 1024): a prompt that reaches it was cut from the LEFT
        # and no longer starts with the episode's prefix -- independent of how many rows per sample the K/V cache holds
        self.max_length = int(max_length)
        d, L, H = cfg.hidden_size, cfg.num_layers, cfg.num_heads
        dev = model.device
        rows = batch_size * capacity
        # the K/V-cache layout (per-layer post-RoPE q|k|v slab, attention outputs, statistics, the dO / dqkv staging rows) serves the steps that
        # run AT ONCE over the cached prefix -- per-step-forward episodes, no-grad steps, the `steps` forms of the attention.  Teacher-forced
        # episodes and accumulation windows read the episode row buffers in place and never touch it: it is allocated on first use
        # (`_kv_layout`; ADVICE r5: a B = 1 x 8 window carried ~9 GB of it for nothing at 7B)
        self.cache = self.attn_buf = self.lse = None
        self.dout_full = self.dqkv_full = None
        self.dkv_acc = [torch.zeros((rows, 2 * d), dtype=F32, device=dev) for _ in range(L)]
        self.kv0 = torch.zeros((batch_size,), dtype=I32, device=dev)
        self.prefix = None
        self._slab = {}
        self.stats = {"prefix_rows": 0, "suffix_rows": []}
        mode = os.environ.get("NAVILLM_EPISODE_DEFER", "all")
        if os.environ.get("NAVILLM_EPISODE_DEFER_WGRAD", "1") == "0":
            mode = "none"
        assert mode in ("all", "wgrad", "none"), mode
        self.mode = mode
        self.defer_wgrad = mode != "none"
        self.lse_s = []                                       # mode "all": per step, per layer lse [B, H, cap] (1 MB each at B = 8)
        self._lse_ptrs = {}                                   # ... and, per step slot, the device table of its L slab pointers
        self.fuse_kvacc = os.environ.get("NAVILLM_EPISODE_FUSE_KVACC", "1") != "0"
        self._E, self._E32, self._ecap, self._cursor, self._last_rows = None, None, 0, 0, 0
        self._seg_total = 0                                   # suffix rows of the episode so far that earlier segments already flushed

    # ------------------------------------------------------------------ helpers
    def _kv_layout(self):
        """the K/V-cache layout's buffers, built when a step first needs them (see __init__)"""
        if self.cache is not None:
            return
        cfg, dev = self.m.cfg, self.m.device
        d, L, H = cfg.hidden_size, cfg.num_layers, cfg.num_heads
        rows = self.B * self.cap
        self.cache = [torch.zeros((rows + 1, 3 * d), dtype=BF16, device=dev) for _ in range(L)]   # + a junk row for padding rows
        self.attn_buf = [torch.zeros((rows + 1, d), dtype=BF16, device=dev) for _ in range(L)]      # (+ junk row: steps are scattered back in finish())
        self.lse = [torch.zeros((self.B, H, self.cap), dtype=F32, device=dev) for _ in range(L)]
        self.dout_full = torch.zeros((rows + 1, d), dtype=BF16, device=dev)
        self.dqkv_full = torch.zeros((rows + 1, 3 * d), dtype=BF16, device=dev)
        if self.prefix is not None:
            self.prefix["cache_valid"] = False         # (whatever ran before did not write the prefix's K/V there)

    def _buf(self, tag, shape, dtype=BF16):
        """grow-only scratch tensors keyed by tag (no allocator traffic inside a step)"""
        n = int(np.prod(shape))
        t = self._slab.get(tag)
        if t is None or t.numel() < n or t.dtype != dtype:
            # 1/8 of head room: the row count of a step / an episode wanders by a few per cent, and every new maximum would otherwise
            # free and re-allocate the slab (hipFree synchronises: tens of ms when the [R, 2 ff] ones move)
            t = torch.empty((n + n // 8 + 64,), dtype=dtype, device=self.m.device)
            self._slab[tag] = t
        return t[:n].view(*shape)

    _EWIDTH = {"n1": (1, 0), "attn": (1, 0), "n2": (1, 0), "h": (0, 1), "dqkv": (3, 0), "dx1": (1, 0), "dgu": (0, 2), "dxo": (1, 0)}
    # mode "all": forward activations only (the gradients of a layer are produced and consumed inside finish()'s layer iteration)
    _EWIDTH_ALL = {"x": (1, 0), "n1": (1, 0), "qkv": (3, 0), "attn": (1, 0), "x1": (1, 0), "n2": (1, 0), "gu": (0, 2), "h": (0, 1)}

    def _ensure_rows(self, rows):
        """per-layer episode buffers [capacity, width] for every token row the episode has pushed through the decoder so far --
        prefix rows first, then each step's block.  mode "wgrad": the Linear inputs (n1, attn, n2, h) and output gradients (dqkv, dx1,
        dgu, dxo); mode "all": every forward activation the backward needs (+ the two fp32 rstd vectors).  Grow-only; growing
        mid-episode copies the rows already written (first episodes only)."""
        if self._E is not None and rows <= self._ecap:
            return
        cfg, dev = self.m.cfg, self.m.device
        d, ff = cfg.hidden_size, cfg.intermediate_size
        widths = self._EWIDTH_ALL if self.mode == "all" else self._EWIDTH
        cap = int(rows * (1.5 if self._cursor else 1.1)) + 64      # growing mid-episode copies: do it rarely
        if not self._rows_fit(cap):
            cap = rows + 64                                        # no head room then
            if not self._rows_fit(cap):
                raise RuntimeError(
                    f"prefix-reuse training: the episode buffers for {rows} token rows need {self._row_bytes() * cap / 2**30:.0f} GiB "
                    f"({self._row_bytes() // 1024} KiB per row over {cfg.num_layers} layers) and do not fit the free device memory; run long "
                    "episodes with NAVILLM_EPISODE_DEFER=none (every step backpropagates at once, nothing is kept) or finish the "
                    "episode earlier")
        new, new32 = [], []
        for i in range(cfg.num_layers):
            bufs, b32 = {}, {}
            for name, (cd, cf) in widths.items():
                t = torch.empty((cap, cd * d + cf * ff), dtype=BF16, device=dev)
                if self._E is not None and self._cursor:
                    t[: self._cursor].copy_(self._E[i][name][: self._cursor])
                bufs[name] = t
            if self.mode == "all":
                for name in ("r1", "r2"):
                    t = torch.empty((cap,), dtype=F32, device=dev)
                    if self._E32 is not None and self._cursor:
                        t[: self._cursor].copy_(self._E32[i][name][: self._cursor])
                    b32[name] = t
            new.append(bufs)
            new32.append(b32)
            if self._E is not None:
                if self._cursor and self.prefix is not None:
                    # growing mid-episode: the prefix's saved activations are VIEWS of the old buffers -- point them at the copies,
                    # or the old set stays alive until finish() and the fit check above under-estimates the peak
                    a, Mp = self.prefix["layers"][i], self.prefix["Mp"]
                    for name in list(a):
                        if name in bufs:
                            a[name] = bufs[name][:Mp]
                    if b32:
                        a["rstd1"], a["rstd2"] = b32["r1"][:Mp], b32["r2"][:Mp]
                self._E[i] = None                      # release layer by layer: never two full copies resident
                if self._E32 is not None:
                    self._E32[i] = None
        self._E, self._E32, self._ecap = new, new32, cap

    def _row_bytes(self):
        cfg = self.m.cfg
        widths = self._EWIDTH_ALL if self.mode == "all" else self._EWIDTH
        per = sum(cd * cfg.hidden_size + cf * cfg.intermediate_size for cd, cf in widths.values()) * 2 + (8 if self.mode == "all" else 0)
        return per * cfg.num_layers

    def _budget_bytes(self):
        """upper bound for the episode buffers: NAVILLM_EPISODE_MAX_GB, default 30 % of the device's memory (86 GB of 288) -- a long
        episode otherwise sizes them for whatever happens to be free (150 GB after the first 64-step run) and everything allocated
        later in the process finds the card full; longer episodes simply run in more segments"""
        gb = float(os.environ.get("NAVILLM_EPISODE_MAX_GB", "0") or 0)
        if gb > 0:
            return int(gb * (1 << 30))
        if self.m.device.type != "cuda":
            return 1 << 62
        return int(0.30 * torch.cuda.get_device_properties(self.m.device).total_memory)

    def release_buffers(self):
        """drop the per-layer episode buffers and the batched backward's scratch (they are re-created, sized for the next episode, by
        begin()); only between episodes"""
        assert self.prefix is None or self._cursor == 0 or not self.prefix.get("recs"), "release_buffers() inside an open episode"
        self._E, self._E32, self._ecap = None, None, 0
        for k in [k for k in self._slab if k.startswith("b.") or k.startswith("lz.")]:
            del self._slab[k]
        self._last_rows = 0
        if self.m.device.type == "cuda":
            torch.cuda.empty_cache()

    def _poison_release(self):
        """NAVILLM_POISON=1 (navillm_amd/debug.py): the episode is over -- whatever it left in the row buffers, the statistics slabs, the
        K/V-cache slabs, the fp32 K/V-gradient accumulators and the scratch becomes NaN, so that state surviving into the next episode
        cannot pass for a plausible number; then the canaries around every live buffer are verified.  (`dout_full`, `kv0` and
        `zeros_md` are zero BY CONTRACT and stay.)"""
        if not debug.POISON:
            return
        for group in (self._E or []), (self._E32 or []):
            for bufs in group:
                for t in (bufs or {}).values():
                    debug.poison_(t)
        for k, t in self._slab.items():
            if k != "zeros_md":
                debug.poison_(t)
        for per_step in self.lse_s:
            for t in per_step:
                debug.poison_(t)
        for t in self.dkv_acc + ((self.lse + [self.dqkv_full]) if self.cache is not None else []):
            debug.poison_(t)
        for t in (self.cache + self.attn_buf) if self.cache is not None else []:
            debug.poison_(t, masked_reads=True)        # the K/V-cache layout: read under the causal mask by design (debug.poison_)
        debug.check_guards("at the end of a prefix-reuse episode")

    def _rows_fit(self, cap):
        """would episode buffers of `cap` rows fit?  (what is held now is released layer by layer while the new ones are built)"""
        if self.m.device.type != "cuda":
            return True
        free, _ = torch.cuda.mem_get_info(self.m.device)
        cfg = self.m.cfg
        held = self._row_bytes() * self._ecap if self._E is not None else 0
        one_layer = self._row_bytes() // cfg.num_layers * cap
        # the batched backward's [R, .] scratch (dx x2, dx1, dattn, dn, dqkv, dgu, dh = 8 d + 3 ff per row: about one layer's worth of
        # episode buffers) is grow-only as well: what it already holds is credited, what `cap` rows would need is charged
        scratch_have = sum(t.numel() * t.element_size() for k, t in self._slab.items() if k.startswith("b."))
        scratch = max(0, (8 * cfg.hidden_size + 3 * cfg.intermediate_size) * 2 * cap * 9 // 8 - scratch_have)
        reserve = 6 << 30                                       # allocator slack / fragmentation, the step scratch
        # (what the caching allocator holds but has not handed out is fragmented: count half of it)
        cached = torch.cuda.memory_reserved(self.m.device) - torch.cuda.memory_allocated(self.m.device)
        return self._row_bytes() * cap - held + one_layer + scratch + reserve <= free + cached // 2

    _DST = {"n1": (1, 0), "qkv": (3, 0), "attn": (1, 0), "x1": (1, 0), "n2": (1, 0), "gu": (0, 2), "h": (0, 1), "x2": (1, 0)}
    _DST32 = {"rstd1": "r1", "rstd2": "r2"}

    def _dst(self, tag, i, rows, names, E, allm):
        """where layer i's forward results `names` go for the token rows `rows` (the `dst` mapping of navillm_amd/layer.py): this block
        of the episode buffers where finish() reads them again (E: the layer's buffers or None; allm: mode "all" keeps everything),
        otherwise the grow-only scratch `<tag><i>.<name>`, so that rows of varying number do not churn the allocator"""
        cfg = self.m.cfg
        n, out = rows.stop - rows.start, {}
        for name in names:
            r = self._DST32.get(name)
            if E is not None and name in E:
                out[name] = E[name][rows]
            elif r is not None:
                out[name] = self._E32[i][r][rows] if allm else self._buf(f"{tag}{i}.{r}", (n,), F32)
            elif allm and name == "x2" and i + 1 < cfg.num_layers:
                out[name] = self._E[i + 1]["x"][rows]      # a layer's output IS the next layer's saved input
            else:
                cd, cf = self._DST[name]
                out[name] = self._buf(f"{tag}{i}.{name}", (n, cd * cfg.hidden_size + cf * cfg.intermediate_size))
        return out

    def has_pending_gradients(self):
        """an open episode whose steps ran a backward(): in the deferred forms those gradients exist only here until finish()"""
        P = self.prefix
        return P is not None and (P.get("kv_steps", 0) > 0 or P.get("segments", 0) > 0 or
                                  any(r.get("dH") is not None or r.get("targets") is not None for r in P.get("recs", ())))

    def assert_no_pending_gradients(self, what):
        if self.has_pending_gradients():
            raise RuntimeError(f"{what} inside an open prefix-reuse episode whose steps already ran backward(): its LM / embedding / "
                               "encoder gradients are handed over by model.finish_episode() -- call that first (under `with "
                               "model.final_backward():` when data-parallel), or model.episode_abort() to drop the episode")

    # ------------------------------------------------------------------ prefix forward, once per episode
    @torch.no_grad()
    def begin(self, prefix_ids, teacher_forced=False, window=False):
        """prefix_ids: B python lists of token ids (no visual tokens) -- the part of every prompt of this episode that never changes.
        teacher_forced (round 4; mode "all" only): the steps' LM FORWARD is deferred to finish() too -- see `_forward_lazy`.
        window (round 5; teacher-forced only): the episode joins the open accumulation window -- see `_begin_window`."""
        if window:
            assert teacher_forced, "an accumulation window batches teacher-forced episodes only"
            return self._begin_window(prefix_ids)
        assert self.Bs == self.B, "this PrefixEpisode was built for accumulation windows"
        m, cfg, st = self.m, self.m.cfg, self.m.store
        B, cap, H, hd, eps, L = self.B, self.cap, cfg.num_heads, cfg.head_dim, cfg.rms_norm_eps, cfg.num_layers
        self.assert_no_pending_gradients("begin_episode()")
        assert len(prefix_ids) == B
        lens = np.array([len(p) for p in prefix_ids], dtype=np.int32)
        assert lens.min() > 0 and lens.max() < cap
        special = set(cfg.special_token_ids)
        assert not any(t in special for p in prefix_ids for t in p), "the static prefix must not contain visual tokens"
        Mp = int(lens.sum())
        cu = np.zeros(B + 1, np.int32)
        cu[1:] = np.cumsum(lens)
        ids = np.concatenate([np.asarray(p, np.int32) for p in prefix_ids])
        pos = np.concatenate([np.arange(n, dtype=np.int32) for n in lens])
        crow = np.concatenate([b * cap + np.arange(n, dtype=np.int32) for b, n in enumerate(lens)])
        dev = m.device
        ids_d, pos_d, crow_d, cu_d, lens_d = (ops.h2d(torch.from_numpy(a), dev) for a in (ids, pos, crow, cu, lens))
        vix = torch.full((Mp,), -1, dtype=I32, device=dev)
        zero_pos0 = torch.zeros((B,), dtype=I32, device=dev)
        Lmax = int(lens.max())
        d, ff = cfg.hidden_size, cfg.intermediate_size
        layers = []
        defer = self.defer_wgrad
        allm = self.mode == "all"
        if defer:
            self._cursor = 0
            # sized for the WHOLE previous episode's suffix rows (first episode: about as many as the prefix has) -- or, when that does
            # not fit the free memory (long-horizon episodes), for the largest share of it that does: the episode then runs in segments
            # (flush_segment).  The buffers only grow here, between episodes: growing mid-episode copies, fragments the allocator and
            # made the first 64-step runs die with 24 GiB reserved-but-unusable.
            want = max(self._last_rows, Mp)
            budget = self._budget_bytes()
            # (round 5: only when the buffers would have to GROW -- `_rows_fit` asks the driver for the free memory, and that query waits
            # for the device to drain: called at every begin() it serialised the host's preparation of the next episode's steps with the
            # previous episode's backward, 2-4 % of GPU idle time once the prefix forward no longer covered it)
            while (self._E is None or Mp + want > self._ecap) and want > 4096 and \
                    (self._row_bytes() * (int((Mp + want) * 1.1) + 64) > budget or not self._rows_fit(int((Mp + want) * 1.1) + 64)):
                want = int(want * 0.6)
            if self._E is not None and self._ecap > 2.5 * (Mp + want) + 4096:
                self.release_buffers()                           # a much longer episode ran before: give its rows back
            self._ensure_rows(Mp + want)
            self._seg_total = 0
            self._cursor = Mp
        lazy = bool(teacher_forced) and allm and defer
        # round 5: in a teacher-forced episode the PREFIX's forward is deferred too -- `_forward_lazy` pushes the prefix rows and all the
        # steps' rows through the decoder as ONE batch (~8 300 rows per GEMM instead of 4 272 + ~4 200: the forward layout runs 7 % faster
        # at that size, profiles/r05_gemm_vs_blaslt.txt, and every row kernel / GEMM of the forward is launched once instead of twice);
        # only the index tables are built here.  NAVILLM_EPISODE_LAZY_PREFIX: 1 (default) = always deferred; 0 = the prefix forward runs
        # now, as in round 4; auto = deferred while the GPU still has queued work, run NOW when the stream is empty (first episode, right
        # after a synchronisation: an idle GPU then gets 45 ms of prefix forward under the host's preparation of the six steps --
        # profiles/r05_episode_gaps_lazy*.txt: the first episode after a sync idles 30 ms with the prefix deferred, 16 ms without).
        # `auto` is NOT the default: which GEMM shapes an episode runs -- hence the last bits of its gradients -- would depend on GPU
        # timing, and in the driver's 20-step window it measured the same as 1 (ABAB 136.4-137.1 vs 136.4-137.2 nav-steps/s)
        lz = os.environ.get("NAVILLM_EPISODE_LAZY_PREFIX", "1")
        pending = lazy and lz != "0"
        if pending and lz == "auto" and dev.type == "cuda" and torch.cuda.current_stream(dev).query():
            pending = False
        self.prefix = dict(ids=[list(p) for p in prefix_ids], ids_np=ids, lens=lens, cu=cu_d, pos=pos_d, crow=crow_d, pos0=zero_pos0,
                           Lmax=Lmax, Mp=Mp, layers=None, steps=0, kv_steps=0, defer=defer, lens_dev=lens_d, recs=[], segments=0,
                           lazy=lazy, pending=pending, cache_valid=not pending, ids_dev=ids_d, vix_dev=vix)
        self.stats = {"prefix_rows": Mp, "suffix_rows": [], "segments_flushed": 0, "recomputed_steps": 0}
        if pending:
            # what finish() reads of the prefix's saved state: views of the episode buffers (filled by `_forward_lazy`) + the lse slabs
            self.prefix["layers"] = [dict(lse=self._buf(f"p{i}.lse", (B, H, Lmax), F32)) for i in range(L)]
            return
        self._prefix_forward()

    # ------------------------------------------------------------------ accumulation window (round 5)
    # The reference's launch line is `--batch_size 1 --gradient_accumulation_step 8` (scripts/multi_wo_pretrain.sh:16): eight episodes
    # of ONE prompt each between two optimizer steps (train.py:68,86-89).  The weights are frozen for the whole window and nothing reads
    # `.grad` inside it, so -- exactly as the steps of one episode are batched -- the teacher-forced episodes of a window can be
    # batched with one another: every `begin()` adds its samples to the window's prefix slots, every step only RESERVES its rows,
    # `finish()` of the first n - 1 episodes returns at once, and the n-th (or anything that needs the gradients: the optimizer's clip /
    # step, `model.parameters()`, a non-windowed `begin_episode`) pushes ALL prefixes and ALL steps of the window through the decoder as
    # one batch: forward, heads + losses, batched backward -- the GEMMs of a B = 1 launch line then see the rows of a B = 8 episode.
    # The kernels do not change: sample slot b of the window is sample b - sb of its episode, and table-step k of the one-launch
    # attention kernels is the k-th step of EVERY episode (a shorter episode has 0 rows there).
    def _begin_window(self, prefix_ids):
        m, cfg = self.m, self.m.cfg
        Bs, cap = self.Bs, self.cap
        assert self.mode == "all" and self.defer_wgrad, "accumulation windows need NAVILLM_EPISODE_DEFER=all"
        for k in ("NAVILLM_EPISODE_ATTN_FWD", "NAVILLM_EPISODE_ATTN_BWD"):
            assert os.environ.get(k, "episode") != "steps", f"{k}=steps shares the K/V-cache rows between episodes: not inside a window"
        assert len(prefix_ids) == Bs
        lens = np.array([len(p) for p in prefix_ids], dtype=np.int32)
        assert lens.min() > 0 and lens.max() < cap
        special = set(cfg.special_token_ids)
        assert not any(t in special for p in prefix_ids for t in p), "the static prefix must not contain visual tokens"
        P = self.prefix
        if P is not None and not P.get("window"):
            self.assert_no_pending_gradients("begin_episode()")
            P = self.prefix = None
        if P is not None:
            if P["finished"] < P["episodes"]:
                if any(r.get("targets") is not None for r in P["recs"][P["ep_rec0"]:]):
                    raise RuntimeError("begin_episode() before the previous episode of the accumulation window was finished: its steps "
                                       "already ran backward() -- call model.finish_episode() first, or model.episode_abort()")
                self._drop_open_episode()
            # the window is full, or its rows would outgrow the budget: hand over what it holds first
            rows = P["prows"] + P["srows"]
            per_ep = rows // max(P["episodes"], 1)
            if P["nb"] + Bs > self.B or self._row_bytes() * int((rows + max(per_ep, 2 * int(lens.sum()))) * 1.1 + 64) > self._budget_bytes():
                self.flush_window()
                P = None
        if P is None:
            self._cursor, self._seg_total = 0, 0
            P = self.prefix = dict(window=True, ids=[], lens=np.zeros(0, np.int32), nb=0, sb=0, episodes=0, finished=0, t=0, steps=0,
                                   kv_steps=0, defer=True, recs=[], segments=0, lazy=True, pending=True, cache_valid=False, prows=0,
                                   srows=0, ep_rec0=0, layers=None, Mp=None)
            self.stats = {"prefix_rows": 0, "suffix_rows": [], "segments_flushed": 0, "recomputed_steps": 0, "window_episodes": 0}
        P["sb"], P["t"], P["ep_rec0"], P["ep_srows0"] = P["nb"], 0, len(P["recs"]), P["srows"]
        P["ids"] += [list(p) for p in prefix_ids]
        P["lens"] = np.concatenate([P["lens"], lens])
        P["nb"] += Bs
        P["episodes"] += 1
        P["prows"] += int(lens.sum())
        self.stats["prefix_rows"] = P["prows"]
        self.stats["window_episodes"] = P["episodes"]

    def _drop_open_episode(self):
        """the window's current episode was begun but never finished, and none of its steps carries a loss: forget it"""
        P = self.prefix
        Bs = self.Bs
        for r in P["recs"][P["ep_rec0"]:]:
            r["step"]["vis_live"] = None
        del P["recs"][P["ep_rec0"]:]
        P["srows"] = P["ep_srows0"]
        P["prows"] -= int(P["lens"][P["sb"]:].sum())
        P["ids"], P["lens"] = P["ids"][:P["sb"]], P["lens"][:P["sb"]]
        P["nb"] -= Bs
        P["episodes"] -= 1

    def window_open(self):
        P = self.prefix
        return P is not None and bool(P.get("window"))

    @torch.no_grad()
    def _seal_window(self):
        """all the window's samples are known: the prefix index tables over every slot (what begin() builds for one episode), the
        episode buffers sized once for prefixes + steps, every step's block placed behind the prefixes"""
        P, m, cfg = self.prefix, self.m, self.m.cfg
        nb, cap, H, L = P["nb"], self.cap, cfg.num_heads, cfg.num_layers
        lens = P["lens"]
        Mp = int(lens.sum())
        cu = np.zeros(nb + 1, np.int32)
        cu[1:] = np.cumsum(lens)
        ids = np.concatenate([np.asarray(p, np.int32) for p in P["ids"]])
        pos = np.concatenate([np.arange(n, dtype=np.int32) for n in lens])
        crow = np.concatenate([b * cap + np.arange(n, dtype=np.int32) for b, n in enumerate(lens)])
        dev = m.device
        ids_d, pos_d, crow_d, cu_d, lens_d = (ops.h2d(torch.from_numpy(a), dev) for a in (ids, pos, crow, cu, lens))
        Lmax = int(lens.max())
        P.update(ids_np=ids, cu=cu_d, pos=pos_d, crow=crow_d, pos0=torch.zeros((nb,), dtype=I32, device=dev), Lmax=Lmax, Mp=Mp,
                 lens_dev=lens_d, ids_dev=ids_d, vix_dev=torch.full((Mp,), -1, dtype=I32, device=dev))
        total = Mp + P["srows"]
        self._cursor = 0                                   # (nothing is in the buffers yet: growing them copies nothing)
        if self._E is not None and self._ecap > 2.5 * total + 4096:
            self.release_buffers()
        self._ensure_rows(total)
        self._cursor = total
        for r in P["recs"]:
            r["r0"] = Mp + r["r0_rel"]
        P["layers"] = [dict(lse=self._buf(f"p{i}.lse", (nb, H, Lmax), F32)) for i in range(L)]

    def flush_window(self):
        """run the open accumulation window NOW (fewer episodes than it was sized for: the last window of an epoch, an optimizer step
        that comes early): all its gradients land in `.grad`"""
        P = self.prefix
        if P is None or not P.get("window"):
            return
        if P["finished"] < P["episodes"]:
            if any(r.get("targets") is not None for r in P["recs"][P["ep_rec0"]:]):
                raise RuntimeError("the accumulation window must hand over its gradients, but its current episode is still open: call "
                                   "model.finish_episode() after the episode's last backward() (or model.episode_abort())")
            self._drop_open_episode()
        if not P["recs"]:
            self.prefix = None
            self._cursor = 0
            return
        self._seal_window()
        self._finish_batched()

    @torch.no_grad()
    def _prefix_forward(self):
        """the prefix rows through the decoder (activations kept, post-RoPE K/V into the per-layer cache): at begin(), or -- a
        teacher-forced episode whose prefix is still pending -- when a step that cannot be deferred needs the cache"""
        m, cfg, st = self.m, self.m.cfg, self.m.store
        P = self.prefix
        B, cap, H, hd, eps, L = self.B, self.cap, cfg.num_heads, cfg.head_dim, cfg.rms_norm_eps, cfg.num_layers
        d, ff = cfg.hidden_size, cfg.intermediate_size
        Mp, Lmax, defer = P["Mp"], P["Lmax"], P["defer"]
        allm = self.mode == "all"
        # round 6: in the default form the steps' attention reads the prefix's K/V from the episode row buffers in place
        # (`_step_forward`: one table-step of nv_attn_fwd_episode_bf16), so the K/V-cache layout is neither allocated nor filled here; a
        # step that does need it (a no-grad step inside the episode, the `steps` forms) copies the rows over then (`_need_prefix_cache`)
        to_cache = not (allm and defer and os.environ.get("NAVILLM_EPISODE_ATTN_FWD", "episode") != "steps")
        if to_cache:
            self._kv_layout()
        ids_d, vix, pos_d, crow_d, cu_d, zero_pos0 = P["ids_dev"], P["vix_dev"], P["pos"], P["crow"], P["cu"], P["pos0"]
        layers = []
        x = ops.embed_vis(st.p("lang_model.model.embed_tokens.weight"), ids_d, vix, None,
                          out=self._E[0]["x"][:Mp] if allm else self._buf("pE", (Mp, d)))
        rows = slice(0, Mp)
        for i in range(L):
            lw = st.layer(i)
            # kept until finish(): grow-only slabs, so prefixes of varying length do not churn the allocator; the four Linear
            # inputs live in the episode buffers when the weight gradients are deferred (rows [0, Mp))
            E = self._E[i] if defer else None
            dst = self._dst("p", i, rows, ("n1", "rstd1", "qkv"), E, allm)
            n1, rstd1 = ops.rmsnorm_fwd(x, lw.w1, eps, out=dst["n1"], rstd=dst["rstd1"])
            qkv = ops.qkv_rope(n1, lw.Wqkv, m.rope_cos, m.rope_sin, Lmax, H, hd, out=dst["qkv"], pos_i32=pos_d)
            if to_cache:
                ops.scatter_rows_bf16_(qkv, crow_d, self.cache[i])
            if i == L - 1 and os.environ.get("NAVILLM_EPISODE_PRUNE_TOP", "1") != "0":
                # round 5: the TOP layer's prefix rows feed nothing but their K/V (no head reads a prefix row, and the steps read a layer's
                # K/V, i.e. its INPUT): attention, o_proj and the MLP of these rows were computed and never read -- the backward has
                # always skipped them (`lo = Mp`)
                layers.append(dict(x=x, n1=n1, rstd1=rstd1, qkv=qkv, attn=None, lse=None, x1=None, n2=None, rstd2=None, gu=None, h=None))
                break
            dst = self._dst("p", i, rows, ("attn", "x1", "n2", "rstd2", "gu", "h", "x2"), E, allm)
            attn = dst["attn"]
            lse = self._buf(f"p{i}.lse", (B, H, Lmax), F32)
            ops.attn_fwd_varlen(qkv, cu_d, zero_pos0, B, Lmax, H, hd, out=attn, lse2=lse)
            x1, n2, rstd2, gu, h, x2 = layer.attn_out_mlp_fwd(lw, x, attn, eps, dst)
            layers.append(dict(x=x, n1=n1, rstd1=rstd1, qkv=qkv, attn=attn, lse=lse, x1=x1, n2=n2, rstd2=rstd2, gu=gu, h=h))
            x = x2                                     # (dkv_acc needs no zero-fill: the first step SETS the prefix rows)
        P["layers"] = layers
        P["pending"] = False
        P["cache_valid"] = to_cache

    def _need_prefix_cache(self):
        """a step that runs NOW (not deferred) reads the prefix's K/V from the per-layer cache: compute the prefix if it is still
        pending, or -- it went through `_forward_lazy` with the in-place attention -- copy its K/V rows into the cache"""
        P = self.prefix
        if P.get("pending"):
            self._prefix_forward()
        self._fill_prefix_cache(P)

    def _fill_prefix_cache(self, P):
        """the prefix's post-RoPE K/V rows into the K/V-cache layout, unless they are there already"""
        had = self.cache is not None
        self._kv_layout()
        if not had:
            P["cache_valid"] = False
        if not P.get("cache_valid", True):
            for i in range(self.m.cfg.num_layers):
                ops.scatter_rows_bf16_(self._E[i]["qkv"][:P["Mp"]], P["crow"], self.cache[i])
            P["cache_valid"] = True

    def _need_prefix(self):
        """a deferred step that runs now and reads the prefix's K/V from the episode row buffers in place: only the prefix's forward"""
        if self.prefix.get("pending"):
            self._prefix_forward()

    def fits(self, ids_list):
        """can this step's prompts run over the cached prefix?  False: at least one prompt was LEFT-TRUNCATED by the tokenizer side
        (`max_length=1024, truncation_side='left'`, modified_lm.py:77-87 -- long-horizon episodes): it no longer starts with the
        registered prefix, and every hidden state of what is left differs from the cached one (the dropped tokens were attended to), so
        the exact computation is the reference's own -- the caller pushes this step through the full `_lm` path (forward + immediate
        backward into the same `.grad` buffers; the episode stays open for its deferred part).  A prompt that is NOT at the length
        limit and does not start with its prefix is a caller error and raises."""
        P = self.prefix
        sb = P["sb"] if P.get("window") else 0             # (accumulation window: this episode's samples sit in slots [sb, sb + Bs))
        assert len(ids_list) == self.Bs
        for j in range(self.Bs):
            lp = int(P["lens"][sb + j])
            if ids_list[j][:lp] == P["ids"][sb + j] and lp < len(ids_list[j]) <= self.cap:
                continue
            if len(ids_list[j]) >= min(self.cap, self.max_length):      # truncated at the tokenizer's limit, or longer than the cache
                self.stats["recomputed_steps"] += 1
                return False
            raise AssertionError("the prompt does not start with the prefix registered for this episode")
        return True

    def _segment_full(self, rows):
        """would the next step's rows overflow the episode buffers (sized between episodes, see begin())?  Then the recorded steps are
        flushed rather than the buffers grown -- except while the buffers are still small (cold start); a SINGLE step that does not fit
        always makes `_ensure_rows` grow them."""
        cap = int(os.environ.get("NAVILLM_EPISODE_MAX_ROWS", "0") or 0)
        if cap and rows > max(cap, self.prefix["Mp"] + 1):
            return True
        if rows <= self._ecap:
            return False
        # a cold start (first episode of a shape: the buffers were sized for "about as many suffix rows as prefix rows") may still grow
        # them once or twice while they are small -- so that short episodes run as ONE batch from the first one on, bit-identical to the
        # later ones; beyond ~3 prefixes' worth of rows (long-horizon episodes) the steps are flushed instead
        small = int(rows * 1.5) + 64 <= 3 * self.prefix["Mp"] + 4096 and self._row_bytes() * (int(rows * 1.5) + 64) <= self._budget_bytes()
        return not (small and self._rows_fit(int(rows * 1.5) + 64))

    # ------------------------------------------------------------------ one step: suffix rows over the cached prefix
    def lm(self, ids_list, vis_idx_list, vis_all):
        """ids_list[b]: the whole prompt of sample b (must start with its registered prefix); vis_idx_list[b][j]: row of vis_all for
        token j or -1.  -> [B, d] final-norm hidden state of every prompt's last token, differentiable w.r.t. vis_all."""
        P = self.prefix
        assert P is not None, "PrefixEpisode.begin() first"
        win = bool(P.get("window"))
        sb = P["sb"] if win else 0                 # first prefix slot of this episode's samples (accumulation window: `_begin_window`)
        B, cap = self.Bs, self.cap
        if win and P["finished"] >= P["episodes"]:
            raise RuntimeError("a navigation step after finish_episode(): begin_episode() opens the window's next episode")
        n = []
        for b in range(B):
            lp = int(P["lens"][sb + b])
            assert ids_list[b][:lp] == P["ids"][sb + b], "the prompt does not start with the prefix registered for this episode"
            assert lp < len(ids_list[b]) <= cap, "prompt longer than the cache (left truncation is not supported in this mode)"
            n.append(len(ids_list[b]) - lp)
        # the step's rows are PACKED, sample after sample (round 3b; round 2 padded every sample to the longest suffix: 6.8 % of the
        # steps' rows at the bench shape were padding that went through every GEMM and row kernel of the step)
        N = max(n)
        off = np.zeros(B + 1, np.int64)
        off[1:] = np.cumsum(n)
        M = int(off[B])
        junk = self.B * cap
        ids_new = np.full(M, self.m.cfg.pad_token_id, np.int32)
        vix_new = np.full(M, -1, np.int32)
        pos_new = np.zeros(M, np.int32)
        crow = np.full(M, junk, np.int32)
        grow = np.zeros(M, np.int32)
        last = np.zeros(B, np.int32)
        for b in range(B):
            lp = int(P["lens"][sb + b])
            s, e = int(off[b]), int(off[b + 1])
            ids_new[s:e] = ids_list[b][lp:]
            vix_new[s:e] = vis_idx_list[b][lp:]
            ar = np.arange(lp, lp + n[b], dtype=np.int32)
            pos_new[s:e] = ar
            crow[s:e] = (sb + b) * cap + ar
            grow[s:e] = (sb + b) * cap + ar
            last[b] = e - 1
        tok_rows = np.flatnonzero(vix_new >= 0)
        R = 0 if vis_all is None else int(vis_all.shape[0])
        assert tok_rows.size == R, f"{tok_rows.size} visual tokens in the step's suffix but {R} visual rows (the static prefix holds none)"
        vis_rows = np.zeros(R, np.int32)
        vis_rows[vix_new[tok_rows]] = tok_rows                 # vis row r is added at block row vis_rows[r]
        packed = np.concatenate([ids_new, vix_new, pos_new, crow, grow, last, vis_rows])
        idx = ops.h2d(torch.from_numpy(packed), self.m.device)
        parts = [idx[k * M:(k + 1) * M] for k in range(5)] + [idx[5 * M:5 * M + B], idx[5 * M + B:]]
        step = dict(M=M, N=N, n=n, off=[int(x) for x in off[:B]], Lmax=int(max(int(P["lens"][sb + b]) + n[b] for b in range(B))),
                    qmin=(int(P["lens"][sb:sb + B].min()) // 128) * 128,
                    ids=parts[0], vix=parts[1], pos=parts[2], crow=parts[3], grow=parts[4], last=parts[5], vis_rows=parts[6],
                    ids_np=ids_new, sb=sb)
        self.stats["suffix_rows"].append(int(sum(n)))
        anchor = self.m._anchor if torch.is_grad_enabled() else None
        if P.get("lazy") and torch.is_grad_enabled():
            # teacher-forced episode: nothing runs now -- the step's rows are reserved in the episode buffers and its whole LM forward
            # happens in finish() / flush_segment(), batched with every other step's (`_forward_lazy`)
            step["vis_live"] = vis_all
            step["batched"] = True
            k = P["steps"]
            P["steps"] = k + 1
            if win:
                # accumulation window: the block's place is only known when the window is sealed (behind ALL the prefixes); its slot
                # in the step tables / lse slabs is the step's index inside its own episode
                if P["t"] >= 128 or N > 1536:
                    raise RuntimeError("accumulation windows batch episodes of at most 128 steps and 1536 suffix tokens per prompt; "
                                       "open long-horizon episodes with accumulate=1")
                rec = dict(step=step, layers=[], x_last=None, rstdf=None, serial=k + 1, r0=None, r0_rel=P["srows"], defer=True, batched=True,
                           k=P["t"], dH=None, lazy=True, targets=None, scale=None)
                P["srows"] += M
                P["t"] += 1
                P["recs"].append(rec)
                return rec
            if P["recs"] and self._segment_full(self._cursor + M):
                self.flush_segment()
            r0 = self._cursor
            self._ensure_rows(r0 + M)
            self._cursor = r0 + M
            rec = dict(step=step, layers=[], x_last=None, rstdf=None, serial=k + 1, r0=r0, defer=True, batched=True, k=len(P["recs"]), dH=None,
                       lazy=True, targets=None, scale=None)
            P["recs"].append(rec)
            return rec
        if win:
            raise RuntimeError("an accumulation window holds teacher-forced TRAINING steps only (a no-grad / sampled step needs the "
                               "prefix's K/V now): open this episode with accumulate=1")
        batched_now = self.mode == "all" and P["defer"] and torch.is_grad_enabled()
        if batched_now and os.environ.get("NAVILLM_EPISODE_ATTN_FWD", "episode") != "steps":
            self._need_prefix()            # (a deferred step whose attention reads the episode buffers in place)
        else:
            self._need_prefix_cache()      # (a step that runs now over the K/V-cache layout: the prefix's K/V must be there)
        if batched_now:
            # the LM sees a detached copy; the live tensor keeps this step's scene-encoder / fusion graph alive until finish()
            step["vis_live"] = vis_all
            step["batched"] = True
            return _SuffixLM.apply(None, anchor, self, step)
        return _SuffixLM.apply(vis_all, anchor, self, step)

    def _step_forward(self, step, vis_all):
        m, cfg, st = self.m, self.m.cfg, self.m.store
        B, cap, H, hd, eps, L, d, ff = self.B, self.cap, cfg.num_heads, cfg.head_dim, cfg.rms_norm_eps, cfg.num_layers, cfg.hidden_size, \
            cfg.intermediate_size
        M, Lmax, qmin = step["M"], step["Lmax"], step["qmin"]
        k = self.prefix["steps"]
        defer = self.defer_wgrad and self.prefix["defer"]
        if self.mode == "all" and not step.get("batched"):
            defer = False                  # a step outside autograd (validation inside an episode): scratch only, the episode buffers hold
        allm = defer and bool(step.get("batched"))                                        # exactly the rows finish() will walk
        if allm and self.prefix["recs"] and self._segment_full(self._cursor + M):
            # long episodes (round 4): the rows of the steps so far no longer fit (or exceed NAVILLM_EPISODE_MAX_ROWS) -- run THEIR
            # deferred backward now (into .grad and the fp32 prefix K/V accumulators), keep the prefix open, reuse their rows
            self.flush_segment()
        r0 = self._cursor
        if defer:
            self._ensure_rows(r0 + M)
            self._cursor = r0 + M
        ks = len(self.prefix["recs"])          # lse slot: the step's index inside the current segment
        if allm:
            while len(self.lse_s) <= ks:
                self.lse_s.append([torch.zeros((B, H, cap), dtype=F32, device=m.device) for _ in range(L)])
        x = ops.embed_vis(st.p("lang_model.model.embed_tokens.weight"), step["ids"], step["vix"], vis_all,
                          out=self._E[0]["x"][r0:r0 + M] if allm else self._buf("E", (M, d)))
        # round 5: a deferred step's attention reads the episode buffers in place (nv_attn_fwd_episode_bf16 with ONE table-step: the
        # prefix's K/V are rows [0, Mp) of the same buffer) instead of scatter -> strided forward over the K/V cache -> gather: one
        # launch per layer instead of three, no attention over the prefix rows above `qmin`, bit-identical (NAVILLM_EPISODE_ATTN_FWD=steps
        # restores the cache form)
        epi = allm and os.environ.get("NAVILLM_EPISODE_ATTN_FWD", "episode") != "steps"
        if epi:
            s_tab = ops.h2d(torch.from_numpy(np.concatenate([np.array([r0 + o for o in step["off"]], np.int32),
                                                             np.array(step["n"], np.int32)])), m.device)
            if ks not in self._lse_ptrs:
                self._lse_ptrs[ks] = ops.h2d(torch.from_numpy(np.array([t_.data_ptr() for t_ in self.lse_s[ks]], np.int64)), m.device)
            s_lse = self._lse_ptrs[ks]
        layers = []
        rows = slice(r0, r0 + M)               # this step's block of the episode buffers: kept for finish()
        for i in range(L):
            lw = st.layer(i)
            E = self._E[i] if defer else None
            dst = self._dst("s", i, rows, ("n1", "rstd1", "attn", "x1", "n2", "rstd2", "gu", "h", "x2"), E, allm)
            n1, rstd1 = ops.rmsnorm_fwd(x, lw.w1, eps, out=dst["n1"], rstd=dst["rstd1"])
            # q|k|v with RoPE in the GEMM epilogue (bit-identical to the GEMM followed by nv_rope_rows_bf16), row r at position pos[r]
            qkv = ops.qkv_rope(n1, lw.Wqkv, m.rope_cos, m.rope_sin, cap, H, hd, out=E["qkv"][rows] if allm else self._buf("qkv", (M, 3 * d)),
                               pos_i32=step["pos"])
            attn = dst["attn"]
            if epi:
                ops.attn_fwd_episode(E["qkv"][:r0 + M], E["attn"][:r0 + M], s_lse[i:i + 1], self.prefix["cu"], s_tab, 1, B, H, hd, cap, step["N"])
            else:
                ops.scatter_rows_bf16_(qkv, step["crow"], self.cache[i])
                lse_i = self.lse_s[ks][i] if allm else self.lse[i]
                ops.attn_fwd_strided(self.cache[i], self.kv0, B, Lmax, cap, H, hd, out=self.attn_buf[i], lse2=lse_i, q_row_min=qmin)
                ops.gather_rows_bf16(self.attn_buf[i], step["grow"], out=attn)
            x1, n2, rstd2, gu, h, x2 = layer.attn_out_mlp_fwd(lw, x, attn, eps, dst)
            if not allm:
                layers.append(dict(x=x, n1=n1, rstd1=rstd1, attn=attn, x1=x1, n2=n2, rstd2=rstd2, gu=gu, h=h))
            x = x2
        x_last = ops.gather_rows_bf16(x, step["last"])
        Hs, rstdf = ops.rmsnorm_fwd(x_last, st.p("lang_model.model.norm.weight"), eps)
        self.prefix["steps"] = k + 1
        saved = dict(step=step, layers=layers, x_last=x_last, rstdf=rstdf, serial=k + 1, r0=r0, defer=defer, batched=allm, k=ks, dH=None)
        if allm:
            self.prefix["recs"].append(saved)
        return Hs, saved

    def _step_backward(self, saved, dH):
        m, cfg, st = self.m, self.m.cfg, self.m.store
        if saved["serial"] != self.prefix["steps"]:
            raise RuntimeError("the step scratch of this episode was reused by a later step before this backward ran; call backward() "
                               "right after each loss (as the rollout loop does)")
        B, cap, H, hd, L, d = self.B, self.cap, cfg.num_heads, cfg.head_dim, cfg.num_layers, cfg.hidden_size
        step = saved["step"]
        M, Lmax, qmin = step["M"], step["Lmax"], step["qmin"]
        st.touch_layers()
        m._dp_begin_backward()
        dx_last = ops.rmsnorm_bwd(dH, saved["x_last"], st.p("lang_model.model.norm.weight"), saved["rstdf"], st.g("lang_model.model.norm.weight"))
        defer, r0 = saved["defer"], saved["r0"]
        first = self.prefix["kv_steps"] == 0           # the first backward of the episode SETS the prefix K/V-gradient accumulators
        rows = slice(r0, r0 + M)
        dx = self._E[L - 1]["dxo"][rows] if defer else self._buf("dx_a", (M, d))
        dx.zero_()
        ops.scatter_rows_bf16_(dx_last, step["last"], dx)
        other = self._buf("dx_b", (M, d))
        zeros_md = self._buf("zeros_md", (M, d))
        zeros_md.zero_()
        ff = cfg.intermediate_size
        wgrad = layer.wgrad_deferred if defer else layer.wgrad_now(ops.EPI_ACCUM)
        for i in reversed(range(L)):
            lw = st.layer(i)
            a = saved["layers"][i]
            E = self._E[i] if defer else None
            dst = {"dh": self._buf("dh", (M, ff)), "dgu": E["dgu"][rows] if defer else self._buf("dgu", (M, 2 * ff)), "dn2": self._buf("dn2", (M, d)),
                   "dx1": E["dx1"][rows] if defer else self._buf("dx1", (M, d)), "dattn": self._buf("dattn", (M, d))}
            dx1, dattn, _ = layer.attn_out_mlp_bwd(lw, dx, a["attn"], a["x1"], a["n2"], a["rstd2"], a["gu"], a["h"], dst, wgrad)
            # attention backward on the cache layout: dO is zero everywhere except this step's rows (written, used, zeroed again:
            # a full-buffer fill per layer was 3 % of the episode)
            ops.scatter_rows_bf16_(dattn, step["crow"], self.dout_full)
            # (round 3: the K/V gradients this step sends into the cached prefix rows go straight from the kernel's fp32 accumulators
            # into dkv_acc -- no bf16 round trip through dqkv_full and no second pass over 4 272 x 8192 values per layer)
            ops.attn_bwd_strided(self.cache[i], self.attn_buf[i], self.dout_full, self.lse[i], self.kv0, B, Lmax, cap, H, hd, self.dqkv_full,
                                 q_row_min=qmin, kv_acc=self.dkv_acc[i] if self.fuse_kvacc else None, prefix_len_i32=self.prefix["lens_dev"],
                                 first=first)
            ops.scatter_rows_bf16_(zeros_md, step["crow"], self.dout_full)
            dqkv = ops.gather_rows_bf16(self.dqkv_full, step["crow"], out=E["dqkv"][rows] if defer else None)
            ops.rope_rows_t_(dqkv, m.rope_cos, m.rope_sin, step["pos"], H, hd)
            if not self.fuse_kvacc:
                ops.kv_grad_accum(self.dqkv_full, self.dkv_acc[i], self.prefix["crow"], first=first)   # what this step sends into the prefix's K/V
            dst = {"dn1": self._buf("dn1", (M, d)), "dx": self._E[i - 1]["dxo"][rows] if defer and i > 0 else other}
            ndx = layer.qkv_in_bwd(lw, dqkv, a["x"], a["n1"], a["rstd1"], dx1, dst, wgrad)
            if defer:
                dx = ndx
            else:
                dx, other = ndx, dx
        self.prefix["kv_steps"] += 1
        dvis = ops.vis_grad(dx, step["vis_rows"]) if step["vis_rows"].numel() else None
        self._embed_grad(dx, step["ids_np"])
        return dvis

    def _embed_grad(self, dE, ids_np):
        st = self.m.store
        order = np.argsort(ids_np, kind="stable")
        uniq, counts = np.unique(ids_np, return_counts=True)
        seg = np.zeros(uniq.size + 1, dtype=np.int32)
        np.cumsum(counts, out=seg[1:])
        dev = dE.device
        ops.embed_grad(dE, ops.h2d(torch.from_numpy(uniq.astype(np.int32)), dev), ops.h2d(torch.from_numpy(seg), dev),
                       ops.h2d(torch.from_numpy(order.astype(np.int32)), dev), st.g("lang_model.model.embed_tokens.weight"))
        st.touch("lang_model.model.embed_tokens.weight")

    # ------------------------------------------------------------------ the prefix's one backward
    @torch.no_grad()
    def finish(self):
        """backward through the prefix with the K/V gradients the episode's steps accumulated, injected layer by layer; call it
        after the last step's backward() and before the optimizer step (inside `final_backward()` under data parallelism)"""
        P = self.prefix
        if P is None:
            return
        if P.get("window"):
            # accumulation window: the episode is complete, its work waits for the window's last episode (or for whoever needs `.grad`)
            P["finished"] = P["episodes"]
            if P["nb"] + self.Bs > self.B:
                self.flush_window()
            return
        m, cfg, st = self.m, self.m.cfg, self.m.store
        B, H, hd, L, d = self.B, cfg.num_heads, cfg.head_dim, cfg.num_layers, cfg.hidden_size
        Mp, Lmax = P["Mp"], P["Lmax"]
        if self.mode == "all" and P["defer"]:
            return self._finish_batched()
        if P["kv_steps"] == 0:                         # no step ran a backward: nothing to propagate (and dkv_acc holds no data)
            self.prefix = None
            self._cursor = 0
            self._poison_release()
            return
        defer = P["defer"]
        R = self._cursor if defer else Mp               # token rows of the whole episode: prefix [0, Mp) + every step's block
        st.touch_layers()
        dx = None
        ff = cfg.intermediate_size
        wgrad = layer.wgrad_deferred if defer else layer.wgrad_now(ops.EPI_ACCUM)
        for i in reversed(range(L)):
            lw = st.layer(i)
            a = P["layers"][i]
            E = self._E[i] if defer else None
            dqkv = E["dqkv"][:Mp] if defer else self._buf("p.dqkv", (Mp, 3 * d))
            dx1 = None
            if dx is not None:                    # (the top layer's prefix outputs feed nothing: only its K/V carry gradient)
                dst = {"dh": self._buf("p.dh", (Mp, ff)), "dgu": E["dgu"][:Mp] if defer else self._buf("p.dgu", (Mp, 2 * ff)),
                       "dn2": self._buf("p.dn2", (Mp, d)), "dx1": E["dx1"][:Mp] if defer else self._buf("p.dx1", (Mp, d)),
                       "dattn": self._buf("p.dattn", (Mp, d))}
                dx1, dattn, _ = layer.attn_out_mlp_bwd(lw, dx, a["attn"], a["x1"], a["n2"], a["rstd2"], a["gu"], a["h"], dst, wgrad)
                ops.attn_bwd_varlen(a["qkv"], a["attn"], dattn, a["lse"], P["cu"], P["pos0"], B, Lmax, H, hd, dqkv, q_row_min=0, rope=None)
            else:
                dqkv.zero_()
            ops.kv_grad_inject(dqkv, self.dkv_acc[i], P["crow"])
            ops.rope_rows_t_(dqkv, m.rope_cos, m.rope_sin, P["pos"], H, hd)

            wgrad_qkv = wgrad
            if defer:
                def wgrad_qkv(*_, lw=lw, E=E, lo=0 if dx is not None else Mp):
                    """the episode's weight gradients of this layer: ONE GEMM per weight over every token row (prefix + all steps), fp32
                    accumulation over the whole contraction.  The top layer's prefix rows carry no gradient outside q|k|v."""
                    if R > lo:
                        ops.gemm_bf16(ops.TN, E["dxo"][lo:R], E["h"][lo:R], out=lw.gd, epilogue=ops.EPI_ACCUM)
                        ops.gemm_bf16(ops.TN, E["dgu"][lo:R], E["n2"][lo:R], out=lw.ggu, epilogue=ops.EPI_ACCUM)
                        ops.gemm_bf16(ops.TN, E["dx1"][lo:R], E["attn"][lo:R], out=lw.go, epilogue=ops.EPI_ACCUM)
                    ops.gemm_bf16(ops.TN, E["dqkv"][:R], E["n1"][:R], out=lw.gqkv, epilogue=ops.EPI_ACCUM)
                dx_out = self._E[i - 1]["dxo"][:Mp] if i > 0 else self._buf("p.dx0", (Mp, d))
            else:
                dx_out = self._buf(f"p.dx{i & 1}", (Mp, d))
            dx = layer.qkv_in_bwd(lw, dqkv, a["x"], a["n1"], a["rstd1"], dx1, {"dn1": self._buf("p.dn1", (Mp, d)), "dx": dx_out}, wgrad_qkv)
            m._dp_layer_done(i, [])
        if defer:
            self._last_rows = R - Mp
            self._cursor = 0
        self._embed_grad(dx, P["ids_np"])
        self.prefix = None
        self._poison_release()
        dp = getattr(m, "_dp", None)
        if dp is not None and dp._exchanging():
            dp._finalize()                         # outside autograd: no engine callback will run the end-of-backward exchange

    def register_loss(self, rec, targets, scale):
        """DeferredLoss.backward(): CE_sum(logits of step `rec`, targets) * scale is part of the episode's objective"""
        if rec.get("targets") is not None:
            raise RuntimeError("a deferred (teacher-forced) navigation step takes ONE loss; its backward() ran twice")
        rec["targets"] = ops.h2d(torch.as_tensor(targets).to(torch.int64).contiguous(), self.m.device)
        rec["scale"] = float(scale)

    def _step_table(self, recs, Bk, Mp):
        """what the one-launch episode attention kernels read: tab = off[T, Bk] | n[T, Bk] (first row / number of rows of table-step k's
        block of prefix slot b; 0 rows where that sample has no such step -- the shorter episodes of an accumulation window) and, per
        layer, the T lse-slab pointers.  One episode: table-step k is the k-th recorded step; a window: the k-th step of every episode."""
        L, Bs = self.m.cfg.num_layers, self.Bs
        T = max(r["k"] for r in recs) + 1
        off = np.full((T, Bk), Mp, np.int32)
        n = np.zeros((T, Bk), np.int32)
        for r in recs:
            sb = r["step"].get("sb", 0)
            off[r["k"], sb:sb + Bs] = [r["r0"] + o for o in r["step"]["off"]]
            n[r["k"], sb:sb + Bs] = r["step"]["n"]
        while len(self.lse_s) < T:
            self.lse_s.append([torch.zeros((self.B, self.m.cfg.num_heads, self.cap), dtype=F32, device=self.m.device) for _ in range(L)])
        ptrs = np.array([[self.lse_s[k][i].data_ptr() for k in range(T)] for i in range(L)], dtype=np.int64)
        dev = self.m.device
        return T, ops.h2d(torch.from_numpy(np.concatenate([off.reshape(-1), n.reshape(-1)])), dev), ops.h2d(torch.from_numpy(ptrs), dev)

    def _forward_lazy(self, recs):
        """teacher-forced episode (round 4): the LM forward of ALL recorded steps as ONE batch over their rows [Mp, R) of the episode
        buffers -- the qkv / o / gate|up / down GEMMs and every row kernel see M = sum of the steps' suffix rows (~4 200 at the bench
        shape) instead of six launches of ~700 rows (the few-hundred-row forward GEMMs ran at 0.37 of the MFMA peak, the large ones at
        0.49), the attention stays one launch per step (each step's queries see the cached prefix + its own rows).  Legal because under
        imitation learning the next step's inputs never depend on the LM: the action is the teacher's (mp3d_agent.py:760-761) and the
        history token is the FUSION output `fuse_embeds[b, a_t]` (mp3d_agent.py:774-778).  Then the action head and the CE of every
        step with a registered loss; their gradient w.r.t. the steps' last rows becomes `dH`, exactly what a step's backward() records
        in the non-lazy form -- the batched backward that follows is unchanged."""
        from . import functions as Fn
        P = self.prefix
        m, cfg, st = self.m, self.m.cfg, self.m.store
        B, cap, H, hd, eps, L, d, ff = self.Bs, self.cap, cfg.num_heads, cfg.head_dim, cfg.rms_norm_eps, cfg.num_layers, cfg.hidden_size, \
            cfg.intermediate_size
        Bk = P.get("nb", self.B)                         # prefix slots in use (an accumulation window: all its episodes' samples)
        Mp, R = P["Mp"], self._cursor
        # round 5: a prefix that has not gone through the decoder yet (begin() of a teacher-forced episode only builds its tables) joins
        # the batch: rows [0, R) instead of [Mp, R).  round 6: `recs` is the TAIL of the recorded steps that has not gone through the
        # decoder yet -- everything in finish(), or (automatic episodes: LazyLogits) the steps since the last time a step's logits were
        # read; rows [r_lo, R) with r_lo = the first of them
        pend = bool(P.get("pending"))
        r_lo = 0 if pend else recs[0]["r0"]
        rows = slice(r_lo, R)
        assert (recs[0]["r0"] == Mp or not pend) and recs[-1]["r0"] + recs[-1]["step"]["M"] == R and \
            all(a["r0"] + a["step"]["M"] == b_["r0"] for a, b_ in zip(recs, recs[1:])), "the pending steps must be the tail of the episode's rows"
        with torch.no_grad():
            vis_parts, vix_parts, off = [], [], 0
            for r in recs:
                sp = r["step"]
                v = sp.get("vis_live")
                nv = 0 if v is None else int(v.shape[0])
                vix_parts.append(torch.where(sp["vix"] >= 0, sp["vix"] + off, sp["vix"]) if off else sp["vix"])
                if nv:
                    vis_parts.append(v.detach())
                off += nv
            ids_cat = torch.cat(([P["ids_dev"]] if pend else []) + [r["step"]["ids"] for r in recs])
            pos_cat = torch.cat(([P["pos"]] if pend else []) + [r["step"]["pos"] for r in recs])
            vix_cat = torch.cat(([P["vix_dev"]] if pend else []) + vix_parts)
            vis_cat = torch.cat(vis_parts, 0).contiguous() if vis_parts else None
            while len(self.lse_s) < max(r["k"] for r in recs) + 1 and not P.get("window"):
                self.lse_s.append([torch.zeros((self.B, H, cap), dtype=F32, device=m.device) for _ in range(L)])
            last_cat = torch.cat([r["step"]["last"] + (r["r0"] - Mp) for r in recs])      # each step's last rows, relative to row Mp
            last_x = last_cat + (Mp - r_lo)                                                # ... relative to the first row of this batch
            prune_top = os.environ.get("NAVILLM_EPISODE_PRUNE_TOP", "1") != "0" and L > 1
            top_now = None
            # round 5: the attention of ALL steps in one launch per layer, reading the episode buffers in place (nv_attn_fwd_episode_bf16;
            # NAVILLM_EPISODE_ATTN_FWD=steps: round 4's scatter -> strided forward -> gather per step, bit-identical)
            # (the kernel's grid is (slots * heads, table-steps * query blocks): beyond 65 535 in y the per-step cache form runs -- ADVICE r5)
            f_nmax = max(r["step"]["N"] for r in recs)
            f_fits = (max(r["k"] for r in recs) + 1) * ((f_nmax + 127) // 128) <= 65535
            epi_fwd = (os.environ.get("NAVILLM_EPISODE_ATTN_FWD", "episode") != "steps" and f_fits) or bool(P.get("window"))
            if epi_fwd:
                T, f_tab, f_lse = self._step_table(recs, Bk, Mp)
            elif pend:
                self._kv_layout()                      # (the layer loop below scatters the prefix rows as it computes them)
            else:
                self._fill_prefix_cache(P)             # the prefix went through the decoder earlier: its K/V rows into the cache layout
            x = ops.embed_vis(st.p("lang_model.model.embed_tokens.weight"), ids_cat, vix_cat, vis_cat, out=self._E[0]["x"][rows])
            for i in range(L):
                lw = st.layer(i)
                E, E32 = self._E[i], self._E32[i]
                n1, _ = ops.rmsnorm_fwd(x, lw.w1, eps, out=E["n1"][rows], rstd=E32["r1"][rows])
                ops.qkv_rope(n1, lw.Wqkv, m.rope_cos, m.rope_sin, cap, H, hd, out=E["qkv"][rows], pos_i32=pos_cat)
                if pend:
                    # the prefix rows' own causal attention (the top layer's is never read: only its K/V are, by the steps' queries)
                    if i < L - 1 or not prune_top:
                        ops.attn_fwd_varlen(E["qkv"][:Mp], P["cu"], P["pos0"], Bk, P["Lmax"], H, hd, out=E["attn"][:Mp], lse2=P["layers"][i]["lse"])
                    if not epi_fwd:
                        ops.scatter_rows_bf16_(E["qkv"][:Mp], P["crow"], self.cache[i])
                if epi_fwd:
                    ops.attn_fwd_episode(E["qkv"][:R], E["attn"][:R], f_lse[i], P["cu"], f_tab, T, Bk, H, hd, cap, f_nmax)
                for r in (() if epi_fwd else recs):  # round 4 form: per step over the K/V cache (prefix rows + this step's rows)
                    sp = r["step"]
                    sl = slice(r["r0"], r["r0"] + sp["M"])
                    ops.scatter_rows_bf16_(E["qkv"][sl], sp["crow"], self.cache[i])
                    ops.attn_fwd_strided(self.cache[i], self.kv0, self.B, sp["Lmax"], cap, H, hd, out=self.attn_buf[i], lse2=self.lse_s[r["k"]][i],
                                         q_row_min=sp["qmin"])
                    ops.gather_rows_bf16(self.attn_buf[i], sp["grow"], out=E["attn"][sl])
                if i == L - 1 and prune_top:
                    # the top layer feeds only each sample's LAST row of every step (nav_model.py:237) -- after its K/V projection and
                    # attention, o_proj / MLP run on those T*B rows instead of on every suffix row (what LlamaStack's pruned last layer
                    # does on the recompute path); the batched backward mirrors it (`top`)
                    x_l = ops.gather_rows_bf16(x, last_x)
                    attn_l = ops.gather_rows_bf16(E["attn"][rows], last_x)
                    x1_l, n2_l, r2_l, gu_l, h_l, x_last = layer.attn_out_mlp_fwd(lw, x_l, attn_l, eps)
                    top_now = dict(idx=last_cat, attn=attn_l, x1=x1_l, n2=n2_l, r2=r2_l, gu=gu_l, h=h_l)
                    P.setdefault("tops", []).append(top_now)
                    break
                dst = {"x1": E["x1"][rows], "n2": E["n2"][rows], "rstd2": E32["r2"][rows], "gu": E["gu"][rows], "h": E["h"][rows],
                       "x2": self._E[i + 1]["x"][rows] if i + 1 < L else self._buf("lz.x2", (max(R, self._ecap), d))[:R - r_lo]}
                x = layer.attn_out_mlp_fwd(lw, x, E["attn"][rows], eps, dst)[5]
            if top_now is None:
                x_last = ops.gather_rows_bf16(x, last_x)
            if pend:
                P["pending"] = False
                P["cache_valid"] = not epi_fwd
            Hs_all, rstdf = ops.rmsnorm_fwd(x_last, st.p("lang_model.model.norm.weight"), eps)
            for t, r in enumerate(recs):
                r["x_last"], r["rstdf"], r["Hs"] = x_last[t * B:(t + 1) * B], rstdf[t * B:(t + 1) * B], Hs_all[t * B:(t + 1) * B]

    def _heads_deferred(self, recs):
        """action head + CE of every recorded step that is through the decoder (`r["Hs"]`) and has no logits / no loss gradient yet (tiny:
        B rows each), through the same autograd functions the non-lazy path uses; their gradient w.r.t. the steps' last rows becomes
        `dH`, exactly what a step's backward() records in the non-lazy form.  A step whose logits were READ (`force_logits(live=True)`)
        carries its own autograd graph and gets its `dH` from the rollout's backward() instead."""
        from . import functions as Fn
        m, B = self.m, self.Bs
        todo = [r for r in recs if r.get("lazy") and r.get("Hs") is not None and r.get("logits_live") is None and
                (r.get("logits") is None or (r.get("targets") is not None and r["dH"] is None))]
        if not todo:
            return
        Hs_leaf = torch.cat([r["Hs"] for r in todo], 0).detach().requires_grad_(True)
        total = None
        with torch.enable_grad():
            for t, r in enumerate(todo):
                col, mask_not = r["head"]
                pred = Fn.HeadBF16.apply(Hs_leaf[t * B:(t + 1) * B], m, "out_head.0")
                logits = torch.gather(pred, 1, col).masked_fill(mask_not, float("-inf"))
                r["logits"] = logits.detach()
                if r.get("targets") is not None and r["dH"] is None:
                    ls = Fn.ActionCE.apply(logits, r["targets"])
                    r["loss_sum"] = ls.detach()
                    total = ls * r["scale"] if total is None else total + ls * r["scale"]
            if total is not None:
                total.backward()
        if Hs_leaf.grad is not None:
            g = Hs_leaf.grad
            for t, r in enumerate(todo):
                if r.get("targets") is not None and r["dH"] is None:
                    r["dH"] = g[t * B:(t + 1) * B].contiguous()

    def _forward_pending(self):
        """every recorded step that has not gone through the decoder yet does so now, as one batch (with the prefix, if that is still
        pending); -> the recorded steps"""
        P = self.prefix
        if P is None:
            raise RuntimeError("the episode of this step is over (finish_episode() ran, or it was aborted): its deferred values are gone")
        if P.get("window"):
            raise RuntimeError("inside an accumulation window (begin_episode(..., accumulate=n)) the logits / loss values exist after the "
                               "window's last finish_episode() or model.flush_accumulation_window()")
        recs = P["recs"]
        pending = [r for r in recs if r.get("lazy") and r["x_last"] is None]
        if pending:
            self._forward_lazy(pending)
        return recs

    def force_logits(self, rec, live=True):
        """automatic episodes (losses.LazyLogits): the rollout READS the logits of step `rec` -- a sampled / argmax step, or a caller that
        looks at them.  All pending steps run their LM forward now; live: -> the step's logits as a tensor connected to autograd (head ->
        gather -> mask on a leaf whose gradient hook records the step's `dH`), so whatever loss the rollout builds on it and
        backpropagates reaches the deferred backward; not live: only the value (`rec["logits"]`)."""
        from . import functions as Fn
        if rec.get("logits_live") is not None:
            return rec["logits_live"]
        if not live and rec.get("logits") is not None:
            return rec["logits"]
        if not any(r is rec for r in (self.prefix or {}).get("recs", ())):
            if rec.get("logits") is not None:
                return rec["logits"]                      # (the episode is over: the value it left behind; no graph any more)
            raise RuntimeError("the episode of this step is over and its logits were never computed")
        self._forward_pending()
        if not live or rec.get("targets") is not None:
            # only the values -- also when the step's deferred loss has ALREADY run backward(): the reference's order in a sampled rollout is
            # loss + backward() (mp3d_agent.py:750-757), THEN `Categorical(nav_probs.float())` (:762-765); the loss stays deferred (the
            # heads pass below computes it and the step's dH now), the reader gets the numbers without a graph
            self._heads_deferred([rec])
            if live:
                self.stats["forced_reads"] = self.stats.get("forced_reads", 0) + 1
            return rec["logits"]
        self.stats["forced_reads"] = self.stats.get("forced_reads", 0) + 1
        leaf = rec["Hs"].detach().clone().requires_grad_(True)

        def hook(g, rec=rec):
            rec["dH"] = g.contiguous().clone() if rec["dH"] is None else rec["dH"] + g
        leaf.register_hook(hook)
        with torch.enable_grad():
            col, mask_not = rec["head"]
            pred = Fn.HeadBF16.apply(leaf, self.m, "out_head.0")
            rec["logits_live"] = torch.gather(pred, 1, col).masked_fill(mask_not, float("-inf"))
        rec["logits"] = rec["logits_live"].detach()
        return rec["logits_live"]

    def force_values(self):
        """automatic episodes: the rollout reads a deferred LOSS value (`loss.item()`, train.py:83): the pending steps' batched forward +
        the heads and losses of every step -- not the backward"""
        self._heads_deferred(self._forward_pending())

    def flush_segment(self):
        """long episodes (round 4; VERDICT r3 next #7a): run the deferred backward of the steps recorded SO FAR -- their rows [Mp, R) only:
        weight gradients into `.grad`, the K/V gradients they send into the prefix rows into the fp32 accumulators (first segment:
        stored, later ones: added), each step's visual-token gradient into its encoder graph -- and hand their rows back.  The prefix
        stays open (its own backward runs once, in finish()); the steps of different segments never see one another (a step attends to
        the prefix and to its own rows), so the result is the same sum.  Called automatically when the next step's rows would not fit
        (`_segment_full`); every recorded step must have run its backward()."""
        P = self.prefix
        if P is None or self.mode != "all" or not P["defer"] or not P["recs"]:
            return
        if any(r["dH"] is None and not (r.get("lazy") and r.get("targets") is not None) for r in P["recs"]):
            raise RuntimeError("prefix-reuse training: the episode's rows must be flushed (they no longer fit / NAVILLM_EPISODE_MAX_ROWS), but a "
                               "recorded step has not run backward() yet; call backward() right after each loss (as the rollout loop does), "
                               "or use NAVILLM_EPISODE_DEFER=none")
        self._finish_batched(final=False)

    def _finish_batched(self, final=True):
        """mode "all": ONE walk down the layers for every token row of the episode (prefix rows [0, Mp), then each step's block).
        final=False (flush_segment): the steps' rows [Mp, R) only, the prefix stays open."""
        P = self.prefix
        m, cfg, st = self.m, self.m.cfg, self.m.store
        B, cap, H, hd, L, d, ff = self.Bs, self.cap, cfg.num_heads, cfg.head_dim, cfg.num_layers, cfg.hidden_size, cfg.intermediate_size
        Bk = P.get("nb", self.B)                         # prefix slots in use (an accumulation window: all its episodes' samples)
        Mp, R = P["Mp"], self._cursor
        recs = P["recs"]
        pending = [r for r in recs if r.get("lazy") and r["x_last"] is None]
        if pending:
            self._forward_lazy(pending)                 # teacher-forced episode: the steps' forward, all at once (those still pending)
        self._heads_deferred(recs)                      # ... then heads + losses of every step that has none yet
        live = [r for r in recs if r["dH"] is not None]
        seg_before = P["segments"]                      # segments already flushed: dkv_acc holds their sums
        if final:
            self._last_rows = self._seg_total + (R - Mp)          # the whole episode's suffix rows: what the next episode is sized for
        else:
            self._seg_total += R - Mp
        if final:
            self.prefix = None
            self._cursor = 0
        else:
            P["recs"] = []
            P["segments"] = seg_before + 1
            self._cursor = Mp
            self.stats["segments_flushed"] += 1
        if not live and not (final and seg_before):
            if final:
                self._poison_release()
            return
        with torch.no_grad():
            # round 5: nothing has written a decoder-layer gradient since zero_grad() (FlatStore.layers_zero) -> the weight-gradient GEMMs of this walk
            # are the first writers of their buffers and STORE: `0 + bf16(dW)` without reading 13.5 GB of zeros (each of the four
            # matrices of a layer is written exactly once per walk).  Later segments of a long episode / a second accumulation read-add.
            wacc = ops.EPI_STORE if (getattr(st, "layers_zero", False) and seg_before == 0
                                     and os.environ.get("NAVILLM_WGRAD_STORE", "1") != "0") else ops.EPI_ACCUM
            if wacc == ops.EPI_STORE and debug.POISON:
                st.assert_layers_zero("finish_episode()")
            st.touch_layers()
            dp0 = getattr(m, "_dp", None)
            if dp0 is not None and final:
                dp0.on_deferred_backward_begin()
            normw, gnormw = st.p("lang_model.model.norm.weight"), st.g("lang_model.model.norm.weight")
            # (scratch sized for the buffers' capacity, not for this walk's R: the segments of a long episode grow from one to the
            # next, and every new maximum would free and re-allocate all eight slabs -- 0.2 s per flush at 7B)
            Rc = max(R, self._ecap)
            dx, other = self._buf("b.dx_a", (Rc, d))[:R], self._buf("b.dx_b", (Rc, d))[:R]
            dx1, dattn, dn = self._buf("b.dx1", (Rc, d))[:R], self._buf("b.dattn", (Rc, d))[:R], self._buf("b.dn", (Rc, d))[:R]
            dqkv, dgu, dh = self._buf("b.dqkv", (Rc, 3 * d))[:R], self._buf("b.dgu", (Rc, 2 * ff))[:R], self._buf("b.dh", (Rc, ff))[:R]
            # gradient of the stack's output: the final norm's backward on each step's B last-token rows; zero everywhere else (the
            # top layer's prefix rows feed nothing, a step without a backward contributes nothing)
            tops = P.pop("tops", None)                 # teacher-forced forward with the pruned top layer: its tail ran on T*B rows
            top = None
            if tops:
                # (one entry per forward batch, in step order: one in a teacher-forced episode, several when an automatic episode's
                # logits were read on the way)
                top = tops[0] if len(tops) == 1 else {k: torch.cat([t_[k] for t_ in tops], 0) for k in tops[0]}
                assert top["idx"].numel() == len(recs) * B, "every recorded step went through the batched forward exactly once"
            if top is not None:
                dxl = torch.zeros((len(recs) * B, d), dtype=BF16, device=m.device)
                for t, r in enumerate(recs):
                    if r["dH"] is not None:
                        dxl[t * B:(t + 1) * B] = ops.rmsnorm_bwd(r["dH"], r["x_last"], normw, r["rstdf"], gnormw)
            else:
                dx.zero_()
                for r in live:
                    dx_last = ops.rmsnorm_bwd(r["dH"], r["x_last"], normw, r["rstdf"], gnormw)
                    ops.scatter_rows_bf16_(dx_last, r["step"]["last"], dx[r["r0"]:r["r0"] + r["step"]["M"]])
            Mz = max([r["step"]["M"] for r in recs] or [1])
            zeros_md = self._buf("zeros_md", (Mz, d))
            zeros_md.zero_()
            Lp_max = P["Lmax"]
            self._lens_dev = P["lens_dev"]
            epi_tab = lse_tab = None
            # (the one-launch kernels keep a step table of 128 entries and 1536 statistics rows in LDS: longer episodes / blocks take
            # the per-step path)
            Nz = max([r["step"]["N"] for r in recs] or [0])
            T_tab = 0
            if recs and ((os.environ.get("NAVILLM_EPISODE_ATTN_BWD", "episode") != "steps" and max(r["k"] for r in recs) < 128 and Nz <= 1536)
                         or P.get("window")):
                # where every step's block sits (r0 | rows per sample | live rows of each sample) and, per layer, where its lse is
                T_tab, epi_tab, lse_tab = self._step_table(recs, Bk, Mp)
                assert recs[0]["r0"] == Mp and all(a["r0"] + a["step"]["M"] == b_["r0"] for a, b_ in zip(recs, recs[1:])) and \
                    recs[-1]["r0"] + recs[-1]["step"]["M"] == R, "the steps' blocks must tile rows [Mp, R) of the episode buffers"
            if epi_tab is None and recs:
                self._fill_prefix_cache(P)                   # the per-step backward form reads the prefix's K/V from the K/V-cache layout
            wgrad = layer.wgrad_now(wacc)
            for i in reversed(range(L)):
                lw = st.layer(i)
                E, E32 = self._E[i], self._E32[i]
                # the top layer's prefix rows feed nothing (only their K/V carry gradient): its MLP / o_proj backward covers the steps' rows
                # only; a segment flush (final=False) never touches the prefix rows
                lo = Mp if (i == L - 1 or not final) else 0
                if i == L - 1 and top is not None:
                    # the pruned tail's backward on the T*B last rows; what flows on into the attention output / the residual stream is
                    # zero everywhere else
                    dx1_l, dattn_l, _ = layer.attn_out_mlp_bwd(lw, dxl, top["attn"], top["x1"], top["n2"], top["r2"], top["gu"], top["h"], wgrad=wgrad)
                    dattn[Mp:].zero_()
                    dx1[Mp:].zero_()
                    ops.scatter_rows_bf16_(dattn_l, top["idx"], dattn[Mp:])
                    ops.scatter_rows_bf16_(dx1_l, top["idx"], dx1[Mp:])
                elif R > lo:
                    dst = {"dh": dh[lo:], "dgu": dgu[lo:], "dn2": dn[lo:], "dx1": dx1[lo:], "dattn": dattn[lo:]}
                    layer.attn_out_mlp_bwd(lw, dx[lo:], E["attn"][lo:R], E["x1"][lo:R], E["n2"][lo:R], E32["r2"][lo:R], E["gu"][lo:R], E["h"][lo:R],
                                           dst, wgrad)
                # attention backward.  The prefix rows' own causal attention (packed rows) ...
                if final:
                    if lo == 0:
                        ops.attn_bwd_varlen(E["qkv"][:Mp], E["attn"][:Mp], dattn[:Mp], P["layers"][i]["lse"], P["cu"], P["pos0"], Bk, Lp_max, H, hd,
                                            dqkv[:Mp], q_row_min=0, rope=None)
                    else:
                        dqkv[:Mp].zero_()
                        dx1[:Mp].zero_()
                # ... and every step's rows over their sample's prefix and the step's own earlier rows
                if epi_tab is not None:
                    # ONE launch per kernel for all the steps, reading the episode buffers in place: the prefix key blocks walk every
                    # step's queries and STORE the fp32 sum in dkv_acc (a later segment of a long episode: ADD to it); dQ and the steps'
                    # own dK|dV land in dqkv through RoPE^T
                    ops.attn_bwd_episode(E["qkv"][:R], E["attn"][:R], dattn, dqkv, lse_tab[i], P["cu"], epi_tab, self.dkv_acc[i], T_tab, Bk, H, hd,
                                         cap, Mp, Lp_max, Nz, rope=(m.rope_cos, m.rope_sin), accumulate=seg_before > 0)
                elif recs:
                    self._attn_bwd_by_step(i, recs, E, dattn, dqkv, zeros_md, first=seg_before == 0)
                q0 = 0
                if final:
                    ops.kv_grad_inject(dqkv[:Mp], self.dkv_acc[i], P["crow"])
                    ops.rope_rows_t_(dqkv[:Mp], m.rope_cos, m.rope_sin, P["pos"], H, hd)
                else:
                    q0 = Mp
                if R > q0:
                    layer.qkv_in_bwd(lw, dqkv[q0:], E["x"][q0:R], E["n1"][q0:R], E32["r1"][q0:R], dx1[q0:], {"dn1": dn[q0:], "dx": other[q0:]}, wgrad)
                dx, other = other, dx
                if final:
                    m._dp_layer_done(i, [])
            if final:
                self._embed_grad(dx[:Mp], P["ids_np"])
            dvis = []
            for r in recs:
                sp = r["step"]
                blk = dx[r["r0"]:r["r0"] + sp["M"]]
                dvis.append(ops.vis_grad(blk, sp["vis_rows"]) if sp["vis_rows"].numel() else None)
                self._embed_grad(blk, sp["ids_np"])
        # each step's visual-token gradient into that step's scene-encoder / fusion graph (kept alive since the step's forward)
        for r, g in zip(recs, dvis):
            v = r["step"].get("vis_live")
            if g is not None and v is not None and v.requires_grad:
                with torch.enable_grad():
                    torch.autograd.backward([v], [g])
            r["step"]["vis_live"] = None
        if final:
            self._poison_release()
        dp = getattr(m, "_dp", None)
        if final and dp is not None and dp._exchanging():
            dp._finalize()                         # outside autograd: no engine callback will run the end-of-backward exchange

    def _attn_bwd_by_step(self, i, recs, E, dattn, dqkv, zeros_md, first=True):
        """round 3a form (NAVILLM_EPISODE_ATTN_BWD=steps): one strided backward per step over the K/V cache: the step's post-RoPE q|k|v
        and its attention outputs go back to their cache rows, dO to the step's rows (zero elsewhere); the gradients the step sends
        into the cached prefix rows are summed in fp32 by the kernel itself (first step: stored)"""
        m, cfg = self.m, self.m.cfg
        B, cap, H, hd = self.B, self.cap, cfg.num_heads, cfg.head_dim
        self._kv_layout()
        for n_, r in enumerate(recs):
            sp = r["step"]
            rows = slice(r["r0"], r["r0"] + sp["M"])
            ops.scatter_rows_bf16_(E["qkv"][rows], sp["crow"], self.cache[i])
            ops.scatter_rows_bf16_(E["attn"][rows], sp["crow"], self.attn_buf[i])
            ops.scatter_rows_bf16_(dattn[rows], sp["crow"], self.dout_full)
            ops.attn_bwd_strided(self.cache[i], self.attn_buf[i], self.dout_full, self.lse_s[r["k"]][i], self.kv0, B, sp["Lmax"], cap,
                                 H, hd, self.dqkv_full, q_row_min=sp["qmin"], kv_acc=self.dkv_acc[i],
                                 prefix_len_i32=self._lens_dev, first=(first and n_ == 0))
            ops.scatter_rows_bf16_(zeros_md[:sp["M"]], sp["crow"], self.dout_full)
            ops.gather_rows_bf16(self.dqkv_full, sp["crow"], out=dqkv[rows])
            ops.rope_rows_t_(dqkv[rows], m.rope_cos, m.rope_sin, sp["pos"], H, hd)
