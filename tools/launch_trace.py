"""Same launches, same bits: record every C-ABI call the decoder formulations make, and hash what they compute.

`navillm_amd.lib._lib` is replaced, after load(), by a proxy that logs each call's symbol and its non-pointer arguments (pointers --
the stream included -- only as null / non-null) before forwarding it; the package itself has no tracing path.  Each scenario runs the
`_episode` helper of tests/test_episode_gpu.py once on the d = 512, 3-layer model (B = 3 ragged prompts, 4 steps) under one set of
formulation knobs, and leaves: the number of calls, the calls per symbol, a SHA-256 over the whole call sequence, and a SHA-256 of
every step's logits and of every gradient group buffer after the episode.

usage: python tools/launch_trace.py run OUT.json [--repo TREE] [--full DIR]
           TREE: import navillm_amd from this tree (an export of another commit, with its built library) instead of this one;
           DIR: also write each scenario's complete call sequence there, one call per line (megabytes: not for the repository)
       python tools/launch_trace.py compare BASE_A.json BASE_B.json HEAD.json
           BASE_A / BASE_B: two runs of the base commit.  A scenario whose digests differ between them is "not bit-reproducible at
           the base" and is compared by trace only.  Exit status 1 unless every scenario's trace equals the base's and every
           reproducible scenario's digests do.
"""
import ctypes
import gc
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> (environment, how the episode runs).  use_prefix=False is the per-step recompute through LlamaStack (navigation prunes the last
# layer to the <cls_1> rows); "lm_loss" adds a summarization step, whose backward walks every layer at full size.
SCENARIOS = {
    "a_recompute_packed": (dict(), dict(use_prefix=False)),
    "a_recompute_padded": (dict(NAVILLM_PACK_ROWS="0"), dict(use_prefix=False)),
    "b_lm_loss_full_layers": (dict(), dict(use_prefix=False, lm_loss=True)),
    "c_defer_all": (dict(NAVILLM_EPISODE_DEFER="all"), dict()),
    "c_defer_wgrad": (dict(NAVILLM_EPISODE_DEFER="wgrad"), dict()),
    "c_defer_none": (dict(NAVILLM_EPISODE_DEFER="none"), dict()),
    "d_all_attn_fwd_steps": (dict(NAVILLM_EPISODE_DEFER="all", NAVILLM_EPISODE_ATTN_FWD="steps"), dict()),
    "d_all_attn_bwd_steps": (dict(NAVILLM_EPISODE_DEFER="all", NAVILLM_EPISODE_ATTN_BWD="steps"), dict()),
    "e_all_teacher_forced": (dict(NAVILLM_EPISODE_DEFER="all"), dict(teacher_forced=True)),
    "f_all_segment_flush": (dict(NAVILLM_EPISODE_DEFER="all"), dict(flush=True)),
    "g_overlap_wgrad_1": (dict(NAVILLM_OVERLAP_WGRAD="1"), dict(use_prefix=False, lm_loss=True)),
    "g_overlap_wgrad_2": (dict(NAVILLM_OVERLAP_WGRAD="2"), dict(use_prefix=False, lm_loss=True)),
    "h_fuse_swiglu_bwd": (dict(NAVILLM_FUSE_SWIGLU_BWD="1"), dict(use_prefix=False, lm_loss=True)),
    "i_head_dim_64": (dict(NAVILLM_EPISODE_DEFER="all"), dict(heads=8)),
}
KNOBS = sorted({k for env, _ in SCENARIOS.values() for k in env} | {"NAVILLM_EPISODE_MAX_ROWS"})


class Recorder:
    """stands in for the loaded library: every attribute is the real ctypes function behind a logging wrapper"""

    def __init__(self, real):
        self._real, self._wrapped, self.calls = real, {}, []

    def __getattr__(self, name):
        fn = self._wrapped.get(name)
        if fn is None:
            real = getattr(self._real, name)
            is_ptr = [t is ctypes.c_void_p or hasattr(t, "contents") for t in (real.argtypes or ())]
            calls = self.calls

            def fn(*args, _real=real, _name=name, _is_ptr=is_ptr):
                calls.append(_name + "(" + ",".join(("0" if not a else "p") if p else repr(a) for a, p in zip(args, _is_ptr)) + ")")
                return _real(*args)
            self._wrapped[name] = fn
        return fn


def _sha(t):
    import torch
    t = t.detach().contiguous()
    if t.dtype == torch.bfloat16:
        t = t.view(torch.int16)
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def run_scenario(rec, env, use_prefix=True, teacher_forced=False, lm_loss=False, flush=False, heads=4, steps=4, B=3, instr_len=180):
    import torch
    from navillm_amd import config as nvcfg, functions as Fn
    from navillm_amd.losses import CrossEntropyLoss
    from navillm_amd.nav_model import NavModel
    from navillm_amd.synthetic import SyntheticEpisodes, lm_aux_step, nav_step
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(env)
    Fn.FUSE_SWIGLU_BWD = env.get("NAVILLM_FUSE_SWIGLU_BWD") == "1"          # (read once, when the module is imported)
    dev = torch.device("cuda:0")
    cfg = nvcfg.NavConfig(hidden_size=512, num_layers=3, num_heads=heads, intermediate_size=1408, base_vocab_size=1000, enc_hidden_size=256,
                          enc_num_heads=4, enc_intermediate_size=512, image_feat_size=768)
    model = NavModel(nav_config=cfg, device=dev, seed=12)
    model.eval()                                                              # dropout off

    def episode():
        ep = SyntheticEpisodes(cfg, B, seed=31, instr_len=instr_len, device=dev)
        for b in range(B):
            ep.instr[b] = ep.instr[b][: instr_len - 23 * b]                   # ragged prompts: prefixes of different lengths
        crit = CrossEntropyLoss()
        model.zero_grad()
        if use_prefix:
            model.begin_episode(ep.prefix_ids(), teacher_forced=teacher_forced)
        outs = []
        for t in range(steps):
            torch.manual_seed(500 + t)
            outs.append(nav_step(model, crit, ep, train=True, last=(t == steps - 1))[1])
        if lm_loss:
            outs.append(lm_aux_step(model, ep, "summarization")[0])
        stats = None
        if use_prefix:
            stats = dict(model.episode.stats)
            model.finish_episode()
        torch.cuda.synchronize()
        return [(o.value if hasattr(o, "value") else o) for o in outs], stats

    if flush:
        # the buffers of one unsegmented episode size the cap: two steps' rows behind the prefix, so the 4-step episode flushes once
        _, st0 = episode()
        os.environ["NAVILLM_EPISODE_MAX_ROWS"] = str(st0["prefix_rows"] + 2 * max(st0["suffix_rows"]))
    # the host side-car's destructors (nv_graph_destroy) run when Python's cycle collector gets to the previous episode's graphs: collect
    # them now and keep the collector out of the recorded episode, so that the call sequence does not depend on its timing
    gc.collect()
    gc.disable()
    del rec.calls[:]
    try:
        outs, stats = episode()
    finally:
        gc.enable()
    if flush:
        assert stats["segments_flushed"] >= 1, stats
    trace = list(rec.calls)
    by_symbol = {}
    for c in trace:
        s = c[:c.index("(")]
        by_symbol[s] = by_symbol.get(s, 0) + 1
    digests = {f"out{t}": _sha(o) for t, o in enumerate(outs)}
    digests.update({f"grad.{g}": _sha(t) for g, t in model.store.grad.items()})
    return dict(env=env, calls=len(trace), trace_sha256=hashlib.sha256("\n".join(trace).encode()).hexdigest(),
                by_symbol=dict(sorted(by_symbol.items())), digests=digests), trace


def run(out_path, repo, full_dir):
    sys.path.insert(0, repo)
    from navillm_amd import lib
    rec = Recorder(lib.load())
    lib._lib = rec                                    # every ops._L() from here on hands out the recorder
    result = {}
    for name, (env, kw) in SCENARIOS.items():
        result[name], trace = run_scenario(rec, env, **kw)
        print(f"{name}: {result[name]['calls']} calls, trace {result[name]['trace_sha256'][:12]}", flush=True)
        if full_dir:
            os.makedirs(full_dir, exist_ok=True)
            with open(os.path.join(full_dir, name + ".txt"), "w") as f:
                f.write("\n".join(trace) + "\n")
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")


def compare(base_a, base_b, head):
    a, b, h = (json.load(open(p)) for p in (base_a, base_b, head))
    ok = True
    for name in SCENARIOS:
        repro = a[name]["digests"] == b[name]["digests"]
        same_trace = a[name]["trace_sha256"] == b[name]["trace_sha256"] == h[name]["trace_sha256"]
        same_bits = h[name]["digests"] == a[name]["digests"]
        verdict = "trace equal" if same_trace else "TRACE DIFFERS"
        if repro:
            verdict += ", digests equal" if same_bits else ", DIGESTS DIFFER"
        else:
            verdict += ", not bit-reproducible at the base (compared by trace only)"
        print(f"{name}: {a[name]['calls']} calls; {verdict}")
        if not same_trace:
            for s in sorted(set(a[name]["by_symbol"]) | set(h[name]["by_symbol"])):
                if a[name]["by_symbol"].get(s) != h[name]["by_symbol"].get(s):
                    print(f"    {s}: base {a[name]['by_symbol'].get(s, 0)} calls, head {h[name]['by_symbol'].get(s, 0)}")
        ok = ok and same_trace and (same_bits or not repro)
    print("PASS" if ok else "FAIL")
    return 0 if ok else 1


if __name__ == "__main__":
    if len(sys.argv) >= 5 and sys.argv[1] == "compare":
        sys.exit(compare(*sys.argv[2:5]))
    if len(sys.argv) < 3 or sys.argv[1] != "run":
        sys.exit(__doc__)
    opt = dict(zip(sys.argv[3::2], sys.argv[4::2]))
    run(sys.argv[2], os.path.abspath(opt.get("--repo", ROOT)), opt.get("--full"))
