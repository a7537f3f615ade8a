"""GPU: the model built on the 64-wide attention kernels -- config.gpt2_small_shaped() (d = 768, 12 heads x 64, ff = 3072) cut to three
layers and a small vocabulary, and the full 12-layer shape once.

  1. navigation against the CPU oracle in bf16 and fp32 on the same weights (the method and criterion of
     tests/test_parity_gpu.py::_nav_vs_oracle), with unequal prompt lengths (left padding) and S > 128, so the RoPE positions, the
     packed-rows path and more than one query block are live.  At head_dim 64 the q|k|v projection takes the plain GEMM + nv_rope
     route (ops.qkv_rope); the 128-wide RoPE epilogue would rotate the wrong column pairs and this is the test that sees it.
  2. gradients of a training episode against the oracle's autograd, for the per-step recompute, the explicit prefix-reuse episode and
     its teacher-forced (batched) form.
  3. the training forms agree with each other: recompute, explicit begin_episode (per-step and teacher-forced) and the automatic lazy
     episode -- this drives epi_fwd / epi_bwd_* / kv_acc through the product path at head_dim 64.
  4. inference: K/V-cache navigation with prompt-prefix reuse equals the no-cache forward; greedy generation over the cache (the
     decoder runtime, nv_attn_decode_bf16, nv_attn_fwd_strided_dyn_bf16) equals the oracle recomputing the whole sequence per token.
  5. other head widths are still refused, loudly.
"""
import numpy as np
import pytest
import torch

from util import load_oracle, bf16_ulps_at_scale
from test_parity_gpu import maxerr
from test_episode_gpu import _episode
from test_parity_r4_gpu import _hip_episode, _rel, GRAD_NAMES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NV_ERR_SHAPE = -2


def _cfg64(layers=3, **over):
    from navillm_amd import config as nvcfg
    kw = dict(num_layers=layers, base_vocab_size=1000, enc_hidden_size=256, enc_num_heads=4, enc_intermediate_size=512, image_feat_size=768)
    kw.update(over)
    cfg = nvcfg.gpt2_small_shaped(**kw)
    assert cfg.head_dim == 64 and cfg.hidden_size == 768 and cfg.num_heads == 12 and cfg.intermediate_size == 3072
    return cfg


def _nav_vs_oracle64(cfg, B, S_instr, steps, tag, ragged):
    """tests/test_parity_gpu.py::_nav_vs_oracle, with sample b's instruction shortened by ragged * b tokens"""
    from navillm_amd import config as nvcfg
    from navillm_amd.nav_model import NavModel
    from navillm_amd.params import synth_state_dict
    from navillm_amd.synthetic import SyntheticEpisodes
    O = load_oracle()
    m = NavModel(nav_config=cfg, device=torch.device(DEV), seed=5)
    m.eval()
    P16 = synth_state_dict(cfg, 5)
    with torch.no_grad():
        assert m.load_reference_state_dict(P16) == len(P16)
    cfg32 = nvcfg.NavConfig(**{**cfg.__dict__, "precision": "fp32"})
    P32 = {k: v.float() for k, v in P16.items()}
    ep = SyntheticEpisodes(cfg, B, seed=77, instr_len=S_instr, device=torch.device(DEV))
    for b in range(B):
        ep.instr[b] = ep.instr[b][: S_instr - ragged * b]
    for step in range(steps):
        pin = ep.panorama_inputs()
        with torch.no_grad():
            pano = m("panorama", pin)
            ref_p = O.scene_encoder(P32, cfg32, pin["view_img_fts"].cpu(), pin["view_lens"].cpu(), pin["loc_fts"].cpu(), pin["nav_types"].cpu())
        assert maxerr(pano["pano_embeds"], ref_p["pano_embeds"]) < 1e-3 * ref_p["pano_embeds"].abs().max().item()
        ep.update_maps(pano["pano_embeds"], pano["pano_masks"], pin["cand_vpids"])
        nav = ep.nav_inputs(pano["pano_embeds"], pano["pano_masks"], pin["cand_vpids"])
        ids, am = ep.tokenise(nav, "<cls_1>")
        assert ids.shape[1] > 128 and int(am.sum(1).min()) < int(am.sum(1).max()), (ids.shape, am.sum(1))   # > 1 query block, left padding
        nav["input_ids"], nav["attention_mask"] = ids, am
        torch.manual_seed(100 + step)
        with torch.no_grad():
            out = m("navigation", nav)
        cpu = {k: (v.detach().cpu() if torch.is_tensor(v) else v) for k, v in nav.items()}
        cpu["hist_vis"] = [[v.cpu() for v in vis] for vis in nav["hist_vis"]]
        outs = {}
        for prec, P, c in (("bf16", P16, cfg), ("fp32", P32, cfg32)):
            torch.manual_seed(100 + step)
            with torch.no_grad():
                outs[prec] = O.navigation(P, c, cpu, ids, am)
        assert maxerr(out["fuse_embeds"], outs["fp32"]["fuse_embeds"]) < 1e-4
        lg = out["fuse_logits"]
        gap, e_hip, e_ref = maxerr(lg, outs["bf16"]["fuse_logits"]), maxerr(lg, outs["fp32"]["fuse_logits"]), \
            maxerr(outs["bf16"]["fuse_logits"], outs["fp32"]["fuse_logits"])
        ref16 = outs["bf16"]["fuse_logits"]
        scale = float(ref16[torch.isfinite(ref16)].abs().max())
        ulp = 2.0 ** (int(np.floor(np.log2(scale))) - 7)                      # spacing of the bf16 logits at their own magnitude
        print(f"[{tag} step {step}] S={ids.shape[1]} logits: |hip-orc32|={e_hip:.5f} vs |orc16-orc32|={e_ref:.5f} (ratio {e_hip / e_ref:.2f}); "
              f"|hip-orc16|={gap:.5f} = {gap / ulp:.2f} bf16 spacings at the logit scale {scale:.2f}")
        # the project's criterion (tests/test_parity_gpu.py): as close to the fp32 truth as the oracle's own bf16 run, x1.25 + one spacing
        assert e_hip <= 1.25 * e_ref + ulp, (e_hip, e_ref, ulp)
        targets = ep.teacher_targets(nav, last=False)
        ep.advance(nav, targets, out["fuse_embeds"])
    del m
    torch.cuda.empty_cache()


def test_hd64_navigation_vs_oracle_three_layers():
    _nav_vs_oracle64(_cfg64(3), 4, 200, 3, "hd64 x3", ragged=29)


def test_hd64_navigation_vs_oracle_full_gpt2_small_shape():
    """all 12 layers of config.gpt2_small_shaped(), the vocabulary cut so that the host oracle stays quick"""
    _nav_vs_oracle64(_cfg64(12), 2, 160, 2, "hd64 x12", ragged=41)


def test_hd64_episode_gradients_vs_oracle_autograd():
    """after tests/test_parity_r4_gpu.py::test_eight_layer_7b_width_episode_gradients_vs_oracle_autograd: selected gradients of a 2-step
    episode, all three explicit training forms, against the oracle's autograd in bf16 and fp32.  Tolerance form and values are that
    test's: e32 <= 1.5 * base + 2e-2 and e16 <= 2.5 * base + 2e-2 with base = |oracle bf16 - oracle fp32| (relative Frobenius)."""
    from navillm_amd import config as nvcfg
    from navillm_amd.nav_model import NavModel
    from navillm_amd.params import synth_state_dict
    O = load_oracle()
    cfg = _cfg64(3)
    names = [n for n in GRAD_NAMES if not n.startswith("lang_model.model.layers.") or int(n.split(".")[3]) < cfg.num_layers]
    names += [f"lang_model.model.layers.{cfg.num_layers - 1}.self_attn.v_proj.weight", "lang_model.model.layers.1.self_attn.o_proj.weight"]
    names = list(dict.fromkeys(names))
    B, steps = 2, 2
    m = NavModel(nav_config=cfg, device=torch.device(DEV), seed=5)
    m.eval()
    P16 = synth_state_dict(cfg, 5)
    with torch.no_grad():
        assert m.load_reference_state_dict(P16) == len(P16)
    rc, _, n_rc = _hip_episode(m, cfg, B, steps, "recompute", 83, 220, ragged=37, keep_inputs=True, grad_names=names)
    pr, _, n_pr = _hip_episode(m, cfg, B, steps, "prefix_reuse", 83, 220, ragged=37, keep_inputs=True, grad_names=names)
    tf, _, n_tf = _hip_episode(m, cfg, B, steps, "prefix_reuse_tf", 83, 220, ragged=37, keep_inputs=True, grad_names=names)
    for other in (pr, tf):
        for t in range(steps):
            assert torch.equal(rc[t]["ids"], other[t]["ids"]) and torch.equal(rc[t]["fuse_embeds"], other[t]["fuse_embeds"])
    del m
    torch.cuda.empty_cache()
    cfg32 = nvcfg.NavConfig(**{**cfg.__dict__, "precision": "fp32"})
    og = {}
    for prec, c in (("bf16", cfg), ("fp32", cfg32)):
        P = {k: (v.float() if prec == "fp32" else v.clone()).requires_grad_(k in names) for k, v in P16.items()}
        for t in range(steps):
            r = rc[t]
            pin = r["pin"]
            pano = O.scene_encoder(P, cfg32, pin["view_img_fts"], pin["view_lens"], pin["loc_fts"], pin["nav_types"])
            nav = dict(r["nav"])
            pe = pano["pano_embeds"]
            nav["vp_img_embeds"] = torch.cat([torch.zeros_like(pe[:, :1]), pe], 1)
            torch.manual_seed(900 + t)
            out = O.navigation(P, c, nav, r["ids"], r["am"])
            (O.action_loss(out["fuse_logits"], r["targets"]) / B).backward()
        og[prec] = {n: P[n].grad.detach().float().clone() for n in names}
        del P
    bad = []
    for n in names:
        base = _rel(og["bf16"][n], og["fp32"][n])
        line = f"[hd64 grad] {n}: |orc16-orc32| {base:.4f}"
        for tag, g in (("recompute", n_rc[n]), ("prefix_reuse", n_pr[n]), ("prefix_reuse_tf", n_tf[n])):
            e16, e32 = _rel(g, og["bf16"][n]), _rel(g, og["fp32"][n])
            line += f"; {tag} vs orc16 {e16:.4f} vs orc32 {e32:.4f}"
            if not (e32 <= 1.5 * base + 2e-2 and e16 <= 2.5 * base + 2e-2):
                bad.append((tag, n, e16, e32, base))
        print(line)
    assert not bad, bad


def test_hd64_training_forms_agree():
    """recompute vs explicit prefix reuse (per-step forward) vs teacher-forced (one batched forward), with the tolerances of
    tests/test_episode_gpu.py::test_prefix_episode_matches_per_step_recompute and
    ::test_teacher_forced_episode_batches_the_forward_and_matches ("mid" size: 3.0 spacings / 2.5e-2 per group against the recompute,
    2.0 spacings / 1.5e-2 batched against per-step forward)."""
    from navillm_amd.nav_model import NavModel
    cfg = _cfg64(3)
    m = NavModel(nav_config=cfg, device=torch.device(DEV), seed=12)
    m.eval()
    steps = 4
    l_ref, g_ref, _ = _episode(m, cfg, steps, use_prefix=False)
    l_ps, g_ps, st_ps = _episode(m, cfg, steps, use_prefix=True)
    l_tf, g_tf, _ = _episode(m, cfg, steps, use_prefix=True, teacher_forced=True)
    for t in range(steps):
        fin = torch.isfinite(l_ref[t])
        assert torch.equal(torch.isfinite(l_ps[t]), fin) and torch.equal(torch.isfinite(l_tf[t]), fin)
        u_ps, u_tf, u_b = bf16_ulps_at_scale(l_ps[t], l_ref[t]), bf16_ulps_at_scale(l_tf[t], l_ref[t]), bf16_ulps_at_scale(l_tf[t], l_ps[t])
        print(f"[hd64 forms step {t}] bf16 spacings: prefix-reuse vs recompute {u_ps:.2f}, batched vs recompute {u_tf:.2f}, batched vs per-step {u_b:.2f}")
        assert u_ps <= 3.0 and u_tf <= 3.0 and u_b <= 2.0
    for g in g_ref:
        a, b, c = _rel(g_ps[g], g_ref[g]), _rel(g_tf[g], g_ref[g]), _rel(g_tf[g], g_ps[g])
        print(f"[hd64 forms] gradient group {g}: prefix-reuse vs recompute {a:.4f}, batched vs recompute {b:.4f}, batched vs per-step {c:.4f}")
        assert a < 2.5e-2 and b < 2.5e-2 and c < 1.5e-2, (g, a, b, c)
    rows_ref = steps * sum(180 - 23 * b + 90 for b in range(3))
    assert st_ps["prefix_rows"] + sum(st_ps["suffix_rows"]) < 0.6 * rows_ref          # the prefix really was computed once


def test_hd64_automatic_lazy_episode_equals_explicit_teacher_forced():
    """the default training form: the unmodified rollout, no begin_episode / finish_episode.  As at head_dim 128
    (tests/test_auto_episode_gpu.py) a teacher-forced rollout through the automatic lazy episode is bit-identical to the explicit
    teacher_forced=True episode: same logits, same gradient buffers."""
    from test_auto_episode_gpu import _model, _rollouts, _values
    cfg = _cfg64(3)
    plan = [(3, 3, 150, "teacher"), (2, 2, 140, "teacher")]
    m = _model(cfg, auto=True)
    seen_a, loss_a = _rollouts(m, cfg, plan, None, accum=1)
    torch.nn.utils.clip_grad_norm_(m.parameters(), 40.)                      # hands the pending gradients over
    val_a = _values(seen_a)
    g_a = {g: t.detach().clone() for g, t in m.store.grad.items()}
    assert m.auto_stats["opened"] == len(plan), m.auto_stats
    del m
    torch.cuda.empty_cache()
    m = _model(cfg, auto=False)
    seen_e, loss_e = _rollouts(m, cfg, plan, True, accum=1)
    torch.nn.utils.clip_grad_norm_(m.parameters(), 40.)
    val_e = _values(seen_e)
    assert loss_a == loss_e, (loss_a, loss_e)
    assert len(val_a) == len(val_e) and all(torch.equal(a, e) for a, e in zip(val_a, val_e))
    for g, t in m.store.grad.items():
        assert torch.equal(t, g_a[g]), g


def test_hd64_prefix_kv_reuse_matches_full_recompute_over_an_episode():
    """the criterion of tests/test_kvcache_gpu.py::test_prefix_kv_reuse_matches_full_recompute_over_an_episode: no-grad navigation
    steps through the K/V cache and through the full forward: |cached - full| < 0.06, same argmax wherever the margin allows, and
    only the prompt suffix recomputed from step 1 on."""
    from navillm_amd.nav_model import NavModel
    from navillm_amd.synthetic import SyntheticEpisodes
    cfg = _cfg64(3)
    m = NavModel(nav_config=cfg, device=torch.device(DEV), seed=9)
    m.eval()
    B = 3
    eps = [SyntheticEpisodes(cfg, B, seed=31, instr_len=300, device=torch.device(DEV)) for _ in range(2)]
    m.enable_kv_cache(B, capacity=1024)
    for step in range(5):
        logits = []
        for use_cache, ep in ((True, eps[0]), (False, eps[1])):
            kv, m.kv = m.kv, (m.kv if use_cache else None)
            with torch.no_grad():
                pin = ep.panorama_inputs()
                pano = m("panorama", pin)
                ep.update_maps(pano["pano_embeds"], pano["pano_masks"], pin["cand_vpids"])
                nav = ep.nav_inputs(pano["pano_embeds"], pano["pano_masks"], pin["cand_vpids"])
                nav["input_ids"], nav["attention_mask"] = ep.tokenise(nav, "<cls_1>")
                torch.manual_seed(500 + step)
                out = m("navigation", nav)
            m.kv = kv
            logits.append(out["fuse_logits"].float().cpu())
            tg = ep.teacher_targets(nav, last=False)
            ep.advance(nav, tg, out["fuse_embeds"])
        a, b = logits
        fin = torch.isfinite(b)
        assert torch.equal(torch.isfinite(a), fin)
        gap = (a[fin] - b[fin]).abs().max().item()
        st = m.kv.last_stats
        print(f"[hd64 kv step {step}] S={nav['input_ids'].shape[1]} prefix={st['prefix']} new={st['new']} |cached-full|={gap:.4f}")
        assert gap < 0.06
        if step > 0:
            assert min(st["prefix"]) > 300 and max(st["new"]) < 120, st
        top2 = b.masked_fill(~fin, -1e9).topk(2, dim=1).values
        safe = (top2[:, 0] - top2[:, 1]) > 4 * gap + 1e-3
        assert torch.equal(a.argmax(1)[safe], b.argmax(1)[safe])


def test_hd64_greedy_generation_matches_oracle_recompute():
    """tests/test_kvcache_gpu.py::test_greedy_generation_matches_oracle_recompute at head_dim 64: K/V-cache greedy decoding (prefill
    through the strided forward, then nv_attn_decode_bf16 steps inside the decoder runtime) against the oracle recomputing the whole
    sequence for every token: identical tokens up to the first step whose top-2 margin is inside the bf16 noise."""
    from navillm_amd.nav_model import NavModel
    from navillm_amd.params import synth_state_dict
    from navillm_amd.kvcache import KVCacheLM
    from test_kvcache_gpu import _gen_case
    O = load_oracle()
    cfg = _cfg64(2)
    m = NavModel(nav_config=cfg, device=torch.device(DEV), seed=5)
    m.eval()
    P16 = synth_state_dict(cfg, 5)
    with torch.no_grad():
        assert m.load_reference_state_dict(P16) == len(P16)
    B = 3
    ids_t, am, cand, hist = _gen_case(cfg, B, 123)
    eos, pad, max_new = 2, 0, 10
    ref_ids, _ = O.greedy_generate(P16, cfg, ids_t, am, cand_vis=cand, hist_vis=hist, max_new_tokens=max_new, eos_token_id=eos, pad_token_id=pad,
                                   trie=None)
    ids_l, vix_l, vis_all, _ = m._vis_layout(ids_t, am, cand.to(DEV), hist.to(DEV), None)
    kv = KVCacheLM(m, B, capacity=256)
    got = kv.generate(ids_l, vix_l, vis_all, max_new_tokens=max_new, eos_token_id=eos, pad_token_id=pad, trie=None)
    print("oracle:", ref_ids)
    print("hip   :", got)
    for b in range(B):
        agree = 0
        for x, y in zip(got[b], ref_ids[b]):
            if x != y:
                break
            agree += 1
        if agree < len(ref_ids[b]):
            seq = torch.tensor(ids_t[b, am[b].bool()].tolist() + ref_ids[b][:agree])[None]
            _, lg, _ = O.lm_forward(P16, cfg, seq, torch.ones_like(seq), cand_vis=cand[2 * b:2 * b + 2], hist_vis=hist[b:b + 1])
            lgl = lg[0, -1].float()
            margin = (lgl[ref_ids[b][agree]] - lgl[got[b][agree]]).item()
            print(f"sample {b}: diverged at step {agree}, oracle margin {margin:.4f}")
            assert abs(margin) < 0.05, (b, agree, margin)
        assert agree >= 1 or len(ref_ids[b]) == 0


def test_other_head_widths_are_still_refused():
    from navillm_amd import config as nvcfg, lib, ops
    from navillm_amd.nav_model import NavModel
    with pytest.raises(NotImplementedError, match="64 and 128"):
        NavModel(nav_config=nvcfg.NavConfig(hidden_size=768, num_heads=8), device=torch.device(DEV))
    L = lib.load()
    B, S, H, hd = 1, 64, 2, 96
    qkv = torch.zeros(B * S, 3 * H * hd, dtype=torch.bfloat16, device=DEV)
    out = torch.full((B * S, H * hd), float("nan"), dtype=torch.bfloat16, device=DEV)
    lse = torch.full((B, H, S), float("nan"), dtype=torch.float32, device=DEV)
    kv0 = torch.zeros(B, dtype=torch.int32, device=DEV)
    assert L.nv_attn_fwd_bf16(qkv.data_ptr(), out.data_ptr(), lse.data_ptr(), kv0.data_ptr(), B, S, H, hd, 0, ops._st()) == NV_ERR_SHAPE
    torch.cuda.synchronize()
    assert bool(torch.isnan(out.float()).all()) and bool(torch.isnan(lse).all())
    assert not L.nv_decoder_create(2, 768, 8, 96, 3072, 1e-6)
    h = L.nv_decoder_create(2, 768, 12, 64, 3072, 1e-6)
    assert h
    L.nv_decoder_destroy(h)
