"""GPU: the fp64 reference checks of tests/test_attention_ref_gpu.py at head_dim 64 -- every sequence and episode attention entry point
of the C ABI over the same case grid (padded / strided / dyn / varlen / episode forward, all backward forms with and without RoPE^T and
kv_acc, store and add), with the same NaN-prefill discipline: rows outside the documented write set stay NaN, rows inside are finite,
rows that see no key and keys no query sees are exact zeros.  Plus the streaming decode kernel (nv_attn_decode_bf16), which has no fp64
check elsewhere, at head_dim 64 and 128.

The case lists, the reference's width-independent helpers, BOUND and MAG_FLOOR are imported from that file; what depends on the head
width (row generation, ref_attention, the RoPE tables, check) is restated here for HD = 64.

Bounds.  The error model in that file's docstring does not depend on the head width: the rounding points are the same, and the two
products summed over the head width (q k^T, dO V^T) get shorter, none gets longer.  So BOUND is taken as it stands there.  Worst values
measured at head_dim 64 on an MI355X over this file's cases (rel, max), beside each bound:
  out    (6e-3, 1.0e-2)   : 2.9e-3, 4.9e-3
  dq     (1.2e-2, 2.5e-2) : 4.9e-3, 1.0e-2  (through RoPE^T)
  dk     (1.2e-2, 2.5e-2) : 4.7e-3, 1.2e-2  (through RoPE^T)
  dv     (1.0e-2, 1.5e-2) : 4.8e-3, 6.5e-3
  kv_dk  (6e-3, 1.0e-2)   : 2.0e-3, 3.2e-3  (fp32 accumulator: no bf16 store)
  kv_dv  (5e-3, 8e-3)     : 2.0e-3, 3.3e-3
  lse2   2e-5             : 4.8e-6 log2 units

MAG_FLOOR (64.0, kept) is a cap, not a measurement: an output that cancels is judged against the size of its terms.  The property
that file states -- for "randn" values the reference itself stays above the floor, so the floor only engages on the "peaked" /
"planted" cases -- rests on a query summing many keys (its terms cancel to ~1/sqrt(keys) at most).  Counted on the CPU with
ref_attention alone over this grid at HD = 64, per (sample or step, head) and output, before the first GPU run:
  * every "randn" sample or step with three or more query rows and a query that sees three or more keys: 0 heads below the floor (smallest reference norm /
    (mag norm / MAG_FLOOR) over the padded and packed cases: 3.4 for out, 4.2 for dq, 4.7 for dk, 4.6 for dv);
  * queries that see ONE key (S = 1, kv_start = S - 1): the softmax is the constant 1, dS = P (dP - D) vanishes term by term and dQ / dK
    are identically zero -- nothing cancels, there is no relative error to take (17 sample-heads of the grid);
  * queries that see TWO keys (the 1-row steps over a 1-row prefix of the T = 128 episode case): dQ / dK are a single difference,
    which falls below 1/64 of its terms by chance in 3 of ~170 such step-heads (reference / floor = 0.74, 0.81, 0.94).
  * on the GPU, where the backward reference is fed the kernel's own out / lse2, one more: dK of the single own key of a 1-row step
    over a 257-row prefix (one query, one term).
check() therefore asserts, for "randn" cases, that no head of a sample / step with more than two query rows whose queries see more
than two keys -- every output of it sums three or more terms somewhere -- is judged against the floor (floor_dist, floor_engaged); the
one- and two-term heads keep the floor as their yardstick, as in that file.
"""
import math

import numpy as np
import pytest
import torch

from test_attention_ref_gpu import (BF, F32, F64, I32, NAN, INF, BOUND, MAG_FLOOR, SEQ_CASES, STRIDED_CASES, VARLEN_CASES, EPI_CASES,
                                    dev, L, st, ok, nans, seed_of, gen, plant_keys, check_lse, all_nan, causal_vis, _layout)

pytestmark = pytest.mark.gpu

HD = 64
SCALE = HD ** -0.5


def make_rows(n, H, dist, g):
    """fp32 [n, 3, H, HD] (q | k | v), randn * 0.8; "peaked": q x7, so the softmax is near one-hot and the exp2 rescale matters"""
    x = torch.randn(n, 3, H, HD, generator=g, device=dev()) * 0.8
    if dist == "peaked":
        x[:, 0] *= 7.0
    return x


def plant(x, key_rows, g, u=None):
    """every query gets a common direction u and the keys key_rows (+1.5 u, so they stay distinct) score ~17 nats above the rest
    for every query that sees them: placed in a late key tile, the online max jumps there and the earlier tiles' sums are
    rescaled by ~e^-17"""
    if u is None:
        u = torch.randint(0, 2, (HD,), generator=g, device=dev()).float() * 2 - 1
    x[:, 0] += u
    x[key_rows, 1] += 1.5 * u
    return u


def split(qkv_rows, H):
    x = qkv_rows.double().view(-1, 3, H, HD)
    return x[:, 0], x[:, 1], x[:, 2]


def ref_attention(q, k, v, visible, dout, scale=SCALE, out_in=None, lse2_in=None):
    """fp64 attention of one sample (or one episode step), head by head.  q [nq, H, HD], k / v [nk, H, HD], visible bool [nq, nk],
    dout [nq, H, HD] or None.  Returns out [nq, H, HD], lse2 [H, nq] (logsumexp(scale q k^T) / ln 2 over the visible keys, +inf
    for a row that sees none), dq, dk, dv (None without dout) and mag: the same products taken over absolute values
    (P |V|, scale P (|dP| + |D|) |K|, ...), the size of the terms each output sums, which check() uses where an output cancels.
    out_in / lse2_in: the backward's own inputs (the kernel forward's bf16 out [nq, H, HD] and lse2 [H, nq]).  The backward entry
    points are specified on them -- P = exp2(scale log2(e) q k^T - lse2_in), D = rowsum(dO * out_in), dS = P (dP - D) -- and with
    them the reference keeps the kernel's exact cancellation where a row's softmax is near one-hot (D ~ dP)."""
    nq, H, _ = q.shape
    q, k, v = q.double(), k.double(), v.double()
    seen = visible.any(1)
    out = torch.zeros(nq, H, HD, dtype=F64, device=q.device)
    lse2 = torch.full((H, nq), INF, dtype=F64, device=q.device)
    mag = {"out": torch.zeros_like(out)}
    dq = dk = dv = None
    if dout is not None:
        dout = dout.double()
        dq, dk, dv = torch.zeros_like(q), torch.zeros_like(k), torch.zeros_like(v)
        mag.update(dq=torch.zeros_like(q), dk=torch.zeros_like(k), dv=torch.zeros_like(v))
    ln2 = math.log(2.0)
    for h in range(H):
        s = (q[:, h] @ k[:, h].T * scale).masked_fill(~visible, -INF)
        lse = torch.logsumexp(s, 1)
        p = torch.exp(s - torch.where(seen, lse, 0.0)[:, None])          # masked: exp(-inf) = 0; a row that sees nothing: all 0
        out[:, h] = p @ v[:, h]
        mag["out"][:, h] = p @ v[:, h].abs()
        lse2[h] = torch.where(seen, lse / ln2, INF)
        if dout is not None:
            do = dout[:, h]
            if lse2_in is not None:
                p = torch.exp(s - lse2_in[h].double()[:, None] * ln2)    # +inf (a row that sees nothing): 0
            o = out[:, h] if out_in is None else out_in[:, h].double()
            dp, dsum = do @ v[:, h].T, (do * o).sum(1, keepdim=True)
            ds, dsa = p * (dp - dsum), p * (dp.abs() + dsum.abs())
            dq[:, h] = scale * ds @ k[:, h]
            dk[:, h] = scale * ds.T @ q[:, h]
            dv[:, h] = p.T @ do
            mag["dq"][:, h] = scale * dsa @ k[:, h].abs()
            mag["dk"][:, h] = scale * dsa.T @ q[:, h].abs()
            mag["dv"][:, h] = p.T @ do.abs()
    return out, lse2, dq, dk, dv, mag


def rope_tables(n):
    inv = 1.0 / (10000.0 ** (torch.arange(0, HD, 2, dtype=F64) / HD))
    fr = torch.outer(torch.arange(n, dtype=F64), inv)
    emb = torch.cat([fr, fr], -1)
    return emb.cos().to(BF).to(dev()).contiguous(), emb.sin().to(BF).to(dev()).contiguous()


def rope_t(gr, cos, sin, pos):
    """transpose of the HF rotation x' = x cos + rotate_half(x) sin, in fp64 with the bf16 tables, rows at positions pos"""
    c, s = cos[pos].double()[:, None], sin[pos].double()[:, None]
    g1, g2 = gr[..., :HD // 2], gr[..., HD // 2:]
    return torch.cat([g1 * c[..., :HD // 2] + g2 * s[..., HD // 2:], g2 * c[..., HD // 2:] - g1 * s[..., :HD // 2]], -1)


def floor_dist(dist, vis):
    """the `dist` check() is told: None (no floor accounting) where the sample / step has at most two query rows (dK / dV of its own
    keys then sum at most two terms) or no query of it sees more than two keys (dQ sums at most two)"""
    return dist if vis.shape[0] > 2 and int(vis.sum(1).max()) > 2 else None


FLOOR_HITS = []   # (tag, name): a "randn" head judged against the floor although its reference is not identically zero


def floor_engaged(ref, mag):
    """per head: is the reference nonzero and smaller than mag / MAG_FLOOR (norm or max), i.e. would the floor set the yardstick"""
    rn, mn = ref.norm(dim=(0, 2)), mag.norm(dim=(0, 2)) / MAG_FLOOR
    rm, mm = ref.abs().amax(dim=(0, 2)), mag.abs().amax(dim=(0, 2)) / MAG_FLOOR
    return ((rn > 0) & (rn < mn)) | ((rm > 0) & (rm < mm))


def check(tag, name, got, ref, mag, zero_rows=None, dist=None):
    """got (kernel) / ref (fp64) / mag (ref_attention's magnitude of the same output), [n, H, HD] of one sample or step: finite,
    exact zeros on zero_rows and where nothing is summed, and per head within BOUND[name]"""
    if got.shape[0] == 0:
        return
    got = got.double()
    assert torch.isfinite(got).all(), f"{tag} {name}: non-finite value inside the write set"
    if zero_rows is not None and bool(zero_rows.any()):
        assert bool((got[zero_rows] == 0).all()), f"{tag} {name}: rows that see no key / no query are not exact zeros"
    if dist == "randn":                              # None: another distribution, or at most two keys per query (module docstring)
        n_floor = int(floor_engaged(ref, mag).sum())
        if n_floor:
            FLOOR_HITS.append((tag, name, n_floor))
        assert n_floor == 0, f"{tag} {name}: MAG_FLOOR engages on {n_floor} head(s) of a randn case"
    err = got - ref
    en, emax = err.norm(dim=(0, 2)), err.abs().amax(dim=(0, 2))
    rn = torch.maximum(ref.norm(dim=(0, 2)), mag.norm(dim=(0, 2)) / MAG_FLOOR)
    rmax = torch.maximum(ref.abs().amax(dim=(0, 2)), mag.abs().amax(dim=(0, 2)) / MAG_FLOOR)
    live = rn > 0
    assert bool((emax[~live] == 0).all()), f"{tag} {name}: nonzero where no term is summed"
    if not bool(live.any()):
        return
    rel = (en[live] / rn[live]).max().item()
    mx = (emax[live] / rmax[live]).max().item()
    print(f"ATTNREF64 {name} rel={rel:.3e} max={mx:.3e} {tag}")
    b_rel, b_max = BOUND[name]
    assert rel <= b_rel and mx <= b_max, f"{tag} {name}: rel {rel:.3e} (bound {b_rel:.1e}), max {mx:.3e} (bound {b_max:.1e})"


def parts(buf, H):
    """dqkv rows [n, 3*H*HD] -> dq, dk, dv views [n, H, HD]"""
    x = buf.view(-1, 3, H, HD)
    return x[:, 0], x[:, 1], x[:, 2]


@pytest.mark.parametrize("B,S,H,kvs,qmin,dist", SEQ_CASES, ids=[f"B{c[0]}-S{c[1]}-H{c[2]}-kv{'_'.join(map(str, c[3][:2]))}-q{c[4]}-{c[5]}"
                                                                 for c in SEQ_CASES])
def test_hd64_padded_fwd_bwd_rope_vs_fp64(B, S, H, kvs, qmin, dist):
    """nv_attn_fwd_bf16, nv_attn_bwd_bf16 and nv_attn_bwd_rope_bf16.  dQ rows below q_row_min are not written (the header: "left
    untouched"); dO of those rows is random here and must not matter.  kv_start = S (a fully padded sample) is accepted: its out
    rows are exact zeros with lse2 = +inf, and all its gradients are exact zeros."""
    g = gen(seed_of("seq", B, S, H, kvs, qmin, dist))
    x = make_rows(B * S, H, dist, g)
    if dist == "planted":
        plant(x, [b * S + j for b in range(B) for j in plant_keys(S)], g)
    qkv = x.reshape(B * S, 3 * H * HD).to(BF).contiguous()
    kv = torch.tensor(kvs, dtype=I32, device=dev())
    out, lse = nans(B * S, H * HD), nans(B, H, S, dtype=F32)
    ok(L().nv_attn_fwd_bf16(qkv.data_ptr(), out.data_ptr(), lse.data_ptr(), kv.data_ptr(), B, S, H, HD, qmin, st()), "nv_attn_fwd_bf16")
    dout = (torch.randn(B * S, H * HD, generator=g, device=dev()) * 0.5).to(BF)
    ws = torch.empty(L().nv_attn_bwd_workspace_bytes(B, S, H) // 4, dtype=F32, device=dev())
    dqkv = nans(B * S, 3 * H * HD)
    ok(L().nv_attn_bwd_bf16(qkv.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), kv.data_ptr(), dqkv.data_ptr(), ws.data_ptr(),
                            B, S, H, HD, qmin, st()), "nv_attn_bwd_bf16")
    cos, sin = rope_tables(S)
    dqkv_r = nans(B * S, 3 * H * HD)
    ok(L().nv_attn_bwd_rope_bf16(qkv.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), kv.data_ptr(), dqkv_r.data_ptr(),
                                 ws.data_ptr(), cos.data_ptr(), sin.data_ptr(), B, S, H, HD, qmin, st()), "nv_attn_bwd_rope_bf16")
    torch.cuda.synchronize()
    for b in range(B):
        tag = f"padded b={b}"
        rows = slice(b * S, (b + 1) * S)
        q, k, v = split(qkv[rows], H)
        vis = causal_vis(S, kvs[b])[qmin:]
        o = out[rows].view(S, H, HD)
        r_out, r_lse, r_dq, r_dk, r_dv, mag = ref_attention(q[qmin:], k, v, vis, dout[rows].view(S, H, HD)[qmin:], out_in=o[qmin:],
                                                            lse2_in=lse[b][:, qmin:])
        q_zero, k_zero = ~vis.any(1), ~vis.any(0)
        dist_ = floor_dist(dist, vis)
        check(tag + " fwd", "out", o[qmin:], r_out, mag["out"], q_zero, dist=dist_)
        all_nan(o[:qmin], tag + " fwd out below q_row_min")
        check_lse(tag + " fwd", lse[b][:, qmin:], r_lse)
        all_nan(lse[b][:, :qmin], tag + " fwd lse2 below q_row_min")
        pos = torch.arange(S, device=dev())
        for name, buf, rot in (("bwd", dqkv, False), ("bwd_rope", dqkv_r, True)):
            dq, dk, dv = parts(buf[rows], H)
            rq = rope_t(r_dq, cos, sin, pos[qmin:]) if rot else r_dq
            rk = rope_t(r_dk, cos, sin, pos) if rot else r_dk
            check(f"{tag} {name}", "dq", dq[qmin:], rq, mag["dq"], q_zero, dist=dist_)
            all_nan(dq[:qmin], f"{tag} {name} dQ below q_row_min")
            check(f"{tag} {name}", "dk", dk, rk, mag["dk"], k_zero, dist=dist_)
            check(f"{tag} {name}", "dv", dv, r_dv, mag["dv"], k_zero, dist=dist_)


@pytest.mark.parametrize("B,S,Sst,H,kvs,qmin,plen,dist", STRIDED_CASES,
                         ids=[f"B{c[0]}-S{c[1]}-st{c[2]}-H{c[3]}-q{c[5]}-{c[7]}" for c in STRIDED_CASES])
def test_hd64_strided_fwd_dyn_bwd_kvacc_vs_fp64(B, S, Sst, H, kvs, qmin, plen, dist):
    """nv_attn_fwd_strided_bf16, nv_attn_fwd_strided_dyn_bf16, nv_attn_bwd_strided_bf16, nv_attn_bwd_strided_kvacc_bf16 (first = 1:
    stored; first = 0: added onto known fp32 values).  Rows [S, S_stride) of every sample are never written; with kv_acc the bf16
    dK | dV of the prefix keys are not written and kv_acc rows >= prefix_len stay untouched.  dO of rows below q_row_min is zero (the
    header's contract for this entry point)."""
    g = gen(seed_of("strided", B, S, Sst, H, kvs, qmin, plen, dist))
    x = make_rows(B * Sst, H, dist, g)
    if dist == "planted":
        plant(x, [b * Sst + j for b in range(B) for j in plant_keys(S)], g)
    qkv = x.reshape(B * Sst, 3 * H * HD).to(BF).contiguous()
    kv = torch.tensor(kvs, dtype=I32, device=dev())
    out, lse = nans(B * Sst, H * HD), nans(B, H, Sst, dtype=F32)
    ok(L().nv_attn_fwd_strided_bf16(qkv.data_ptr(), out.data_ptr(), lse.data_ptr(), kv.data_ptr(), B, S, Sst, H, HD, qmin, st()),
       "nv_attn_fwd_strided_bf16")
    dyn = torch.tensor([S, qmin], dtype=I32, device=dev())
    out_d, lse_d = nans(B * Sst, H * HD), nans(B, H, Sst, dtype=F32)
    ok(L().nv_attn_fwd_strided_dyn_bf16(qkv.data_ptr(), out_d.data_ptr(), lse_d.data_ptr(), kv.data_ptr(), B, Sst, H, HD, dyn.data_ptr(),
                                        st()), "nv_attn_fwd_strided_dyn_bf16")
    dout = (torch.randn(B, Sst, H * HD, generator=g, device=dev()) * 0.5)
    dout[:, :qmin] = 0
    dout = dout.reshape(B * Sst, H * HD).to(BF)
    ws = torch.empty(L().nv_attn_bwd_workspace_bytes(B, Sst, H) // 4, dtype=F32, device=dev())
    dqkv = nans(B * Sst, 3 * H * HD)
    ok(L().nv_attn_bwd_strided_bf16(qkv.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), kv.data_ptr(), dqkv.data_ptr(),
                                    ws.data_ptr(), B, S, Sst, H, HD, qmin, st()), "nv_attn_bwd_strided_bf16")
    pl = torch.tensor(plen, dtype=I32, device=dev())
    runs = {}
    for first in (1, 0):
        acc = nans(B * Sst, 2 * H * HD, dtype=F32)
        base = torch.randn(B, Sst, 2 * H * HD, generator=g, device=dev())
        if not first:
            for b in range(B):
                acc.view(B, Sst, -1)[b, :plen[b]] = base[b, :plen[b]]
        dq_acc = nans(B * Sst, 3 * H * HD)
        ok(L().nv_attn_bwd_strided_kvacc_bf16(qkv.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), kv.data_ptr(), dq_acc.data_ptr(),
                                              ws.data_ptr(), acc.data_ptr(), pl.data_ptr(), first, B, S, Sst, H, HD, qmin, st()),
           "nv_attn_bwd_strided_kvacc_bf16")
        runs[first] = (dq_acc, acc, base)
    torch.cuda.synchronize()
    for b in range(B):
        tag = f"strided b={b}"
        rows = slice(b * Sst, b * Sst + S)
        q, k, v = split(qkv[rows], H)
        vis = causal_vis(S, kvs[b])[qmin:]
        r_out, r_lse, r_dq, r_dk, r_dv, mag = ref_attention(q[qmin:], k, v, vis, dout[rows].view(S, H, HD)[qmin:],
                                                            out_in=out[rows].view(S, H, HD)[qmin:], lse2_in=lse[b][:, qmin:S])
        q_zero, k_zero = ~vis.any(1), ~vis.any(0)
        dist_ = floor_dist(dist, vis)
        for name, o_, l_ in (("fwd_strided", out, lse), ("fwd_strided_dyn", out_d, lse_d)):
            o = o_.view(B, Sst, H, HD)[b]
            check(f"{tag} {name}", "out", o[qmin:S], r_out, mag["out"], q_zero, dist=dist_)
            all_nan(o[:qmin], f"{tag} {name} out below q_row_min")
            all_nan(o[S:], f"{tag} {name} out rows >= S")
            check_lse(f"{tag} {name}", l_[b][:, qmin:S], r_lse)
            all_nan(l_[b][:, :qmin], f"{tag} {name} lse2 below q_row_min")
            all_nan(l_[b][:, S:], f"{tag} {name} lse2 rows >= S")
        dq, dk, dv = parts(dqkv.view(B, Sst, -1)[b], H)
        check(f"{tag} bwd_strided", "dq", dq[qmin:S], r_dq, mag["dq"], q_zero, dist=dist_)
        check(f"{tag} bwd_strided", "dk", dk[:S], r_dk, mag["dk"], k_zero, dist=dist_)
        check(f"{tag} bwd_strided", "dv", dv[:S], r_dv, mag["dv"], k_zero, dist=dist_)
        all_nan(dq[:qmin], f"{tag} bwd_strided dQ below q_row_min")
        all_nan(dqkv.view(B, Sst, -1)[b, S:], f"{tag} bwd_strided rows >= S")
        P = plen[b]
        for first, (dq_acc, acc, base) in runs.items():
            t2 = f"{tag} kvacc first={first}"
            dq, dk, dv = parts(dq_acc.view(B, Sst, -1)[b], H)
            check(t2, "dq", dq[qmin:S], r_dq, mag["dq"], q_zero, dist=dist_)
            all_nan(dq[:qmin], t2 + " dQ below q_row_min")
            check(t2, "dk", dk[P:S], r_dk[P:], mag["dk"][P:], k_zero[P:], dist=dist_)
            check(t2, "dv", dv[P:S], r_dv[P:], mag["dv"][P:], k_zero[P:], dist=dist_)
            all_nan(dk[:P], t2 + " bf16 dK of prefix keys")
            all_nan(dv[:P], t2 + " bf16 dV of prefix keys")
            all_nan(dq_acc.view(B, Sst, -1)[b, S:], t2 + " rows >= S")
            a = acc.view(B, Sst, 2, H, HD)[b]
            got = a[:P] if first else a[:P] - base[b, :P].view(P, 2, H, HD)
            check(t2, "kv_dk", got[:, 0], r_dk[:P], mag["dk"][:P], k_zero[:P], dist=dist_)
            check(t2, "kv_dv", got[:, 1], r_dv[:P], mag["dv"][:P], k_zero[:P], dist=dist_)
            all_nan(a[P:], t2 + " kv_acc rows >= prefix_len")


@pytest.mark.parametrize("lens,H,qmin,pos0,dist", VARLEN_CASES,
                         ids=[f"n{len(c[0])}-S{max(c[0])}-H{c[1]}-q{c[2]}-{c[4]}" for c in VARLEN_CASES])
def test_hd64_varlen_fwd_bwd_vs_fp64(lens, H, qmin, pos0, dist):
    """nv_attn_fwd_varlen_bf16 and nv_attn_bwd_varlen_bf16 without and with RoPE^T (position pos0[b] + i).  Query rows below a
    sample's first computed row (q_row_min, or its own last 128-row block for -1) are not written, in out, lse2 and dQ alike;
    lse2 entries >= the sample's length are not written either."""
    g = gen(seed_of("varlen", lens, H, qmin, pos0, dist))
    B, Smax = len(lens), max(lens)
    cu = [0] + list(np.cumsum(lens))
    rows = cu[-1]
    x = make_rows(rows, H, dist, g)
    if dist == "planted":
        plant(x, [cu[b] + j for b in range(B) for j in plant_keys(lens[b])], g)
    qkv = x.reshape(rows, 3 * H * HD).to(BF).contiguous()
    cu_d = torch.tensor(cu, dtype=I32, device=dev())
    p0 = torch.tensor(pos0, dtype=I32, device=dev())
    out, lse = nans(rows, H * HD), nans(B, H, Smax, dtype=F32)
    ok(L().nv_attn_fwd_varlen_bf16(qkv.data_ptr(), out.data_ptr(), lse.data_ptr(), cu_d.data_ptr(), p0.data_ptr(), B, Smax, H, HD, qmin,
                                   st()), "nv_attn_fwd_varlen_bf16")
    dout = (torch.randn(rows, H * HD, generator=g, device=dev()) * 0.5).to(BF)
    ws = torch.empty(L().nv_attn_bwd_workspace_bytes(B, Smax, H) // 4, dtype=F32, device=dev())
    cos, sin = rope_tables(max(p + n for p, n in zip(pos0, lens)))
    res = {}
    for rot in (False, True):
        dqkv = nans(rows, 3 * H * HD)
        ok(L().nv_attn_bwd_varlen_bf16(qkv.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), cu_d.data_ptr(), p0.data_ptr(),
                                       dqkv.data_ptr(), ws.data_ptr(), cos.data_ptr() if rot else None, sin.data_ptr() if rot else None,
                                       B, Smax, rows, H, HD, qmin, st()), "nv_attn_bwd_varlen_bf16")
        res[rot] = dqkv
    torch.cuda.synchronize()
    for b in range(B):
        S = lens[b]
        tag = f"varlen b={b} S={S}"
        qm = min(qmin, S) if qmin >= 0 else ((S - 1) // 128) * 128
        r = slice(cu[b], cu[b + 1])
        q, k, v = split(qkv[r], H)
        vis = causal_vis(S, 0)[qm:]
        o = out[r].view(S, H, HD)
        r_out, r_lse, r_dq, r_dk, r_dv, mag = ref_attention(q[qm:], k, v, vis, dout[r].view(S, H, HD)[qm:], out_in=o[qm:],
                                                            lse2_in=lse[b][:, qm:S])
        k_zero = ~vis.any(0)
        dist_ = floor_dist(dist, vis)
        check(tag + " fwd", "out", o[qm:], r_out, mag["out"], dist=dist_)
        all_nan(o[:qm], tag + " fwd out below the first computed row")
        check_lse(tag + " fwd", lse[b][:, qm:S], r_lse)
        all_nan(lse[b][:, :qm], tag + " fwd lse2 below the first computed row")
        all_nan(lse[b][:, S:], tag + " fwd lse2 beyond the sample")
        pos = pos0[b] + torch.arange(S, device=dev())
        for rot, buf in res.items():
            t2 = f"{tag} bwd rope={rot}"
            dq, dk, dv = parts(buf[r], H)
            check(t2, "dq", dq[qm:], rope_t(r_dq, cos, sin, pos[qm:]) if rot else r_dq, mag["dq"], dist=dist_)
            all_nan(dq[:qm], t2 + " dQ below the first computed row")
            check(t2, "dk", dk, rope_t(r_dk, cos, sin, pos) if rot else r_dk, mag["dk"], k_zero, dist=dist_)
            check(t2, "dv", dv, r_dv, mag["dv"], k_zero, dist=dist_)


@pytest.mark.parametrize("lps,ns,H,rope,dist", EPI_CASES,
                         ids=[f"B{len(c[0])}-T{len(c[1])}-lp{max(c[0])}-n{max(map(max, c[1]))}-H{c[2]}-{c[4]}" for c in EPI_CASES])
def test_hd64_episode_fwd_bwd_vs_fp64(lps, ns, H, rope, dist):
    """nv_attn_fwd_episode_bf16 (step blocks last step first, with sentinel gap rows), then over a gapless sample-major layout
    nv_attn_fwd_episode_bf16, then nv_attn_bwd_episode_bf16 (RoPE as the case says) and nv_attn_bwd_episode_acc_bf16 with
    accumulate = 0 and 1 (onto known fp32 values), RoPE the other way round.  Prefix rows and gap rows of out / dqkv, lse2 entries outside [lp, lp + n) and kv_acc rows >= lp are
    never written; RoPE^T at position lp + j."""
    g = gen(seed_of("episode", lps, ns, H, rope, dist))
    B, T = len(lps), len(ns)
    cu = [0] + list(np.cumsum(lps))
    Mp = cu[-1]
    Lp_max = max(lps)
    N_max = max(max(r) for r in ns)
    cap = max(lps[b] + ns[t][b] for t in range(T) for b in range(B)) + 5
    d = H * HD
    # the values, layout-free: prefix rows of sample b, rows of (step t, sample b), their dO
    xp = [make_rows(lp, H, dist, g) for lp in lps]
    xs = [[make_rows(ns[t][b], H, dist, g) for b in range(B)] for t in range(T)]
    if dist == "planted":
        for b in range(B):                                # one direction per sample: the prefix's last key and late keys of every step
            u = plant(xp[b], [lps[b] - 1], g)
            for t in range(T):
                plant(xs[t][b], plant_keys(ns[t][b]), g, u)
    xp = [x.to(BF) for x in xp]
    xs = [[x.to(BF) for x in r] for r in xs]
    dos = [[(torch.randn(ns[t][b], H, HD, generator=g, device=dev()) * 0.5).to(BF) for b in range(B)] for t in range(T)]
    cu_d = torch.tensor(cu, dtype=I32, device=dev())
    cos, sin = rope_tables(cap)

    def build(order, gap):
        off, R = _layout(lps, ns, order, gap)
        qkv = (torch.randn(R, 3 * d, generator=g, device=dev()) * 0.8).to(BF)   # gap rows: finite values no query may see
        dout = (torch.randn(R, d, generator=g, device=dev()) * 0.5).to(BF)
        for b in range(B):
            qkv[cu[b]:cu[b + 1]] = xp[b].reshape(lps[b], 3 * d)
            for t in range(T):
                n = ns[t][b]
                qkv[off[t, b]:off[t, b] + n] = xs[t][b].reshape(n, 3 * d)
                dout[off[t, b]:off[t, b] + n] = dos[t][b].reshape(n, d)
        tab = torch.tensor(np.concatenate([off.reshape(-1), np.array(ns, np.int64).reshape(-1)]).astype(np.int32), device=dev())
        return off, R, qkv, dout, tab

    def fwd(qkv, tab, R):
        out, lse = nans(R, d), nans(T, B, H, cap, dtype=F32)
        ptrs = torch.tensor([lse[t].data_ptr() for t in range(T)], dtype=torch.int64, device=dev())
        ok(L().nv_attn_fwd_episode_bf16(qkv.data_ptr(), out.data_ptr(), ptrs.data_ptr(), cu_d.data_ptr(), tab.data_ptr(), T, B, H, HD, cap,
                                        N_max, R, st()), "nv_attn_fwd_episode_bf16")
        return out, lse, ptrs

    offA, RA, qkvA, _, tabA = build("rev", 3)
    outA, lseA, _ = fwd(qkvA, tabA, RA)
    off, R, qkv, dout, tab = build("b", 0)
    out, lse, ptrs = fwd(qkv, tab, R)
    ws = torch.empty(max(R - Mp, 1) * H, dtype=F32, device=dev())
    runs = []
    for entry, accumulate, rot in (("bwd_episode", 0, rope), ("bwd_episode_acc", 0, not rope), ("bwd_episode_acc", 1, not rope)):
        dqkv, acc = nans(R, 3 * d), nans(B * cap, 2 * d, dtype=F32)
        base = torch.randn(B, cap, 2 * d, generator=g, device=dev())
        if accumulate:
            for b in range(B):
                acc.view(B, cap, -1)[b, :lps[b]] = base[b, :lps[b]]
        rc_, rs_ = (cos.data_ptr(), sin.data_ptr()) if rot else (None, None)
        args = (qkv.data_ptr(), out.data_ptr(), dout.data_ptr(), dqkv.data_ptr(), ws.data_ptr(), ptrs.data_ptr(), cu_d.data_ptr(),
                tab.data_ptr(), acc.data_ptr(), rc_, rs_, T, B, H, HD, cap, Mp, R, Lp_max, N_max)
        if entry == "bwd_episode":
            ok(L().nv_attn_bwd_episode_bf16(*args, st()), "nv_attn_bwd_episode_bf16")
        else:
            ok(L().nv_attn_bwd_episode_acc_bf16(*args, accumulate, st()), "nv_attn_bwd_episode_acc_bf16")
        runs.append((f"{entry} acc={accumulate} rope={rot}", accumulate, rot, dqkv, acc, base))
    torch.cuda.synchronize()

    # reference, step by step; the prefix keys' gradients summed over the steps
    acc_ref = [[torch.zeros(lps[b], H, HD, dtype=F64, device=dev()) for _ in range(4)] for b in range(B)]   # dK, dV, their magnitudes
    seenA = torch.zeros(RA, dtype=torch.bool, device=dev())
    seen = torch.zeros(R, dtype=torch.bool, device=dev())
    step_ref = {}
    many = [False] * B                                   # sample b has a step whose queries see more than two keys
    for t in range(T):
        for b in range(B):
            n, lp = ns[t][b], lps[b]
            if n == 0:
                continue
            tag = f"episode t={t} b={b} lp={lp} n={n}"
            q, k, v = split(xs[t][b].reshape(n, -1), H)
            _, kp_, vp_ = split(xp[b].reshape(lp, -1), H)
            j = torch.arange(n, device=dev())
            vis = torch.cat([torch.ones(n, lp, dtype=torch.bool, device=dev()), j[None, :] <= j[:, None]], 1)
            rows = slice(int(off[t, b]), int(off[t, b]) + n)
            dist_ = floor_dist(dist, vis)
            many[b] = many[b] or dist_ is not None
            r_out, r_lse, r_dq, r_dk, r_dv, mag = ref_attention(q, torch.cat([kp_, k]), torch.cat([vp_, v]), vis, dos[t][b],
                                                                out_in=out[rows].view(n, H, HD), lse2_in=lse[t, b][:, lp:lp + n])
            acc_ref[b][0] += r_dk[:lp]
            acc_ref[b][1] += r_dv[:lp]
            acc_ref[b][2] += mag["dk"][:lp]
            acc_ref[b][3] += mag["dv"][:lp]
            step_ref[t, b] = (r_dq, r_dk[lp:], r_dv[lp:], mag["dq"], mag["dk"][lp:], mag["dv"][lp:], dist_)
            for o_, l_, of_, sn_, nm in ((outA, lseA, offA, seenA, "fwd_episode gaps"), (out, lse, off, seen, "fwd_episode")):
                rows = slice(int(of_[t, b]), int(of_[t, b]) + n)
                check(f"{tag} {nm}", "out", o_[rows].view(n, H, HD), r_out, mag["out"], dist=dist_)
                check_lse(f"{tag} {nm}", l_[t, b][:, lp:lp + n], r_lse)
                all_nan(l_[t, b][:, :lp], f"{tag} {nm} lse2 below the step's positions")
                all_nan(l_[t, b][:, lp + n:], f"{tag} {nm} lse2 beyond the step's positions")
                sn_[rows] = True
        for l_, nm in ((lseA, "fwd_episode gaps"), (lse, "fwd_episode")):
            for b in range(B):
                if ns[t][b] == 0:
                    all_nan(l_[t, b], f"episode t={t} b={b} {nm}: lse2 of a step without rows")
    all_nan(outA[~seenA], "fwd_episode gaps: prefix and gap rows")
    all_nan(out[~seen], "fwd_episode: prefix rows")
    for name, accumulate, rot, dqkv, acc, base in runs:
        all_nan(dqkv[:Mp], f"{name}: dqkv prefix rows")
        for (t, b), (r_dq, r_dk, r_dv, m_dq, m_dk, m_dv, dist_) in step_ref.items():
            n, lp = ns[t][b], lps[b]
            pos = lp + torch.arange(n, device=dev())
            dq, dk, dv = parts(dqkv[int(off[t, b]):int(off[t, b]) + n], H)
            t2 = f"episode t={t} b={b} lp={lp} n={n} {name}"
            check(t2, "dq", dq, rope_t(r_dq, cos, sin, pos) if rot else r_dq, m_dq, dist=dist_)
            check(t2, "dk", dk, rope_t(r_dk, cos, sin, pos) if rot else r_dk, m_dk, dist=dist_)
            check(t2, "dv", dv, r_dv, m_dv, dist=dist_)
        a = acc.view(B, cap, 2, H, HD)
        for b in range(B):
            lp = lps[b]
            got = a[b, :lp] if not accumulate else a[b, :lp] - base[b, :lp].view(lp, 2, H, HD)
            check(f"episode b={b} lp={lp} {name}", "kv_dk", got[:, 0], acc_ref[b][0], acc_ref[b][2], dist=dist if many[b] else None)
            check(f"episode b={b} lp={lp} {name}", "kv_dv", got[:, 1], acc_ref[b][1], acc_ref[b][3], dist=dist if many[b] else None)
            all_nan(a[b, lp:], f"episode b={b} {name}: kv_acc rows >= prefix length")


# ====================================================================================== decode: one query row per sample
DECODE_CASES = [
    # cap, pos[r] (sample r attends its cache rows 0 .. pos[r]), H, values
    (64, [0, 1, 7, 8, 63], 2, "randn"),
    (256, [15, 16, 127, 128, 255, 31], 3, "peaked"),
    (1024, [511, 512, 1023, 64, 65, 700, 3, 640], 12, "randn"),
    (2100, [2047, 2048, 2099], 2, "peaked"),                  # more keys than one pass of the 16 waves covers (512 / 1024 per pass)
]


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("cap,pos,H,dist", DECODE_CASES, ids=[f"cap{c[0]}-M{len(c[1])}-H{c[2]}-{c[3]}" for c in DECODE_CASES])
def test_decode_vs_fp64(cap, pos, H, dist, hd):
    """nv_attn_decode_bf16: query r = the q slice of cache row crow[r] = r * cap + pos[r] against the keys / values of cache rows
    r * cap + [0, pos[r]], out [M, H * hd] compact.  Cache rows behind pos[r] hold NaN: they must not be read.  The `out` bound of the
    tile kernels holds a fortiori (fp32 probabilities, one bf16 rounding at the store).
    Worst measured on an MI355X (rel, max): 2.1e-3, 3.8e-3 at head_dim 64; 2.0e-3, 3.6e-3 at 128 (bound 6e-3, 1.0e-2)."""
    g = gen(seed_of("decode", cap, pos, H, dist, hd))
    M = len(pos)
    x = torch.randn(M, cap, 3, H, hd, generator=g, device=dev()) * 0.8
    if dist == "peaked":
        x[:, :, 0] *= 7.0
    for r in range(M):
        x[r, pos[r] + 1:] = NAN
    kv = x.reshape(M * cap, 3 * H * hd).to(BF).contiguous()
    pos_d = torch.tensor(pos, dtype=I32, device=dev())
    crow = torch.tensor([r * cap + pos[r] for r in range(M)], dtype=I32, device=dev())
    out = nans(M, H * hd)
    ok(L().nv_attn_decode_bf16(kv.data_ptr(), crow.data_ptr(), pos_d.data_ptr(), out.data_ptr(), M, H, hd, cap, st()), "nv_attn_decode_bf16")
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all(), "decode: non-finite output"
    b_rel, b_max = BOUND["out"]
    for r in range(M):
        rows = kv.view(M, cap, 3, H, hd)[r, :pos[r] + 1].double()
        q, k, v = rows[-1, 0], rows[:, 1], rows[:, 2]                       # [H, hd], [n, H, hd]
        p = torch.softmax(torch.einsum("hd,nhd->hn", q, k) * hd ** -0.5, dim=1)
        ref, mag = torch.einsum("hn,nhd->hd", p, v), torch.einsum("hn,nhd->hd", p, v.abs())
        err = out[r].view(H, hd).double() - ref
        rn = torch.maximum(ref.norm(dim=1), mag.norm(dim=1) / MAG_FLOOR)
        rmax = torch.maximum(ref.abs().amax(dim=1), mag.abs().amax(dim=1) / MAG_FLOOR)
        rel, mx = (err.norm(dim=1) / rn).max().item(), (err.abs().amax(dim=1) / rmax).max().item()
        print(f"ATTNREF64 decode hd={hd} rel={rel:.3e} max={mx:.3e} r={r} pos={pos[r]}")
        assert rel <= b_rel and mx <= b_max, f"decode hd={hd} r={r} pos={pos[r]}: rel {rel:.3e} (bound {b_rel:.1e}), max {mx:.3e} (bound {b_max:.1e})"
