"""GPU, `tiny` configuration: the AdamW state-precision modes through NavModel + FlatAdamW -- 30 optimizer steps on one fixed synthetic
navigation batch per mode, with and without the overlapped update, interrupted by a save / load at step 15; state dicts of another
precision and of the reference's format; the fp8 deployment releasing the master; two data-parallel ranks rounding identically."""
import os
import socket

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = ("fp32_master", "stochastic")
LR = 1e-4
STEPS, HALF = 30, 15


def _model(seed=3):
    from navillm_amd import config as C
    from navillm_amd.nav_model import NavModel
    m = NavModel(nav_config=C.tiny(), device=torch.device(DEV), seed=seed)
    m.eval()                                           # dropout off: the batch and the weights determine every gradient
    return m


def _train(model, opt, steps, ep_seed=9, wrapped=None):
    """`steps` optimizer steps, each on the same freshly built synthetic batch"""
    from navillm_amd.losses import CrossEntropyLoss
    from navillm_amd.synthetic import SyntheticEpisodes, nav_step
    crit = CrossEntropyLoss()
    for _ in range(steps):
        ep = SyntheticEpisodes(model.cfg, 2, seed=ep_seed, instr_len=40, n_views=8, device=model.device)
        torch.manual_seed(1)
        nav_step(wrapped or model, crit, ep, train=True, last=True)
        opt.clip_grad_norm_(40.0)
        opt.step()
        opt.zero_grad()
    torch.cuda.synchronize()


def _snap(model):
    st = model.store
    model.store.wait_params()
    torch.cuda.synchronize()
    out = {f"param/{g}": t.clone() for g, t in st.param.items()}
    out.update({f"exp_avg/{g}": t.clone() for g, t in st.exp_avg.items()})
    out.update({f"exp_avg_sq/{g}": t.clone() for g, t in st.exp_avg_sq.items()})
    if st.master is not None:
        out["master/lm"] = st.master["lm"].clone()
    return out


def _same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        x, y = a[k].contiguous(), b[k].contiguous()
        assert x.dtype == y.dtype and torch.equal(x.view(torch.uint8), y.view(torch.uint8)), f"{what}: {k} differs"


_runs = {}


def _uninterrupted(mode):
    """30 steps without the overlapped update -> (snapshot at 30, model and optimizer state dicts at 15, snapshot at 0); once per mode"""
    from navillm_amd.optim import FlatAdamW
    if mode not in _runs:
        m = _model()
        opt = FlatAdamW(m, lr=LR, state_precision=mode, sr_seed=21)
        opt.overlap_update = False
        start = _snap(m)
        _train(m, opt, HALF)
        saved = ({k: v.clone() for k, v in m.state_dict().items()}, opt.state_dict())
        _train(m, opt, STEPS - HALF)
        _runs[mode] = (_snap(m), saved, start)
    return _runs[mode]


@pytest.mark.parametrize("mode", MODES)
def test_thirty_steps_train_the_model(mode):
    end, _, start = _uninterrupted(mode)
    for g in ("lm", "f32"):
        assert torch.isfinite(end[f"param/{g}"].float()).all() and not torch.equal(end[f"param/{g}"], start[f"param/{g}"])
    assert end["exp_avg/lm"].dtype == (torch.float32 if mode == "fp32_master" else torch.bfloat16)
    if mode == "fp32_master":
        w, p = end["master/lm"], end["param/lm"]
        upd = w != 0                                   # updated segments (tensors that never had a gradient keep a zero master)
        assert upd.float().mean() > 0.5 and torch.equal(w.to(torch.bfloat16)[upd], p[upd])
        assert (w[upd] != p[upd].float()).float().mean() > 0.5          # the master holds more than the bf16 parameter


@pytest.mark.parametrize("mode", MODES)
def test_overlapped_update_is_bit_identical(mode):
    from navillm_amd.optim import FlatAdamW
    m = _model()
    opt = FlatAdamW(m, lr=LR, state_precision=mode, sr_seed=21)
    opt.overlap_update = True                          # the LM group on the side stream, cut at the decoder layers' boundaries
    _train(m, opt, STEPS)
    _same(_snap(m), _uninterrupted(mode)[0], f"{mode}: overlap_update on vs off")


@pytest.mark.parametrize("mode", MODES)
def test_save_at_15_load_and_continue_is_bit_identical(mode):
    from navillm_amd.optim import FlatAdamW
    end, (model_sd, opt_sd), _ = _uninterrupted(mode)
    assert opt_sd["state_precision"] == mode and opt_sd["sr_seed"] == 21 and ("master" in opt_sd) == (mode == "fp32_master")
    m = _model(seed=8)                                 # other weights, other optimizer seed: everything must come from the two state dicts
    opt = FlatAdamW(m, lr=1.0, state_precision=mode, sr_seed=0)
    opt.overlap_update = False
    m.load_state_dict(model_sd)
    opt.load_state_dict(opt_sd)
    assert opt.step_count == HALF and opt.sr_seed == 21 and abs(opt.lr - LR) < 1e-15
    _train(m, opt, STEPS - HALF)
    _same(_snap(m), end, f"{mode}: resumed at step {HALF}")


def test_states_of_other_precision_and_reference_format_load_and_continue():
    from navillm_amd.optim import FlatAdamW
    src = _model()
    o = FlatAdamW(src, lr=LR)
    assert o.state_precision == "bf16" and src.store.exp_avg["lm"].dtype == torch.bfloat16
    _train(src, o, 3)
    model_sd = {k: v.clone() for k, v in src.state_dict().items()}
    flat_sd, ref_sd = o.state_dict(), o.reference_state_dict()
    for mode, sd in (("fp32_master", flat_sd), ("fp32_master", ref_sd), ("stochastic", ref_sd), ("bf16", ref_sd)):
        m = _model(seed=8)
        m.load_state_dict(model_sd)
        opt = FlatAdamW(m, lr=LR, state_precision=mode)
        opt.load_state_dict(sd)
        torch.cuda.synchronize()
        assert opt.step_count == 3 and opt.born == o.born
        dt = torch.float32 if mode == "fp32_master" else torch.bfloat16
        for key in ("exp_avg", "exp_avg_sq"):
            got, want = getattr(m.store, key), getattr(src.store, key)
            assert got["lm"].dtype == dt and torch.equal(got["lm"], want["lm"].to(dt)), (mode, key)      # the upcast values
            assert torch.equal(got["f32"], want["f32"])
        before = m.store.param["lm"].clone()
        _train(m, opt, 2)
        assert opt.step_count == 5 and torch.isfinite(m.store.param["lm"].float()).all() and not torch.equal(before, m.store.param["lm"])
        if mode == "fp32_master":                      # no master in either state: adopted from the loaded parameters
            w, p = m.store.master["lm"], m.store.param["lm"]
            assert torch.equal(w.to(torch.bfloat16)[w != 0], p[w != 0]) and (w != 0).float().mean() > 0.5


def test_fp8_deployment_releases_the_master():
    from navillm_amd.optim import FlatAdamW
    m = _model()
    opt = FlatAdamW(m, lr=LR, state_precision="fp32_master")
    _train(m, opt, 1)
    assert m.store.master["lm"].dtype == torch.float32 and m.store.master["lm"].any()
    m.to_fp8_weight_only()
    assert m.store.master is None and m.store.exp_avg is None and m.store.exp_avg_sq is None and m.store.grad is None


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _stochastic_rank(rank, world, port, q):
    """both ranks on GPU 0, torch.distributed on gloo (tests/test_dp_gpu.py::_shared_gpu_rank): different batches per rank, three
    optimizer steps in "stochastic" mode"""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0",
                      NAVILLM_COMM="torch", NAVILLM_AUTO_EPISODE="0")
    import torch.distributed as dist
    from navillm_amd import config as C
    from navillm_amd.nav_model import NavModel
    from navillm_amd.parallel import init_distributed_device, NavDataParallel
    from navillm_amd.optim import FlatAdamW
    dev, r, w = init_distributed_device(backend="gloo", device_index=0)
    model = NavModel(nav_config=C.tiny(), device=dev, seed=4 + rank)        # rank-dependent weights: the wrapper broadcasts rank 0's
    model.eval()
    ddp = NavDataParallel(model, reduce="step")
    opt = FlatAdamW(model, lr=LR, state_precision="stochastic")
    p0 = model.store.param["lm"].clone()
    _train(model, opt, 3, ep_seed=100 + rank, wrapped=ddp)
    moved = float((model.store.param["lm"] != p0).float().mean())
    pack = lambda d: {k: v.detach().cpu().float().numpy() for k, v in d.items()}          # by value: shared-memory handles die with the rank
    q.put((rank, pack(_snap(model)), moved))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_round_identically_in_stochastic_mode():
    """the Philox key is the optimizer's `sr_seed`, not torch's generator: after 3 steps on different batches both replicas hold
    bit-identical parameters and moments (bf16 widened exactly to fp32 for the trip through the queue)"""
    import numpy as np
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_stochastic_rank, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=600) for _ in range(2)], key=lambda t: t[0])
    for p in procs:
        p.join(120)
    (_, a, moved0), (_, b, moved1) = res
    assert moved0 > 0.2 and moved0 == moved1
    for k in a:
        assert np.array_equal(a[k], b[k]), f"replicas diverged in {k}"
