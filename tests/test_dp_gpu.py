"""The data-parallel wrapper on real GPUs.

World of one (the test box has a single MI355X): RCCL collectives on the flat gradient slices are launched from inside the
backward on the communication stream and joined at the end of the autograd pass.  With one rank every collective is the
identity, so the gradients must equal the plain run's bit for bit -- what this checks is the stream/event/callback wiring
under the real runtime, for both transports (the C-ABI nv_comm_* default and torch.distributed/nccl), both reduction points
(`step`: once, from the final backward or from the optimizer's flush; `backward`: DDP's) and both algorithms.

World of two (runs when the box has >= 2 GPUs): two real ranks, real `LlamaStack.backward`, gradients must equal the mean of
the two single-rank gradients (tools/optims.py:52-54, mp3d_agent.py:661-676)."""
import os
import socket

import pytest
import torch
import torch.distributed as dist

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _cfg():
    from navillm_amd import config as nvcfg
    return nvcfg.NavConfig(hidden_size=512, num_layers=3, num_heads=4, intermediate_size=1408, base_vocab_size=1000,
                           enc_hidden_size=256, enc_num_heads=4, enc_intermediate_size=512, image_feat_size=768)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _step(model, wrapped, seed, dev=DEV, final=True):
    from navillm_amd.synthetic import SyntheticEpisodes, nav_step
    from navillm_amd.losses import CrossEntropyLoss
    ep = SyntheticEpisodes(model.cfg, 3, seed=seed, instr_len=150, device=torch.device(dev))
    crit = CrossEntropyLoss()
    model.zero_grad()
    torch.manual_seed(1)
    for i in range(2):
        nav_step(wrapped, crit, ep, train=True, last=(i == 1), final=final and i == 1)   # step 0 inside no_sync
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in model.store.grad.items()}


@pytest.mark.parametrize("transport,reduce,algo", [("rccl", "step", "rs_ag"), ("rccl", "step", "allreduce"),
                                                   ("rccl", "backward", "rs_ag"), ("torch", "step", "allreduce"),
                                                   ("rccl", "flush", "rs_ag")])
def test_dp_wrapper_world1_matches_plain_run(transport, reduce, algo, monkeypatch):
    from navillm_amd.nav_model import NavModel
    from navillm_amd.parallel import NavDataParallel, RcclComm
    from navillm_amd.optim import FlatAdamW
    model = NavModel(nav_config=_cfg(), device=torch.device(DEV), seed=4)
    model.train()
    base = _step(model, model, 17)
    comm = None
    if transport == "torch":
        monkeypatch.setenv("NAVILLM_COMM", "torch")
        if not dist.is_initialized():
            dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{_free_port()}", world_size=1, rank=0,
                                    device_id=torch.device(DEV))
    else:
        comm = RcclComm(0, 1)
    flush = reduce == "flush"
    ddp = NavDataParallel(model, comm=comm, force_sync=True, reduce="step" if flush else reduce, algo=algo)
    assert (ddp.comm is None) == (transport == "torch")
    # the back-reference must not register the wrapper as a child of the model it wraps
    ddp.train(); model.train(); model.state_dict(); ddp.state_dict()
    ddp.profile = True                           # round 5: HIP events around every slice's collective and around the join (bench.py `dp.exchange`)
    got = _step(model, ddp, 17, final=not flush)
    if flush:
        assert ddp._pending                      # nothing exchanged yet: the optimizer's flush does it, once
        opt = FlatAdamW(model, lr=0.0)
        opt.clip_grad_norm_(40.0)
        torch.cuda.synchronize()
        got = {k: v.clone() for k, v in model.store.grad.items()}
    assert not ddp._pending
    xs = ddp.exchange_stats()
    n_slices = model.cfg.num_layers + 3          # one per decoder layer + embeddings | norm + heads | the fp32 group
    total_bytes = sum(t.numel() * t.element_size() for t in ddp.slices.all_slices())
    assert xs is not None and xs["exchanges"] == 1 and xs["slices_per_exchange"] == n_slices and xs["bytes_per_exchange"] == total_bytes, xs
    assert xs["collective_busy_ms_per_exchange"] > 0 and xs["exposed_ms_per_exchange"] >= 0, xs
    assert ddp.exchange_stats() is None          # (reset)
    object.__setattr__(model, "_dp", None)
    for k in base:
        assert torch.equal(base[k], got[k]), f"{transport}/{reduce}/{algo}: gradient buffer {k} differs from the plain run"
    assert float(base["lm"].float().abs().sum()) > 0
    if comm is not None:
        comm.close()


def test_comm_init_checks_rccl_version_and_enum_values():
    """the rccl.h constants restated in comm_rccl.hip are verified against the librccl that was bound:
    nv_comm_init runs a mean all-reduce of known bf16 / fp32 vectors and fails unless the values come back right."""
    from navillm_amd import lib as L
    from navillm_amd.parallel import RcclComm
    v = L.load().nv_comm_rccl_version()
    assert 20000 <= v < 30000, v
    comm = RcclComm(0, 1)                    # raises if the self-check inside nv_comm_init fails
    t = torch.tensor([1.0, 3.0, -2.5, 12.0] * 16, dtype=torch.bfloat16, device=DEV)
    want = t.clone()
    comm.allreduce_mean_(t)
    comm.reduce_scatter_all_gather_mean_(t)
    torch.cuda.synchronize()
    assert torch.equal(t, want)
    comm.close()


def _rank_main(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    from navillm_amd.nav_model import NavModel
    from navillm_amd.parallel import init_distributed_device, NavDataParallel
    dev, r, w = init_distributed_device()
    model = NavModel(nav_config=_cfg(), device=dev, seed=4 + rank)       # rank-dependent weights: the wrapper broadcasts rank 0's
    model.train()
    ddp = NavDataParallel(model)
    cal = ddp.calibrate(iters=1)
    p0 = {k: v.clone().cpu() for k, v in model.store.param.items()}
    g = _step(model, ddp, 100 + rank, dev=str(dev))
    pack = lambda d: {k: v.detach().cpu().float().numpy() for k, v in d.items()}      # by value: shared-memory handles die with the rank
    q.put((rank, pack(g), pack(p0), cal))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs")
def test_dp_world2_real_backward_matches_mean_of_single_rank_gradients():
    import torch.multiprocessing as mp
    from navillm_amd.nav_model import NavModel
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_main, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=600) for _ in range(world)], key=lambda t: t[0])
    for p in procs:
        p.join(120)
    unpack = lambda d: {k: torch.from_numpy(v) for k, v in d.items()}
    (_, g0, p0, cal0), (_, g1, p1, _) = [(r_[0], unpack(r_[1]), unpack(r_[2]), r_[3]) for r_ in res]
    for k in g0:
        assert torch.equal(p0[k], p1[k]), "parameters were not broadcast from rank 0"
        assert torch.equal(g0[k], g1[k]), "ranks disagree on the averaged gradient"
    assert cal0 is not None and cal0["chosen"] in ("rs_ag", "allreduce")
    # reference: the two ranks' batches on ONE GPU with rank 0's weights, averaged
    model = NavModel(nav_config=_cfg(), device=torch.device(DEV), seed=4)
    model.train()
    a = _step(model, model, 100)
    b = _step(model, model, 101)
    for k in a:
        want = (a[k].float() + b[k].float()) * 0.5
        got = g0[k].float().to(want.device)
        err = (got - want).abs().max().item()
        scale = want.abs().max().item()
        assert err <= 0.01 * scale + 1e-6, (k, err, scale)


def _episode(model, wrapped, seed, with_objects, dev=DEV, final_overlap=True):
    """two nav steps (step 0 inside no_sync) and, when `with_objects`, an object-grounding backward in between -- the rank
    whose batch carries objects is the only one whose `obj_projector` / `og_head` get a LOCAL gradient"""
    from navillm_amd.synthetic import SyntheticEpisodes, nav_step, og_step
    from navillm_amd.losses import CrossEntropyLoss
    ep = SyntheticEpisodes(model.cfg, 3, seed=seed, instr_len=150, device=torch.device(dev), task="reverie" if with_objects else "r2r")
    crit = CrossEntropyLoss()
    model.zero_grad()
    torch.manual_seed(1)
    nav_step(wrapped, crit, ep, train=True, last=False)
    if with_objects:
        og_step(wrapped, crit, ep, train=True, sync="plain")
    nav_step(wrapped, crit, ep, train=True, last=True, final=final_overlap)
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in model.store.grad.items()}


def _shared_gpu_rank(rank, world, port, q, reduce, final_overlap):
    """both ranks on GPU 0, torch.distributed on gloo, the exchange staged through the host (two ranks cannot form an RCCL
    communicator on one device): everything of the N > 1 path except RCCL itself, with the REAL kernels"""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0",
                      NAVILLM_COMM="torch")
    from navillm_amd.nav_model import NavModel
    from navillm_amd.parallel import init_distributed_device, NavDataParallel
    from navillm_amd.optim import FlatAdamW
    dev, r, w = init_distributed_device(backend="gloo", device_index=0)
    assert (r, w) == (rank, world)
    model = NavModel(nav_config=_cfg(), device=dev, seed=4 + rank)       # rank-dependent weights: the wrapper broadcasts rank 0's
    model.train()
    ddp = NavDataParallel(model, reduce=reduce)
    assert ddp.comm is None
    p0 = {k: v.clone().cpu() for k, v in model.store.param.items()}
    # reduce="backward" is DDP's semantics: every synced backward is a collective, so (as under the reference's task-id
    # broadcast, tasks/loaders.py:176-179) both ranks must run the same sub-tasks; reduce="step" only accumulates locally
    g = _episode(model, ddp, 100 + rank, with_objects=(rank == 1 or reduce == "backward"), dev=str(dev), final_overlap=final_overlap)
    pending = ddp._pending
    opt = FlatAdamW(model, lr=1e-3)
    opt.clip_grad_norm_(40.0)                # reduce="step" without a flagged final backward: the flush exchanges here
    torch.cuda.synchronize()
    g_after = {k: v.clone().cpu() for k, v in model.store.grad.items()}
    opt.step()
    torch.cuda.synchronize()
    p1 = {k: v.clone().cpu() for k, v in model.store.param.items()}
    # by VALUE (numpy, bf16 widened exactly to fp32): torch tensors would travel as shared-memory handles that die with this process
    pack = lambda d: {k: v.detach().cpu().float().numpy() for k, v in d.items()}
    q.put((rank, pack(g), pack(g_after), pack(p0), pack(p1), dict(opt.born), pending))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("reduce,final_overlap", [("step", True), ("step", False), ("backward", True)])
def test_dp_world2_shared_gpu_real_backward_mean_and_replica_consistency(reduce, final_overlap):
    """VERDICT r2 missing #1: an N > 1 gradient mean through the REAL backward.  Two ranks, different episode seeds, rank 1's
    batch carries objects (rank 0's does not): after the exchange both ranks hold the same gradients == the mean of the two
    single-rank gradients (tools/optims.py:52-54, mp3d_agent.py:661-676); after clip + AdamW both replicas are bit-identical,
    including `obj_projector`, which (reduce="step") only rank 1 touched locally (DDP find_unused_parameters semantics)."""
    import torch.multiprocessing as mp
    from navillm_amd.nav_model import NavModel
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_shared_gpu_rank, args=(r, world, port, q, reduce, final_overlap)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=900) for _ in range(world)], key=lambda t: t[0])
    for p in procs:
        p.join(120)
    unpack = lambda d: {k: torch.from_numpy(v) for k, v in d.items()}
    (_, g0, ga0, p00, p10, born0, pend0), (_, g1, ga1, p01, p11, born1, pend1) = \
        [(r_[0],) + tuple(unpack(x) for x in r_[1:5]) + tuple(r_[5:]) for r_ in res]
    # the reference: both ranks' episodes on ONE model holding rank 0's weights, averaged on the host in fp32
    model = NavModel(nav_config=_cfg(), device=torch.device(DEV), seed=4)
    model.train()
    for k in p00:
        assert torch.equal(p00[k], p01[k]), "parameters were not broadcast from rank 0"
        assert torch.equal(p00[k], model.store.param[k].cpu().float())
    a = _episode(model, model, 100, with_objects=(reduce == "backward"))
    b = _episode(model, model, 101, with_objects=True)
    if reduce == "step" and not final_overlap:
        assert pend0 and pend1                   # nothing was exchanged inside the backwards; clip_grad_norm_'s flush did it
        g0, g1 = ga0, ga1
    else:
        assert not pend0 and not pend1
        for k in g0:
            assert torch.equal(g0[k], ga0[k]), "the flush averaged a second time"
    for k in a:
        assert torch.equal(g0[k], g1[k]), f"ranks disagree on the averaged gradient buffer {k}"
        want = (a[k].float() + b[k].float()).cpu() * 0.5
        got = g0[k].float()
        if reduce == "backward":
            # DDP semantics: the og backward of rank 1 was a synced one too, so the mean was taken twice over partial sums; equal
            # in exact arithmetic, one more bf16 rounding per element here
            tol = 0.02
        else:
            tol = 0.01
        err = (got - want).abs().max().item()
        scale = want.abs().max().item()
        assert err <= tol * scale + 1e-6, (k, err, scale)
        # and the mean is a real mean: it differs from either rank's own gradient
        assert (got - a[k].float().cpu()).abs().max().item() > 1e-3 * scale
    assert born0 == born1
    obj = [n for n in born0 if "obj_projector" in n]
    assert obj, "obj_projector must be updated on both ranks although only rank 1 saw objects"
    for k in p10:
        assert torch.equal(p10[k], p11[k]), f"replicas diverged after the optimizer step ({k})"
    st = model.store
    n = obj[0]
    o, sz = st.offsets[n], st.sizes[n]
    assert not torch.equal(p10["f32"][o:o + sz], p00["f32"][o:o + sz]), "obj_projector did not move on rank 0"


def test_two_rank_rehearsal_on_one_gpu_prints_one_n2_line():
    """The N > 1 control flow of bench.py with REAL kernels on a box with one GPU (NAVILLM_BENCH_REHEARSAL=1: both ranks share
    GPU 0, torch.distributed on gloo, the gradient exchange staged through the host): `--gpus 2` without a torchrun environment
    relaunches itself under torch.distributed.run, both ranks build the model, wrap it in NavDataParallel, run warmup + timed steps
    incl. the exchange from inside the episode's last backward, agree on the max-over-ranks clock -- and stdout carries exactly ONE
    JSON line with n_gpus = 2, marked as a rehearsal."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, NAVILLM_BENCH_REHEARSAL="1", NAVILLM_BUILD_REUSE="1")
    env.pop("WORLD_SIZE", None); env.pop("RANK", None); env.pop("LOCAL_RANK", None)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--model", "tiny", "--steps", "7", "--warmup", "1",
                        "--prewarm", "1", "--instr-len", "40", "--batch", "2", "--no-cpu-baseline", "--infer-steps", "0", "--full"],
                       capture_output=True, text=True, timeout=600, env=env, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 7 and d["value"] > 0 and "rehearsal" in d
    assert d["config"]["parallelism"] == "dp2" and d["dp"]["reduce"] == "step"
    # K = 7: episodes of 6 + 1 steps, the last timed step closes its episode; then both ranks run the whole-episode window and the
    # other training mode (each with its own exchanges) and still agree on one line
    assert "6 + 1" in d["config"]["timed_window"] and d["whole_episodes"]["steps"] == 18 and d["whole_episodes"]["nav_steps_per_s"] > 0
    assert d["other_mode"]["mode"] == "recompute" and d["other_mode"].get("nav_steps_per_s_per_gpu", 0) > 0, d["other_mode"]


def _prefix_episode(model, wrapped, seed, steps, dev=DEV, teacher_forced=False):
    """one prefix-reuse training episode (navillm_amd/episode.py, the bench's default mode): every step's backward() only records its
    output gradient; ALL gradients of the episode appear in finish_episode(), which under the wrapper runs inside `final_backward()`
    and launches the per-layer exchange from the deferred backward walk"""
    from navillm_amd.synthetic import SyntheticEpisodes, prefix_reuse_episode, accumulation_window
    from navillm_amd.losses import CrossEntropyLoss
    ep = SyntheticEpisodes(model.cfg, 3, seed=seed, instr_len=150, device=torch.device(dev))
    model.zero_grad()
    torch.manual_seed(1)
    if teacher_forced == "auto":
        # round 6: AUTOMATIC episode -- the rollout makes no begin_episode / finish_episode call (synthetic.reference_rollout = the
        # reference's loop); its deferred work runs when the gradients are handed over -- by the optimizer's clip / step, which under the
        # wrapper runs it inside final_backward() by itself, so that the per-layer exchange is launched from the deferred backward walk
        from navillm_amd.synthetic import reference_rollout
        model.auto_episode, model.auto_form = True, "lazy"
        reference_rollout(wrapped, CrossEntropyLoss(), ep, steps)
        assert model._auto_open
        model.grad_handover("optimizer")          # (what FlatAdamW.clip_grad_norm_ / step call first: under a wrapper it runs inside final_backward())
        model.auto_episode = False
    elif teacher_forced == "window":
        # round 5: an accumulation window of two teacher-forced episodes (begin_episode(..., accumulate=2)); the second finish_episode()
        # runs the whole window inside final_backward()
        ep_b = SyntheticEpisodes(model.cfg, 3, seed=seed + 50, instr_len=110, device=torch.device(dev))
        accumulation_window(wrapped, CrossEntropyLoss(), [ep, ep_b], [steps, max(steps - 1, 1)])
    else:
        prefix_reuse_episode(wrapped, CrossEntropyLoss(), ep, steps, teacher_forced=teacher_forced)
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in model.store.grad.items()}


def _shared_gpu_rank_prefix(rank, world, port, q, steps_by_rank, teacher_forced=False):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0",
                      NAVILLM_COMM="torch")
    from navillm_amd.nav_model import NavModel
    from navillm_amd.parallel import init_distributed_device, NavDataParallel
    from navillm_amd.optim import FlatAdamW
    dev, r, w = init_distributed_device(backend="gloo", device_index=0)
    model = NavModel(nav_config=_cfg(), device=dev, seed=4 + rank)
    model.train()
    ddp = NavDataParallel(model, reduce="step")
    p0 = {k: v.clone().cpu() for k, v in model.store.param.items()}
    g = _prefix_episode(model, ddp, 100 + rank, steps_by_rank[rank], dev=str(dev), teacher_forced=teacher_forced)
    pending = ddp._pending
    opt = FlatAdamW(model, lr=1e-3)
    opt.clip_grad_norm_(40.0)
    torch.cuda.synchronize()
    g_after = {k: v.clone().cpu() for k, v in model.store.grad.items()}
    opt.step()
    torch.cuda.synchronize()
    p1 = {k: v.clone().cpu() for k, v in model.store.param.items()}
    pack = lambda d: {k: v.detach().cpu().float().numpy() for k, v in d.items()}
    q.put((rank, pack(g), pack(g_after), pack(p0), pack(p1), pending))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("teacher_forced", [False, True, "window", "auto"])
def test_dp_world2_shared_gpu_prefix_reuse_episode_mean_and_replica_consistency(teacher_forced):
    """the HEADLINE training mode under data parallelism with two real ranks and the real kernels.  Rank 0 runs a
    2-step episode, rank 1 a 3-step one (ranks may run different numbers of nav steps, mp3d_agent.py:661-676: only the final backward
    synchronises); the exchange is launched from inside finish_episode()'s deferred backward walk under final_backward().  After it both
    ranks hold bit-identical gradients == the mean of the two single-rank prefix-reuse gradients, nothing is left for the optimizer's
    flush, and after clip + AdamW the replicas are bit-identical.  teacher_forced: the same with the steps' forward deferred and batched
    into finish_episode() (round 4), i.e. the bench's default training step under data parallelism.  "window" (round 5): each rank runs
    an accumulation window of two teacher-forced episodes; the exchange runs from inside the window's batched backward.  "auto" (round
    6): the unmodified rollout, automatic episodes, the handover inside final_backward()."""
    import torch.multiprocessing as mp
    from navillm_amd.nav_model import NavModel
    world, steps_by_rank = 2, (2, 3)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_shared_gpu_rank_prefix, args=(r, world, port, q, steps_by_rank, teacher_forced)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=900) for _ in range(world)], key=lambda t: t[0])
    for p in procs:
        p.join(120)
    unpack = lambda d: {k: torch.from_numpy(v) for k, v in d.items()}
    (_, g0, ga0, p00, p10, pend0), (_, g1, ga1, p01, p11, pend1) = [(r_[0],) + tuple(unpack(x) for x in r_[1:5]) + (r_[5],) for r_ in res]
    model = NavModel(nav_config=_cfg(), device=torch.device(DEV), seed=4)
    model.train()
    a = _prefix_episode(model, model, 100, steps_by_rank[0], teacher_forced=teacher_forced)
    b = _prefix_episode(model, model, 101, steps_by_rank[1], teacher_forced=teacher_forced)
    assert not pend0 and not pend1, "the exchange must have run from inside finish_episode() (final_backward), not be left to the flush"
    for k in a:
        assert torch.equal(p00[k], p01[k]), "parameters were not broadcast from rank 0"
        assert torch.equal(g0[k], g1[k]), f"ranks disagree on the averaged gradient buffer {k}"
        assert torch.equal(g0[k], ga0[k]) and torch.equal(g1[k], ga1[k]), "the optimizer's flush averaged a second time"
        want = (a[k].float() + b[k].float()).cpu() * 0.5
        got = g0[k].float()
        err, scale = (got - want).abs().max().item(), want.abs().max().item()
        assert err <= 0.01 * scale + 1e-6, (k, err, scale)
        assert (got - a[k].float().cpu()).abs().max().item() > 1e-3 * scale      # a real mean, not rank 0's own gradient
    for k in p10:
        assert torch.equal(p10[k], p11[k]), f"replicas diverged after the optimizer step ({k})"
        assert not torch.equal(p10[k], p00[k])
