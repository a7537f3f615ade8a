"""The three AdamW update kernels of the LM group on one 2^28-element buffer: ms per launch (HIP events, median) and achieved GB/s.

    python tools/adamw_modes_bench.py [--log2n 28] [--reps 15] [--warmup 3]

"bf16" is nv_adamw_zero_grad (the reference-exact default, the yardstick), "fp32_master" nv_adamw_master, "stochastic" nv_adamw_sr, all
with the gradient zeroed as it is consumed (FlatAdamW's default).  Bytes per element, counted from the kernels' accesses:
    bf16, stochastic   read p, g, m, v (8)  + write p, m, v (6)  + zero g (2)                  = 16
    fp32_master        read p, g (4) + master, m, v (12)  + write p (2) + master, m, v (12) + zero g (2) = 32
The modes alternate inside one loop (the same clock and neighbours for all three) and the gradient is refilled with the same random
values before every launch, outside the timed window.  Needs a GPU; prints one line per mode and one JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from navillm_amd import ops  # noqa: E402

BYTES = {"bf16": 16, "fp32_master": 32, "stochastic": 16}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=28)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("adamw_modes_bench: no GPU (a timing from anything else would mean nothing)")
    dev, n = torch.device("cuda:0"), 1 << a.log2n
    gen = torch.Generator(device=dev).manual_seed(0)
    bf = lambda scale: (torch.randn(n, generator=gen, device=dev) * scale).to(torch.bfloat16)
    g0 = bf(1e-3)
    g = g0.clone()
    clip = torch.tensor([1.0, 0.37], dtype=torch.float32, device=dev)
    st = {}
    for mode in BYTES:
        dt = torch.float32 if mode == "fp32_master" else torch.bfloat16
        st[mode] = dict(p=bf(0.02), m=torch.zeros(n, dtype=dt, device=dev), v=torch.zeros(n, dtype=dt, device=dev))
    st["fp32_master"]["w"] = torch.zeros(n, dtype=torch.float32, device=dev)
    h = dict(lr=1e-5, wd=0.01, clip=clip, zero_grad=True)

    def launch(mode, step):
        s = st[mode]
        if mode == "bf16":
            ops.adamw_(s["p"], g, s["m"], s["v"], step, **h)
        elif mode == "fp32_master":
            ops.adamw_master_(s["p"], g, s["w"], s["m"], s["v"], step, **h)
        else:
            ops.adamw_sr_(s["p"], g, s["m"], s["v"], step, elem0=0, seed=0, **h)

    ms = {mode: [] for mode in BYTES}
    for rep in range(a.warmup + a.reps):
        for mode in BYTES:
            g.copy_(g0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            launch(mode, rep + 1)
            e1.record()
            e1.synchronize()
            if rep >= a.warmup:
                ms[mode].append(e0.elapsed_time(e1))
    assert not g.any()
    out = {"n": n, "reps": a.reps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "modes": {}}
    base = None
    for mode in BYTES:
        med = statistics.median(ms[mode])
        gbs = BYTES[mode] * n / (med * 1e-3) / 1e9
        base = base or (med, gbs)
        out["modes"][mode] = {"ms_median": round(med, 4), "ms_min": round(min(ms[mode]), 4), "ms_max": round(max(ms[mode]), 4),
                              "bytes_per_element": BYTES[mode], "GBps": round(gbs, 1), "time_vs_bf16": round(med / base[0], 3),
                              "bandwidth_vs_bf16": round(gbs / base[1], 3)}
        print(f"{mode:12s} {med:8.3f} ms (min {min(ms[mode]):.3f}, max {max(ms[mode]):.3f}; median of {a.reps})  {BYTES[mode]:2d} B/element  "
              f"{gbs:7.1f} GB/s  time x{med / base[0]:.2f}  bandwidth x{gbs / base[1]:.2f} of the bf16 kernel", file=sys.stderr)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
