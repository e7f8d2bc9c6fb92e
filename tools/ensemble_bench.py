#!/usr/bin/env python3
"""What the flip / rotate self-ensemble costs beyond its K forwards.

At the evaluation shape B = 4 imagesets of V = 32 views of 128 x 128 (x3: 384 x 384 SR), K = 8 members, in bf16 and in bf16x3, this
times in ONE process, alternating round by round after a warm-up, with device events around `reps` back-to-back calls:

    ensemble      HRNet.forward_ensemble(lrs, alphas, "dihedral")            expand + one forward of K*B samples + mean
    forward(K*B)  the plain forward on a batch of K*B = 32 samples            unchanged code: the yardstick
    expand        hrn_dihedral_expand alone, (B*V, H, W) -> (K, B*V, H, W)
    mean          hrn_dihedral_mean alone, (K, B, 1, 3H, 3W) -> (B, 1, 3H, 3W)

and prints the overhead, ensemble - forward(K*B), in microseconds beside the byte floor of the two kernels: each moves
(1 + K) * N * H * W * 4 bytes, at the 6.3 TB/s a streaming kernel reaches on an MI355X (8 TB/s peak).  There is no pass / fail
threshold on time.

usage: python tools/ensemble_bench.py [B V S] [--precision P[,P...]] [--mode flip|dihedral] [--rounds R] [--reps N]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "highres-net_amd"))
import numpy as np
import torch

from oracle import synth, weights            # seeded weights / synthetic inputs only (no oracle arithmetic on the path)
from DeepNetworks.HRNet import HRNet
from hrnet_hip import augment, binding

HBM_ACHIEVABLE = 6.3e12                      # bytes / s: a float4 copy on the MI355X (79 % of the 8 TB/s peak)
LAUNCH_US = 1.5                              # a dependent kernel boundary on one stream, microseconds


def _options(argv):
    pos, opts, i = [], {}, 0
    while i < len(argv):
        if argv[i] in ("--precision", "--mode", "--rounds", "--reps"):
            opts[argv[i]] = argv[i + 1]
            i += 2
        else:
            pos.append(argv[i])
            i += 1
    return pos, opts


def _timed(fn, reps):
    """Microseconds per call: device events around `reps` calls enqueued back to back."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / reps


def main():
    args, opts = _options(sys.argv[1:])
    B, V, S = (int(a) for a in args[:3]) if len(args) >= 3 else (4, 32, 128)
    precs = opts.get("--precision", "bf16,bf16x3").split(",")
    mode = opts.get("--mode", "dihedral")
    rounds, reps = int(opts.get("--rounds", 7)), int(opts.get("--reps", 10))
    if not torch.cuda.is_available():
        raise SystemExit("ensemble_bench needs a ROCm device: a time cannot be measured without one")
    dev = torch.device("cuda:0")
    codes = augment.ensemble_codes(mode)
    K = len(codes)
    lrs, alphas = synth.fast_batch(3, B, V, S)
    x, a = torch.from_numpy(lrs).to(dev), torch.from_numpy(alphas).to(dev)
    big_lrs, big_alphas = synth.fast_batch(4, K * B, V, S)
    bx, ba = torch.from_numpy(big_lrs).to(dev), torch.from_numpy(big_alphas).to(dev)
    expand_bytes = (1 + K) * B * V * S * S * 4
    results = []
    models = {}
    for prec in precs:
        m = HRNet(weights.HRNET_CONFIG)
        m.load_state_dict(weights.to_torch_state(weights.hrnet_state(1234)))
        m.precision = prec
        models[prec] = m.to(dev).eval()
    scale = models[precs[0]]._scale
    srs = torch.rand((K, B, 1, scale * S, scale * S), device=dev)
    mean_bytes = (1 + K) * B * (scale * S) ** 2 * 4
    floor_us = (expand_bytes + mean_bytes) / HBM_ACHIEVABLE * 1e6
    with torch.no_grad():
        runs = {}
        for prec, m in models.items():
            runs[prec] = {"ensemble": lambda m=m: m.forward_ensemble(x, a, mode), "forward(K*B)": lambda m=m: m(bx, ba),
                          "expand": lambda: binding.dihedral_expand(x, codes), "mean": lambda: binding.dihedral_mean(srs, codes)}
        for r in runs.values():                                  # warm-up: every shape of the timed window, workspace growth included
            for fn in r.values():
                for _ in range(3):
                    fn()
        torch.cuda.synchronize()
        times = {prec: {k: [] for k in r} for prec, r in runs.items()}
        for _ in range(rounds):
            for prec, r in runs.items():
                for name, fn in r.items():
                    times[prec][name].append(_timed(fn, reps))
    for prec, t in times.items():
        med = {k: float(np.median(v)) for k, v in t.items()}
        spread = {k: (float(np.min(v)), float(np.max(v))) for k, v in t.items()}
        overhead = med["ensemble"] - med["forward(K*B)"]
        print(f"B={B} V={V} {S}x{S} x{scale} {prec} K={K} ({mode}), median of {rounds} rounds x {reps} calls:")
        for k in t:
            print(f"    {k:13s} {med[k]:10.1f} us   (min {spread[k][0]:.1f}, max {spread[k][1]:.1f})")
        print(f"    overhead = ensemble - forward(K*B): {overhead:.1f} us = {100 * overhead / med['forward(K*B)']:.2f} % of the forward; "
              f"expand + mean alone {med['expand'] + med['mean']:.1f} us")
        print(f"    byte floor of the two kernels: expand {expand_bytes / 1e6:.1f} MB + mean {mean_bytes / 1e6:.1f} MB at "
              f"{HBM_ACHIEVABLE / 1e12:.1f} TB/s = {floor_us:.1f} us; ten floors + two launches = {10 * floor_us + 2 * LAUNCH_US:.1f} us")
        results.append({"precision": prec, "B": B, "V": V, "S": S, "scale": scale, "K": K, "mode": mode, "median_us": med,
                        "overhead_us": overhead, "byte_floor_us": floor_us, "rounds": rounds, "reps": reps})
    print(json.dumps({"ensemble_bench": results}))


if __name__ == "__main__":
    main()
