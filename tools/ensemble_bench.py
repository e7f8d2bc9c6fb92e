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
import _common
import torch

from _common import HBM_ACHIEVABLE, LAUNCH_US
from oracle import synth, weights            # seeded weights / synthetic inputs only (no oracle arithmetic on the path)
from DeepNetworks.HRNet import HRNet
from hrnet_hip import augment, binding


PARSER = _common.parser(__doc__, group=("B V S", (4, 32, 128)), precision=["bf16", "bf16x3"], mode="dihedral", rounds=7, reps=10)


def main():
    o = PARSER.parse_args()
    B, V, S, precs, mode, rounds, reps = o.B, o.V, o.S, o.precision, o.mode, o.rounds, o.reps
    _common.require_gpu("ensemble_bench")
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
            runs.update({(prec, "ensemble"): lambda m=m: m.forward_ensemble(x, a, mode), (prec, "forward(K*B)"): lambda m=m: m(bx, ba),
                         (prec, "expand"): lambda: binding.dihedral_expand(x, codes), (prec, "mean"): lambda: binding.dihedral_mean(srs, codes)})
        times = _common.alternate(runs, rounds, reps, warmup=3)
    for prec in models:
        t = {name: _common.spread(v) for (p, name), v in times.items() if p == prec}
        med = {k: v[0] for k, v in t.items()}
        overhead = med["ensemble"] - med["forward(K*B)"]
        print(f"B={B} V={V} {S}x{S} x{scale} {prec} K={K} ({mode}), median of {rounds} rounds x {reps} calls:")
        for k in t:
            print(f"    {k:13s} {med[k]:10.1f} us   (min {t[k][1]:.1f}, max {t[k][2]:.1f})")
        print(f"    overhead = ensemble - forward(K*B): {overhead:.1f} us = {100 * overhead / med['forward(K*B)']:.2f} % of the forward; "
              f"expand + mean alone {med['expand'] + med['mean']:.1f} us")
        print(f"    byte floor of the two kernels: expand {expand_bytes / 1e6:.1f} MB + mean {mean_bytes / 1e6:.1f} MB at "
              f"{HBM_ACHIEVABLE / 1e12:.1f} TB/s = {floor_us:.1f} us; ten floors + two launches = {10 * floor_us + 2 * LAUNCH_US:.1f} us")
        results.append({"precision": prec, "B": B, "V": V, "S": S, "scale": scale, "K": K, "mode": mode, "median_us": med,
                        "overhead_us": overhead, "byte_floor_us": floor_us, "rounds": rounds, "reps": reps})
    _common.emit("ensemble_bench", results)


if __name__ == "__main__":
    main()
