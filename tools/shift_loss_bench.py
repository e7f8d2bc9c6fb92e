#!/usr/bin/env python3
"""Time the searched loss's kernels against the scorer they generalise.

At B samples of S x S (default 32 of 192 x 192 and of 384 x 384: the x3 training patch and the evaluation scene), border 3, this times in
ONE process, call by call alternating, after a warm-up:

    shift_loss_fwd   hrn_shift_loss_train      every pixel of srs / hrs / maps once, the 49 offsets out of LDS: 12 B S^2 bytes
    shift_loss_bwd   hrn_shift_loss_backward   one elementwise pass: 16 B S^2 bytes
    shift_cpsnr      hrn_shift_cpsnr           the unchanged scorer: 49 workgroups per sample, each re-reading the sample out of L2

Each call's time is the pair of device events the library's profiler (hrn_profile_enable) puts around its launches, so the Python
between two calls is not in it.  The calls walk over enough input sets to exceed the 256 MB last-level cache, so the bytes come from
HBM.  A round is `reps` calls of each; the figure is the median over the rounds, with min and max as the run-to-run spread.  The byte
floors are the algorithmic bytes at the 6.3 TB/s a streaming kernel reaches on an MI355X (8 TB/s peak).  There is no pass / fail
threshold on time.

usage: python tools/shift_loss_bench.py [B] [--sizes S[,S...]] [--border W] [--rounds R] [--reps N]
"""
import _common
import torch

from _common import HBM_ACHIEVABLE, LLC_BYTES
from hrnet_hip import binding

FAMILIES = ("shift_loss_fwd", "shift_loss_bwd", "shift_cpsnr")


PARSER = _common.parser(__doc__, positional=dict(B=32), sizes=[192, 384], border=3, rounds=7, reps=20)


def floors_us(B, S):
    """the byte floors of the forward (12 B S^2) and the backward (16 B S^2) in microseconds"""
    return 12.0 * B * S * S / HBM_ACHIEVABLE * 1e6, 16.0 * B * S * S / HBM_ACHIEVABLE * 1e6


def bench(B, S, border, rounds, reps):
    dev = torch.device("cuda:0")
    nsets = max(2, -(-2 * LLC_BYTES // (12 * B * S * S)))
    gen = torch.Generator(device=dev).manual_seed(S)
    sets = []
    for _ in range(nsets):
        srs = torch.rand((B, S, S), device=dev, generator=gen)
        hrs = torch.rand((B, S, S), device=dev, generator=gen)
        maps = (torch.rand((B, S, S), device=dev, generator=gen) > 0.1).float()
        sets.append((srs, hrs, maps))
    d_out = torch.full((B,), -1.0 / B, device=dev)

    def one(i):
        s, h, m = sets[i % nsets]
        out, stats = binding.shift_loss_train(s, h, m, "cPSNR", border, True)
        binding.shift_loss_backward(s, h, m, stats, d_out, "cPSNR", border, True)
        old = binding.shift_cpsnr(s, h, m, border, True)
        return out, old

    out, old = one(0)
    worst = float(((out - old).abs() / old.abs()).max())        # the two forwards score alike before either is timed
    for i in range(2 * nsets):
        one(i)
    torch.cuda.synchronize()
    per_round = {f: [] for f in FAMILIES}
    for r in range(rounds):
        binding.profile_enable(True)
        for i in range(reps):
            one(r * reps + i)
        torch.cuda.synchronize()
        rec = binding.profile_read()
        binding.profile_enable(False)
        for f in FAMILIES:
            per_round[f].append(rec[f]["ms"] * 1e3 / rec[f]["launches"])
    fwd_floor, bwd_floor = floors_us(B, S)
    res = {"B": B, "S": S, "border": border, "input_sets": nsets, "rounds": rounds, "reps": reps, "fwd_vs_shift_cpsnr_rel": worst,
           "fwd_floor_us": fwd_floor, "bwd_floor_us": bwd_floor}
    print(f"B={B} {S}x{S} border {border}: median of {rounds} rounds x {reps} calls over {nsets} input sets "
          f"(forward vs hrn_shift_cpsnr: {worst:.1e} relative)")
    for f in FAMILIES:
        med, lo, hi = _common.spread(per_round[f])
        res[f] = {"median_us": med, "min_us": lo, "max_us": hi}
        floor = bwd_floor if f == "shift_loss_bwd" else fwd_floor
        print(f"    {f:15s} {med:9.1f} us   (min {lo:.1f}, max {hi:.1f})   byte floor {floor:.1f} us = "
              f"{100 * floor / med:.0f} % of it")
    print(f"    hrn_shift_cpsnr / hrn_shift_loss_train: {res['shift_cpsnr']['median_us'] / res['shift_loss_fwd']['median_us']:.2f} x")
    return res


def main():
    o = PARSER.parse_args()
    _common.require_gpu("shift_loss_bench")
    _common.emit("shift_loss_bench", [bench(o.B, S, o.border, o.rounds, o.reps) for S in o.sizes])


if __name__ == "__main__":
    main()
