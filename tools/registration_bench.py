#!/usr/bin/env python3
"""Time the sub-pixel registration of LR views (hrnet_hip.registration).

At B imagesets of V views of S x S (default 32 x 32 of 128 x 128: one batch of PROBA-V LR frames), P points per axis and L levels
(default 7 and 6), this times in ONE process, call by call alternating, after a warm-up:

    mncc_search   hrn_mncc_search   the whole search of every view in one launch: a workgroup per view, the view in LDS
    mncc_apply    hrn_mncc_apply    the views resampled by the shifts found

Each call's time is the pair of device events the library's profiler (hrn_profile_enable) puts around its launch, so the Python between
two calls is not in it.  A round is `reps` calls of each; the figure is the median over the rounds, with min and max as the run-to-run
spread.  The search is also stated per (view x level x grid point), and against its arithmetic floor: the counted operations at the
fp32 vector peak of an MI355X (256 CUs x 128 lanes x 2 per fused multiply-add x 2.4 GHz = 157 TFLOP/s).  The count, per pixel and level:
the pass along rows, P x 6 taps x 2, and per grid point the pass along columns, the mask test and the six sums, P^2 x (6 x 2 + 20).
For scale, the fp64 restatement the tests compare against (tests/registration_ref.py, numpy) is timed on the CPU for one view.
There is no pass / fail threshold on time.

usage: python tools/registration_bench.py [B] [--views V] [--sizes S[,S...]] [--points P] [--levels L] [--rounds R] [--reps N]
"""
import time

import _common
import torch

from hrnet_hip import binding

FAMILIES = ("mncc_search", "mncc_apply")
FP32_VECTOR_PEAK = 256 * 128 * 2 * 2.4e9     # FLOP / s

PARSER = _common.parser(__doc__, positional=dict(B=32), views=32, sizes=[128], points=7, levels=6, rounds=7, reps=5)


def level_flops_per_pixel(P):
    """the counted arithmetic of one level, per pixel: rows P 6 2, then per grid point columns 6 2 and about 20 for the mask and the sums"""
    return P * 6 * 2 + P * P * (6 * 2 + 20)


def restatement_seconds(S, P, levels):
    """one view through tests/registration_ref.search on the CPU"""
    _common.tests_on_path()
    import registration_ref as R
    shifts = R.random_shifts(1, 0.9, seed=S)
    ref, ref_mask, views, view_masks = R.scene(S, S, shifts, seed=S)
    t0 = time.perf_counter()
    R.search(ref, ref_mask, views[0], view_masks[0], P, levels, 1.0)
    return time.perf_counter() - t0


def bench(B, V, S, P, levels, rounds, reps):
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(S)
    # smooth frames, every view a crop one whole pixel off the reference's at the most, so that the search has a peak to walk to
    base = torch.nn.functional.avg_pool2d(torch.rand((B, 1, S + 12, S + 12), device=dev, generator=gen), 5, 1)
    offs = torch.randint(3, 6, (V, 2), generator=torch.Generator().manual_seed(S))
    views = torch.stack([base[:, 0, oy:oy + S, ox:ox + S] for oy, ox in offs.tolist()], 1).contiguous()
    ref = base[:, 0, 4:4 + S, 4:4 + S].contiguous()
    masks = (torch.rand((B, V, S, S), device=dev, generator=gen) > 0.05).float()
    ref_mask = (torch.rand((B, S, S), device=dev, generator=gen) > 0.05).float()

    def one():
        shifts, _ = binding.mncc_search(ref, ref_mask, views, masks, P, levels, 1.0)
        binding.mncc_apply(views, masks, shifts)
        return shifts

    shifts = one()
    found = float((shifts - (4.0 - offs.to(dev).float())[None]).abs().max())           # the search finds the offsets before it is timed
    for _ in range(3):
        one()
    torch.cuda.synchronize()
    per_round = {f: [] for f in FAMILIES}
    for _ in range(rounds):
        binding.profile_enable(True)
        for _ in range(reps):
            one()
        torch.cuda.synchronize()
        rec = binding.profile_read()
        binding.profile_enable(False)
        for f in FAMILIES:
            per_round[f].append(rec[f]["ms"] * 1e3 / rec[f]["launches"])
    flops = float(level_flops_per_pixel(P)) * levels * B * V * S * S
    floor_us = flops / FP32_VECTOR_PEAK * 1e6
    cpu_s = restatement_seconds(S, P, levels)
    res = {"B": B, "V": V, "S": S, "points": P, "levels": levels, "rounds": rounds, "reps": reps, "worst_shift_error_px": found,
           "search_flops": flops, "flops_per_pixel_per_level": level_flops_per_pixel(P), "search_floor_us": floor_us,
           "restatement_one_view_cpu_s": cpu_s}
    print(f"B={B} V={V} {S}x{S} P={P} levels={levels}: median of {rounds} rounds x {reps} calls (worst shift error {found:.4f} px)")
    for f in FAMILIES:
        med, lo, hi = _common.spread(per_round[f])
        res[f] = {"median_us": med, "min_us": lo, "max_us": hi}
        print(f"    {f:12s} {med:10.1f} us   (min {lo:.1f}, max {hi:.1f})")
    med = res["mncc_search"]["median_us"]
    res["ns_per_view_level_point"] = med * 1e3 / (B * V * levels * P * P)
    print(f"    search: {res['ns_per_view_level_point']:.2f} ns per (view x level x grid point); {flops / 1e9:.1f} GFLOP counted "
          f"({level_flops_per_pixel(P)} per pixel per level) = {flops / med / 1e6:.1f} TFLOP/s, arithmetic floor {floor_us:.0f} us = "
          f"{100 * floor_us / med:.0f} % of it")
    print(f"    the fp64 restatement, one view on the CPU: {cpu_s:.2f} s = {cpu_s * B * V:.0f} s for the batch")
    return res


def main():
    o = PARSER.parse_args()
    _common.require_gpu("registration_bench")
    _common.emit("registration_bench", [bench(o.B, o.views, S, o.points, o.levels, o.rounds, o.reps) for S in o.sizes])


if __name__ == "__main__":
    main()
