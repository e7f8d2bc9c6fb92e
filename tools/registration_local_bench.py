#!/usr/bin/env python3
"""Time the shift field of a scene (hrnet_hip.registration's mncc_search_local / shift_field) against the one
shift per view of section 7g on the same inputs.

In ONE process, call by call alternating, after a warm-up, at P points per axis (default 7), B imagesets of V views of S x S (default
2 x 32 of 512 x 512):

    global       mncc_search_scene, L levels of radius 1                               (default 6)
    local        mncc_search_local from those shifts, LL levels of radius 0.5, `block` (default 4 levels, block 128)
    apply_scene  shift_scene by the global shifts
    apply_field  shift_field by the same shifts as a constant field: the same pixels out, every pixel by taps of its own

Each is timed by device events around `reps` calls (tools/_common.py); a round is one such window per candidate, the figure the median
over the rounds with min and max as the run-to-run spread.  A search has one pre-pass for the means besides its levels, so the time per
level is reported as (time - means) / levels with the means' time taken from a one-level search: level = (t_L - t_1) / (L - 1).  The
level kernels do the same work, so local / global per level is expected at parity; 1.10 is where it would be reported as a problem.
There is no pass / fail threshold on time.

usage: python tools/registration_local_bench.py [B] [--views V] [--size S] [--block N] [--points P] [--levels L] [--local-levels LL]
                                                [--rounds R] [--reps N]
"""
import _common
import torch

from hrnet_hip import binding, registration
from registration_scene_bench import frames

PARSER = _common.parser(__doc__, positional=dict(B=2), views=32, size=512, block=128, points=7, levels=6, local_levels=4, rounds=7, reps=5)


def bench(B, V, S, block, P, levels, local_levels, rounds, reps):
    ref, ref_mask, views, masks, true = frames(B, V, S, torch.device("cuda:0"))
    shifts, _ = binding.mncc_search_scene(ref, ref_mask, views, masks, P, levels, 1.0)
    by, bx = registration.local_blocks(S, S, block)
    const = shifts[:, :, None, None, :].expand(B, V, by, bx, 2).contiguous()
    field, _, ok = binding.mncc_search_local(ref, ref_mask, views, masks, shifts, P, local_levels, 0.5, block, 0.25)
    res = {"B": B, "V": V, "S": S, "block": block, "blocks": [by, bx], "points": P, "levels": levels, "local_levels": local_levels,
           "rounds": rounds, "reps": reps, "worst_global_error_px": float((shifts - true[None]).abs().max()),
           "worst_node_error_px": float((field - true[None, :, None, None, :]).abs().max()), "blocks_ok": float(ok.mean())}
    a, b = binding.mncc_apply_scene(views, masks, shifts), binding.mncc_apply_field(views, masks, const, block)
    res["constant_field_is_shift_scene"] = bool(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]))
    runs = {"global": lambda: binding.mncc_search_scene(ref, ref_mask, views, masks, P, levels, 1.0),
            "global_1": lambda: binding.mncc_search_scene(ref, ref_mask, views, masks, P, 1, 1.0),
            "local": lambda: binding.mncc_search_local(ref, ref_mask, views, masks, shifts, P, local_levels, 0.5, block, 0.25),
            "local_1": lambda: binding.mncc_search_local(ref, ref_mask, views, masks, shifts, P, 1, 0.5, block, 0.25),
            "apply_scene": lambda: binding.mncc_apply_scene(views, masks, shifts),
            "apply_field": lambda: binding.mncc_apply_field(views, masks, const, block)}
    times = _common.alternate(runs, rounds, reps, warmup=3)
    print(f"{B} x {V} x {S} x {S}, P={P}, block {block} ({by} x {bx} blocks): median of {rounds} rounds x {reps} calls")
    for name, t in times.items():
        med, lo, hi = _common.spread(t)
        res[name] = {"median_us": med, "min_us": lo, "max_us": hi}
        print(f"    {name:12s} {med:10.1f} us (min {lo:.1f}, max {hi:.1f})")
    us = lambda name: res[name]["median_us"]
    res["global_level_us"] = (us("global") - us("global_1")) / (levels - 1) if levels > 1 else us("global")
    res["local_level_us"] = (us("local") - us("local_1")) / (local_levels - 1) if local_levels > 1 else us("local")
    res["local_over_global_per_level"] = res["local_level_us"] / res["global_level_us"]
    res["apply_field_over_apply_scene"] = us("apply_field") / us("apply_scene")
    print(f"    per level: global {res['global_level_us']:.1f} us, local {res['local_level_us']:.1f} us, local / global "
          f"{res['local_over_global_per_level']:.3f}; apply_field / apply_scene {res['apply_field_over_apply_scene']:.2f}; worst error: "
          f"global {res['worst_global_error_px']:.4f} px, nodes {res['worst_node_error_px']:.4f} px, {100 * res['blocks_ok']:.0f} % of blocks ok; "
          f"a constant field gives shift_scene's bits: {res['constant_field_is_shift_scene']}")
    return res


def main():
    o = PARSER.parse_args()
    _common.require_gpu("registration_local_bench")
    _common.emit("registration_local_bench", bench(o.B, o.views, o.size, o.block, o.points, o.levels, o.local_levels, o.rounds, o.reps))


if __name__ == "__main__":
    main()
