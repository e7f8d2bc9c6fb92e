#!/usr/bin/env python3
"""Time the coarse-to-fine registration search (hrnet_hip.registration's mncc_search_pyramid / reduce2) against
the plain scene search of section 7g on the same inputs.

In ONE process, call by call alternating, after a warm-up, at P points per axis (default 7), B imagesets of V views of S x S (default
2 x 32 of 512 x 512) whose views lie up to 5 * 2^(K-1) whole pixels from the reference:

    scene     mncc_search_scene, L levels of radius 4                                   (default 6; it cannot find these shifts)
    pyramid   mncc_search_pyramid over K octaves: radius 4 and CL levels at the top, radius 1 below, L levels at octave 0
              (default K = 3, CL = 3)
    reduce2   the masked reduction of the B V views and the B references of octave 0, with masks
    copy      a device copy of a buffer of 5 bytes per pixel of those planes: 10 H W bytes per plane read and written, streamed

Each is timed by device events around `reps` calls (tools/_common.py); a round is one such window per candidate, the figure the median
over the rounds with min and max as the run-to-run spread.  The level count predicts pyramid / scene = (L + CL / 4 + .. + CL / 4^K) / L
plus the reductions, the doublings and K more passes for the means; the excess over that count is reported.  reduce2 is reported
against its byte floor (10 H W bytes a plane at tools/_common.HBM_ACHIEVABLE) and against the copy.  There is no pass / fail threshold
on time.

usage: python tools/registration_pyramid_bench.py [B] [--views V] [--size S] [--octaves K] [--points P] [--levels L]
                                                  [--coarse-levels CL] [--rounds R] [--reps N]
"""
import _common
import torch

from hrnet_hip import binding

PARSER = _common.parser(__doc__, positional=dict(B=2), views=32, size=512, octaves=3, points=7, levels=6, coarse_levels=3, rounds=7, reps=5)


def frames(B, V, S, reach, dev):
    """Smooth frames, every view a crop up to `reach` whole pixels off the reference's: -> (ref, ref_mask, views, masks, true (V, 2))"""
    gen = torch.Generator(device=dev).manual_seed(S)
    pad = reach + 2
    base = torch.nn.functional.avg_pool2d(torch.rand((B, 1, S + 2 * pad + 4, S + 2 * pad + 4), device=dev, generator=gen), 5, 1)
    offs = torch.randint(-reach, reach + 1, (V, 2), generator=torch.Generator().manual_seed(S))
    views = torch.stack([base[:, 0, pad + oy:pad + oy + S, pad + ox:pad + ox + S] for oy, ox in offs.tolist()], 1).contiguous()
    ref = base[:, 0, pad:pad + S, pad:pad + S].contiguous()
    masks = (torch.rand((B, V, S, S), device=dev, generator=gen) > 0.05).float()
    ref_mask = (torch.rand((B, S, S), device=dev, generator=gen) > 0.05).float()
    return ref, ref_mask, views, masks, -offs.to(dev).float()         # ref(y, x) = view(y - oy, x - ox)


def bench(B, V, S, K, P, levels, coarse_levels, rounds, reps):
    dev = torch.device("cuda:0")
    reach = 5 * 2 ** (K - 1) if K else 2
    ref, ref_mask, views, masks, true = frames(B, V, S, reach, dev)
    found, _ = binding.mncc_search_pyramid(ref, ref_mask, views, masks, K, P, levels, 4.0, coarse_levels, 1.0)
    plain, _ = binding.mncc_search_scene(ref, ref_mask, views, masks, P, levels, 4.0)
    planes = torch.cat([views.reshape(-1, S, S), ref])
    plane_masks = torch.cat([masks.reshape(-1, S, S), ref_mask])
    src = torch.empty(planes.shape[0] * S * S * 5 // 4, dtype=torch.float32, device=dev).normal_()
    dst = torch.empty_like(src)
    res = {"B": B, "V": V, "S": S, "octaves": K, "points": P, "levels": levels, "coarse_levels": coarse_levels, "rounds": rounds, "reps": reps,
           "largest_true_shift_px": float(true.abs().max()), "worst_pyramid_error_px": float((found - true[None]).abs().max()),
           "worst_scene_error_px": float((plain - true[None]).abs().max())}
    runs = {"scene": lambda: binding.mncc_search_scene(ref, ref_mask, views, masks, P, levels, 4.0),
            "pyramid": lambda: binding.mncc_search_pyramid(ref, ref_mask, views, masks, K, P, levels, 4.0, coarse_levels, 1.0),
            "reduce2": lambda: binding.mncc_reduce2(planes, plane_masks),
            "copy": lambda: dst.copy_(src)}
    times = _common.alternate(runs, rounds, reps, warmup=3)
    print(f"{B} x {V} x {S} x {S}, P={P}, {K} octaves, shifts up to {reach} px: median of {rounds} rounds x {reps} calls")
    for name, t in times.items():
        med, lo, hi = _common.spread(t)
        res[name] = {"median_us": med, "min_us": lo, "max_us": hi}
        print(f"    {name:8s} {med:10.1f} us (min {lo:.1f}, max {hi:.1f})")
    us = lambda name: res[name]["median_us"]
    res["predicted_ratio_by_levels"] = (levels + sum(coarse_levels / 4.0 ** k for k in range(1, K + 1))) / levels
    res["pyramid_over_scene"] = us("pyramid") / us("scene")
    res["reduce2_bytes"] = 10 * planes.shape[0] * S * S
    res["reduce2_floor_us"] = res["reduce2_bytes"] / _common.HBM_ACHIEVABLE * 1e6
    res["reduce2_over_floor"] = us("reduce2") / res["reduce2_floor_us"]
    res["reduce2_over_copy"] = us("reduce2") / us("copy")
    res["working_set_fits_llc"] = res["reduce2_bytes"] <= _common.LLC_BYTES
    print(f"    pyramid / scene {res['pyramid_over_scene']:.3f} (the level count predicts {res['predicted_ratio_by_levels']:.3f}); reduce2 "
          f"{res['reduce2_over_floor']:.2f} x its byte floor of {res['reduce2_floor_us']:.1f} us and {res['reduce2_over_copy']:.2f} x the copy of the "
          f"same bytes (working set {'inside' if res['working_set_fits_llc'] else 'beyond'} the last-level cache); worst error: pyramid "
          f"{res['worst_pyramid_error_px']:.4f} px, plain search {res['worst_scene_error_px']:.2f} px at shifts up to "
          f"{res['largest_true_shift_px']:.0f} px")
    return res


def main():
    o = PARSER.parse_args()
    _common.require_gpu("registration_pyramid_bench")
    _common.emit("registration_pyramid_bench", bench(o.B, o.views, o.size, o.octaves, o.points, o.levels, o.coarse_levels, o.rounds, o.reps))


if __name__ == "__main__":
    main()
