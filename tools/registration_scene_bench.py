#!/usr/bin/env python3
"""Time the sub-pixel registration of frames of any size (hrnet_hip.registration's scene path) against the
LDS-resident kernels of section 7f at the same pixel count.

In ONE process, call by call alternating, after a warm-up, at P points per axis and L levels (default 7 and 6):

    scene      hrn_mncc_search_scene / hrn_mncc_apply_scene   B imagesets of V views of S x S        (default 2 x 32 of 512 x 512)
    lds        hrn_mncc_search / hrn_mncc_apply                LB imagesets of V views of LS x LS     (default 32 x 32 of 128 x 128)
    scene_lds  the scene entry points at the LDS kernels' shape: what the tiles, the halo and the 1 + 2 L launches cost there

Each call's time is the pair of device events the library's profiler (hrn_profile_enable) puts around its launches - all 1 + 2 L of a
scene search are inside one pair - so the Python between two calls is not in it.  A round is `reps` calls of each; the figure is the
median over the rounds, with min and max as the run-to-run spread.  The searches are compared per (pixel x level x grid point): the
scene path's figure over the LDS kernels' is the ratio the design allows 1.25 for.  There is no pass / fail threshold on time.

usage: python tools/registration_scene_bench.py [B] [--views V] [--size S] [--lds-batch LB] [--lds-size LS] [--points P] [--levels L]
                                                [--rounds R] [--reps N]
"""
import _common
import torch

from hrnet_hip import binding

PARSER = _common.parser(__doc__, positional=dict(B=2), views=32, size=512, lds_batch=32, lds_size=128, points=7, levels=6, rounds=7, reps=5)


def frames(B, V, S, dev):
    """Smooth frames, every view a crop one whole pixel off the reference's at the most, so that the search has a peak to walk to:
    -> (ref, ref_mask, views, masks, the true shifts (V, 2))"""
    gen = torch.Generator(device=dev).manual_seed(S)
    base = torch.nn.functional.avg_pool2d(torch.rand((B, 1, S + 12, S + 12), device=dev, generator=gen), 5, 1)
    offs = torch.randint(3, 6, (V, 2), generator=torch.Generator().manual_seed(S))
    views = torch.stack([base[:, 0, oy:oy + S, ox:ox + S] for oy, ox in offs.tolist()], 1).contiguous()
    ref = base[:, 0, 4:4 + S, 4:4 + S].contiguous()
    masks = (torch.rand((B, V, S, S), device=dev, generator=gen) > 0.05).float()
    ref_mask = (torch.rand((B, S, S), device=dev, generator=gen) > 0.05).float()
    return ref, ref_mask, views, masks, (4.0 - offs.to(dev).float())


def bench(B, V, S, LB, LS, P, levels, rounds, reps):
    dev = torch.device("cuda:0")
    big, small = frames(B, V, S, dev), frames(LB, V, LS, dev)

    def run(search, apply, data):
        ref, ref_mask, views, masks, _ = data
        shifts, _ = search(ref, ref_mask, views, masks, P, levels, 1.0)
        apply(views, masks, shifts)
        return shifts

    candidates = {"scene": (lambda: run(binding.mncc_search_scene, binding.mncc_apply_scene, big), ("mncc_search_scene", "mncc_apply_scene"), big),
                  "lds": (lambda: run(binding.mncc_search, binding.mncc_apply, small), ("mncc_search", "mncc_apply"), small),
                  "scene_lds": (lambda: run(binding.mncc_search_scene, binding.mncc_apply_scene, small), ("mncc_search_scene", "mncc_apply_scene"), small)}
    res = {"B": B, "V": V, "S": S, "lds_batch": LB, "lds_size": LS, "points": P, "levels": levels, "rounds": rounds, "reps": reps}
    per_round = {name: {"search": [], "apply": []} for name in candidates}
    for name, (fn, _, data) in candidates.items():
        res[name] = {"worst_shift_error_px": float((fn() - data[4][None]).abs().max())}       # the search finds the offsets before it is timed
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for name, (fn, families, _) in candidates.items():
            binding.profile_enable(True)
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            rec = binding.profile_read()
            binding.profile_enable(False)
            for what, family in zip(("search", "apply"), families):
                per_round[name][what].append(rec[family]["ms"] * 1e3 / rec[family]["launches"])
    print(f"P={P} levels={levels}: median of {rounds} rounds x {reps} calls")
    for name, (_, _, data) in candidates.items():
        b, v, h, w = data[2].shape
        for what in ("search", "apply"):
            med, lo, hi = _common.spread(per_round[name][what])
            res[name][what] = {"median_us": med, "min_us": lo, "max_us": hi}
        res[name]["shape"] = [b, v, h, w]
        res[name]["ps_per_pixel_level_point"] = res[name]["search"]["median_us"] * 1e6 / (b * v * h * w * levels * P * P)
        print(f"    {name:10s} {b} x {v} x {h} x {w}: search {res[name]['search']['median_us']:10.1f} us (min {res[name]['search']['min_us']:.1f}, "
              f"max {res[name]['search']['max_us']:.1f}) = {res[name]['ps_per_pixel_level_point']:.3f} ps per (pixel x level x grid point); "
              f"apply {res[name]['apply']['median_us']:8.1f} us (min {res[name]['apply']['min_us']:.1f}, max {res[name]['apply']['max_us']:.1f}); "
              f"worst shift error {res[name]['worst_shift_error_px']:.4f} px")
    lds = res["lds"]["ps_per_pixel_level_point"]
    res["scene_over_lds"] = res["scene"]["ps_per_pixel_level_point"] / lds
    res["scene_lds_over_lds"] = res["scene_lds"]["ps_per_pixel_level_point"] / lds
    res["apply_scene_over_apply"] = res["scene_lds"]["apply"]["median_us"] / res["lds"]["apply"]["median_us"]
    print(f"    per (pixel x level x grid point), scene / lds: {res['scene_over_lds']:.3f} at {S} x {S}, {res['scene_lds_over_lds']:.3f} at "
          f"{LS} x {LS}; apply_scene / apply at {LS} x {LS}: {res['apply_scene_over_apply']:.3f}")
    return res


def main():
    o = PARSER.parse_args()
    _common.require_gpu("registration_scene_bench")
    _common.emit("registration_scene_bench", bench(o.B, o.views, o.size, o.lds_batch, o.lds_size, o.points, o.levels, o.rounds, o.reps))


if __name__ == "__main__":
    main()
