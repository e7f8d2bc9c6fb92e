#!/usr/bin/env python3
"""Time the backward of the six-tap resampler (hrn_mncc_apply_backward) against its forward, its byte floors and
torch autograd through the same definition.

In ONE process, call by call alternating, after a warm-up, at two shapes - B imagesets of V views of S x S (default 2 x 32 of 512 x 512)
and SB of V views of SS x SS (default 32 x 32 of 128 x 128):

    forward   hrn_mncc_apply_scene                            reads the view and its mask, writes out and valid
    d_views   hrn_mncc_apply_backward, d_shifts NULL          one launch:  reads d_out and valid, writes d_views
    d_shifts  hrn_mncc_apply_backward, d_views NULL           two launches: reads the view, d_out and valid
    both      hrn_mncc_apply_backward with both               three launches

Each time is the pair of device events the library's profiler (hrn_profile_enable) puts around a call's launches, so the Python between
two calls is not in it.  A round is `reps` calls of each; the figure is the median over the rounds, with min and max as the run-to-run
spread.  Each half is stated as a ratio to the forward's time in the same process and to its byte floor: 12 bytes a pixel for either
half (the forward moves 16) at the bandwidth a streaming kernel reaches.

`torch` is the same definition composed from 36 shifted slices of the views with the taps as differentiable functions of the shifts,
forward and backward under torch autograd, timed with device events around the pair.  Its shifts share their whole parts, so that the
slices are plain views; its gradients are compared with the library's (worst absolute difference over the worst magnitude).  There is
no pass / fail threshold on time.

usage: python tools/warp_bench.py [B] [--views V] [--size S] [--small-batch SB] [--small-size SS] [--rounds R] [--reps N]
"""
import math

import _common
import torch

from hrnet_hip import binding

PARSER = _common.parser(__doc__, positional=dict(B=2), views=32, size=512, small_batch=32, small_size=128, rounds=7, reps=5)
FAMILIES = {"forward": ("mncc_apply_scene",), "d_views": ("mncc_apply_backward_views",), "d_shifts": ("mncc_apply_backward_shifts",),
            "both": ("mncc_apply_backward_views", "mncc_apply_backward_shifts")}
FLOOR_BYTES = {"forward": 16, "d_views": 12, "d_shifts": 12, "both": 24}      # per pixel of a plane


def data(B, V, S, dev):
    """Smooth views, masks with 5 % of the pixels set, shifts in (0, 1) x (-1, 0) - one whole part per axis - and a standard normal d_out"""
    gen = torch.Generator(device=dev).manual_seed(S)
    views = torch.nn.functional.avg_pool2d(torch.rand((B * V, 1, S + 4, S + 4), device=dev, generator=gen), 5, 1).reshape(B, V, S, S).contiguous()
    masks = (torch.rand((B, V, S, S), device=dev, generator=gen) > 0.05).float()
    shifts = torch.rand((B, V, 2), device=dev, generator=gen) * 0.8 + 0.1
    shifts[..., 1] -= 1.0
    d_out = torch.randn((B, V, S, S), device=dev, generator=gen)
    return views, masks, shifts, d_out


def torch_warp(views, shifts):
    """S(view, shift) where the footprint is inside the frame, from 36 slices: the whole parts are (0, -1) for every view"""
    H, W = views.shape[2:]
    o = torch.arange(-2, 4, device=views.device, dtype=torch.float64)

    def taps(d):
        x = o - (d.double() - torch.floor(d.double()))[..., None]
        k = torch.sinc(x) * torch.sinc(x / 3.0)
        return (k / k.sum(-1, keepdim=True)).float()

    ky, kx = taps(shifts[..., 0]), taps(shifts[..., 1])
    ny, nx = 0, -1
    y0, y1, x0, x1 = max(0, 2 - ny), min(H, H - 3 - ny), max(0, 2 - nx), min(W, W - 3 - nx)
    out = 0.0
    for a in range(6):
        for b in range(6):
            out = out + (ky[..., a] * kx[..., b])[..., None, None] * views[:, :, y0 + ny + a - 2:y1 + ny + a - 2, x0 + nx + b - 2:x1 + nx + b - 2]
    return out, (y0, y1, x0, x1)


def bench_shape(B, V, S, rounds, reps, dev):
    views, masks, shifts, d_out = data(B, V, S, dev)
    _, valid = binding.mncc_apply_scene(views, masks, shifts)
    runs = {"forward": lambda: binding.mncc_apply_scene(views, masks, shifts),
            "d_views": lambda: binding.mncc_apply_backward(views, shifts, valid, d_out, True, False),
            "d_shifts": lambda: binding.mncc_apply_backward(views, shifts, valid, d_out, False, True),
            "both": lambda: binding.mncc_apply_backward(views, shifts, valid, d_out, True, True)}

    # torch autograd through the same definition, on the gradient the library sees: d_out where valid
    tv, ts = views.clone().requires_grad_(True), shifts.clone().requires_grad_(True)

    def torch_pair():
        tv.grad = ts.grad = None
        out, (y0, y1, x0, x1) = torch_warp(tv, ts)
        out.backward((d_out * valid)[:, :, y0:y1, x0:x1])

    torch_pair()
    d_views, d_shifts = runs["both"]()
    res = {"shape": [B, V, S, S],
           "d_views_vs_torch": float((d_views - tv.grad).abs().max() / tv.grad.abs().max()),
           "d_shifts_vs_torch": float((d_shifts - ts.grad).abs().max() / ts.grad.abs().max())}
    for fn in runs.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    per_round = {name: [] for name in runs}
    torch_us = []
    for _ in range(rounds):
        for name, fn in runs.items():
            binding.profile_enable(True)
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            rec = binding.profile_read()
            binding.profile_enable(False)
            per_round[name].append(sum(rec[f]["ms"] for f in FAMILIES[name]) * 1e3 / reps)
        torch_us.append(_common.timed_us(torch_pair, 1))
    pixels = B * V * S * S
    print(f"{B} x {V} x {S} x {S}: median of {rounds} rounds x {reps} calls")
    for name in runs:
        med, lo, hi = _common.spread(per_round[name])
        floor_us = FLOOR_BYTES[name] * pixels / _common.HBM_ACHIEVABLE * 1e6
        res[name] = {"median_us": med, "min_us": lo, "max_us": hi, "floor_us": floor_us, "over_floor": med / floor_us}
    for name in runs:
        res[name]["over_forward"] = res[name]["median_us"] / res["forward"]["median_us"]
        r = res[name]
        print(f"    {name:9s} {r['median_us']:9.1f} us (min {r['min_us']:.1f}, max {r['max_us']:.1f}) = {r['over_forward']:.2f} x forward, "
              f"{r['over_floor']:.2f} x its byte floor of {r['floor_us']:.1f} us")
    med, lo, hi = _common.spread(torch_us)
    res["torch"] = {"median_us": med, "min_us": lo, "max_us": hi, "over_both": med / (res["forward"]["median_us"] + res["both"]["median_us"])}
    print(f"    torch     {med:9.1f} us (min {lo:.1f}, max {hi:.1f}) forward + backward from 36 slices = {res['torch']['over_both']:.1f} x "
          f"forward + both; d_views differs by {res['d_views_vs_torch']:.2e}, d_shifts by {res['d_shifts_vs_torch']:.2e} of the largest")
    assert math.isfinite(res["d_views_vs_torch"]) and math.isfinite(res["d_shifts_vs_torch"])
    return res


def main():
    o = PARSER.parse_args()
    _common.require_gpu("warp_bench")
    dev = torch.device("cuda:0")
    _common.emit("warp_bench", [bench_shape(o.B, o.views, o.size, o.rounds, o.reps, dev),
                                bench_shape(o.small_batch, o.views, o.small_size, o.rounds, o.reps, dev)])


if __name__ == "__main__":
    main()
