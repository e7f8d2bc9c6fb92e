#!/usr/bin/env python3
"""What tiled inference costs: three measurements on one MI355X, in ONE process.

    tax     a scene that also fits whole (default B = 1, V = 32, 512 x 512): HRNet.forward_tiled at each --tiles side against the
            plain whole-frame forward, alternating round by round after a warm-up, device events around `reps` back-to-back calls.
            Printed beside the plan's overhead factor n_windows * t * t / (H * W): time beyond that factor is the tax of tiling.
    kernels hrn_tile_gather + hrn_tile_scatter over the whole plan alone, against their byte floor (each moves its windows once in
            and once out, at the 6.3 TB/s a streaming kernel reaches on an MI355X) and against the same gather and scatter done
            with torch slicing, one copy per window (2 * n_windows small launches instead of 2).
    big     one scene that cannot run whole (default B = 1, V = 32, 2048 x 1536): that it completes, its wall time, and
            torch.cuda.max_memory_allocated against the bound of forward_tiled: the output, one chunk of windows (LR and SR), one
            forward's workspace (plus the input itself).

There is no pass / fail threshold on time.

usage: python tools/tiled_bench.py [--only tax,kernels,big] [--precision P[,P...]] [--tiles 128,256] [--scene B,V,H,W] [--big B,V,H,W]
                                   [--big-tile T] [--rounds R] [--reps N]
"""
import time

import _common
import torch

from _common import HBM_ACHIEVABLE
from oracle import synth, weights            # seeded weights / synthetic inputs only (no oracle arithmetic on the path)
from DeepNetworks.HRNet import HRNet
from hrnet_hip import binding, tiling


PARSER = _common.parser(__doc__, only=["tax", "kernels", "big"], precision=["bf16", "bf16x3"], tiles=[128, 256], scene=[1, 32, 512, 512],
                        big=[1, 32, 2048, 1536], big_tile=128, rounds=5, reps=3)


def _spreads(runs, rounds, reps):
    """{name: fn} -> {name: (median, min, max) microseconds} of the candidates alternating round by round after a warm-up."""
    return {k: _common.spread(v) for k, v in _common.alternate(runs, rounds, reps, warmup=2).items()}


def _scene(seed, B, V, H, W, dev):
    """Synthetic (lrs, alphas) of a (B, V, H, W) scene: fast_batch chips of 256 x 256 laid side by side."""
    side = 256
    ny, nx = -(-H // side), -(-W // side)
    lrs, alphas = synth.fast_batch(seed, B, V, side)
    x = torch.from_numpy(lrs).to(dev).repeat(1, 1, ny, nx)[:, :, :H, :W].contiguous()
    return x, torch.from_numpy(alphas).to(dev)


def _model(prec, dev):
    m = HRNet(weights.HRNET_CONFIG)
    m.load_state_dict(weights.to_torch_state(weights.hrnet_state(1234)))
    m.precision = prec
    return m.to(dev).eval()


def tax(precs, tiles, scene, rounds, reps, dev):
    B, V, H, W = scene
    x, a = _scene(5, B, V, H, W, dev)
    out = []
    for prec in precs:
        m = _model(prec, dev)
        R = tiling.halo(m._num_layers, V)
        runs = {"whole": lambda: m(x, a)}
        for t in tiles:
            runs[f"tile {t}"] = lambda t=t: m.forward_tiled(x, a, t)
        med = _spreads(runs, rounds, reps)
        same = {t: bool(torch.equal(m.forward_tiled(x, a, t), m(x, a))) for t in tiles}
        print(f"tax: B={B} V={V} {H}x{W} {prec}, R={R}, median of {rounds} rounds x {reps} calls:")
        print(f"    whole frame   {med['whole'][0] / 1e3:10.2f} ms   (min {med['whole'][1] / 1e3:.2f}, max {med['whole'][2] / 1e3:.2f})")
        for t in tiles:
            p = tiling.plan(H, W, t, R)
            k = f"tile {t}"
            ratio = med[k][0] / med["whole"][0]
            print(f"    {k:13s} {med[k][0] / 1e3:10.2f} ms   (min {med[k][1] / 1e3:.2f}, max {med[k][2] / 1e3:.2f})   {len(p.windows)} windows, "
                  f"overhead factor {p.overhead:.3f}, time ratio {ratio:.3f}, tax beyond the factor {100 * (ratio / p.overhead - 1):+.1f} %, "
                  f"bit-equal to whole: {same[t]}")
            out.append({"precision": prec, "B": B, "V": V, "H": H, "W": W, "tile": t, "R": R, "windows": len(p.windows),
                        "overhead_factor": p.overhead, "whole_ms": med["whole"][0] / 1e3, "tiled_ms": med[k][0] / 1e3, "ratio": ratio,
                        "bit_equal": same[t]})
    return out


def kernels(tiles, scene, scale, rounds, reps, dev):
    B, V, H, W = scene
    S = scale
    x, _ = _scene(6, B, V, H, W, dev)
    R = tiling.halo(weights.HRNET_CONFIG["encoder"]["num_layers"], V)
    res = []
    for t in tiles:
        p = tiling.plan(H, W, t, R)
        n = len(p.windows)
        srs = torch.rand((n, B, 1, S * t, S * t), device=dev)
        big = torch.empty((B, 1, S * H, S * W), device=dev)
        wins = torch.empty((n, B, V, t, t), device=dev)

        def slice_gather():
            for i, w in enumerate(p.windows):
                wins[i].copy_(x[:, :, w.y0:w.y0 + t, w.x0:w.x0 + t])

        runs = {"gather": lambda: binding.tile_gather(x, t, R, 0, n), "scatter": lambda: binding.tile_scatter(big, srs, t, R, S, 0, n),
                "gather by slicing": slice_gather, "scatter by slicing": lambda: tiling.scatter(big, srs, p.windows, t, S)}
        med = _spreads(runs, rounds, reps)
        g_bytes = 2 * n * B * V * t * t * 4
        s_bytes = 2 * B * S * H * S * W * 4
        print(f"kernels: B={B} V={V} {H}x{W} x{S} tile {t}, R={R}, {n} windows, median of {rounds} rounds x {reps} calls:")
        for k, by in (("gather", g_bytes), ("scatter", s_bytes)):
            floor = by / HBM_ACHIEVABLE * 1e6
            print(f"    {k:8s} {med[k][0]:9.1f} us   (min {med[k][1]:.1f}, max {med[k][2]:.1f})   {by / 1e6:.1f} MB -> byte floor {floor:.1f} us "
                  f"({med[k][0] / floor:.2f}x);   by slicing ({n} copies): {med[k + ' by slicing'][0]:.1f} us ({med[k + ' by slicing'][0] / med[k][0]:.1f}x)")
        res.append({"B": B, "V": V, "H": H, "W": W, "scale": S, "tile": t, "windows": n, "median_us": {k: v[0] for k, v in med.items()},
                    "gather_floor_us": g_bytes / HBM_ACHIEVABLE * 1e6, "scatter_floor_us": s_bytes / HBM_ACHIEVABLE * 1e6})
    return res


def big(precs, scene, tile, dev):
    B, V, H, W = scene
    x, a = _scene(7, B, V, H, W, dev)
    out = []
    for prec in precs:
        m = _model(prec, dev)
        S = m._scale
        R = tiling.halo(m._num_layers, V)
        p = tiling.plan(H, W, tile, R)
        chunk = max(1, 32 // B)
        _, dt = m.packed_parameters()
        ws = binding.load_library().hrn_hrnet_workspace_bytes(dt, chunk * B, V, p.t, p.t)
        whole_ws = binding.load_library().hrn_hrnet_workspace_bytes(dt, B, V, H, W)
        bound = x.numel() * 4 + B * S * H * S * W * 4 + chunk * B * (V + S * S) * p.t * p.t * 4 + ws
        with torch.no_grad():
            m.forward_tiled(x[:, :, :2 * tile, :2 * tile].contiguous(), a, tile)            # warm-up: the chunk's shapes and workspace
            torch.cuda.synchronize()
            before = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            sr = m.forward_tiled(x, a, tile)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
        peak = torch.cuda.max_memory_allocated()
        ok = bool(torch.isfinite(sr).all())
        print(f"big: B={B} V={V} {H}x{W} {prec} tile {tile}, R={R}: {len(p.windows)} windows in chunks of {chunk}, overhead factor "
              f"{p.overhead:.3f}; completed (finite: {ok}), output {tuple(sr.shape)}, wall {wall:.3f} s")
        print(f"    max_memory_allocated {peak / 2**30:.2f} GiB ({before / 2**30:.2f} GiB held before the call: input, parameters, cached "
              f"workspace); bound input + output + one chunk (LR and SR) + one forward's workspace = {bound / 2**30:.2f} GiB; "
              f"a whole-frame forward's workspace alone would be {whole_ws / 2**30:.1f} GiB")
        out.append({"precision": prec, "B": B, "V": V, "H": H, "W": W, "tile": tile, "R": R, "windows": len(p.windows), "wall_s": wall,
                    "max_memory_allocated": peak, "bound_bytes": bound, "whole_frame_workspace_bytes": whole_ws, "finite": ok})
        del sr
    return out


def main():
    o = PARSER.parse_args()
    _common.require_gpu("tiled_bench")
    dev = torch.device("cuda:0")
    result = {}
    with torch.no_grad():
        if "tax" in o.only:
            result["tax"] = tax(o.precision, o.tiles, tuple(o.scene), o.rounds, o.reps, dev)
        if "kernels" in o.only:
            result["kernels"] = kernels(o.tiles, tuple(o.scene), weights.HRNET_CONFIG["decoder"]["deconv"]["stride"], o.rounds, max(o.reps, 10), dev)
        if "big" in o.only:
            result["big"] = big(o.precision, tuple(o.big), o.big_tile, dev)
    _common.emit("tiled_bench", result)


if __name__ == "__main__":
    main()
