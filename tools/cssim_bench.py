#!/usr/bin/env python3
"""Time the shift-searched SSIM's kernels against the torch composition a user would write without them.

At B samples of S x S (default 32 of 192 x 192 and of 384 x 384), border 3, for the gaussian (11 taps) and the uniform (7 taps) window,
this times in ONE process, call by call alternating, after a warm-up:

    cssim_pre      n_k and bias_k of every sample and offset (the pre-pass and its finish)
    cssim_tile     the tile kernel: three filtered fields per offset out of LDS, the SSIM map and its fp64 sums
    cssim_finish   the tiles' sums in index order, the scores and the argmax
    torch          the same definition in torch on the device, one offset at a time: the crops, the bias, five fields filtered by
                   slicing adds along each axis, the SSIM map and its mean, all fp32

The three families' times are the device events the library's profiler (hrn_profile_enable) puts around their launches; the torch
composition's is a pair of device events around one call.  The calls walk over enough input sets to exceed the 256 MB last-level
cache.  A round is `reps` fused calls and `torch_reps` torch calls, alternating; the figure is the median over the rounds, with min and
max as the run-to-run spread.  Printed per size and window: the time per (map pixel, offset) of the fused path, its ratio to the time
of the counted arithmetic - 12 T + 40 flops per (map pixel, offset): three fields, two passes, T multiply-adds, and the SSIM itself - at
the 157.3 TFLOP/s fp32 vector peak of an MI355X, the ratio to the torch composition, and the largest |difference| between the two
paths' scores, taken before anything is timed.  There is no pass / fail threshold on time.

--backward times the gradient of the score as a loss instead, again call by call in one process:

    cssim_bwd_tile     the backward's tile kernel: six fields filtered at the selected offset, alpha', beta, gamma per map pixel, the
                       three filtered back, the raw D and the fp64 sums of m D
    cssim_bwd_finish   the mean M and the elementwise pass that writes d_srs
    cssim_tile         the forward's tile kernel in the same calls, the 49 offsets the backward does not walk
    torch              torch autograd (forward and backward) through the composition of the ONE offset the forward selected

and prints the backward beside the forward's tile kernel and beside torch, and the largest |difference| of the two gradients over
the largest |gradient|.

usage: python tools/cssim_bench.py [B] [--sizes S[,S...]] [--border W] [--windows gaussian,uniform] [--rounds R] [--reps N] [--torch-reps N]
                                   [--backward]
"""
import _common
import torch

from _common import LLC_BYTES
from hrnet_hip import binding

FAMILIES = ("cssim_pre", "cssim_tile", "cssim_finish")
BWD_FAMILIES = ("cssim_bwd_tile", "cssim_bwd_finish")
FP32_VECTOR_PEAK = 157.3e12          # flop / s

OPTIONS = dict(positional=dict(B=32), sizes=[192, 384], border=3, windows=["gaussian", "uniform"], rounds=5, reps=10, torch_reps=2)
PARSER = _common.parser(__doc__, **OPTIONS)                          # what a measurement of either mode takes
CLI = _common.parser(__doc__, backward=False, **OPTIONS)             # the command line: those, and the switch between the modes


def taps_of(window, device):
    if window == "uniform":
        return torch.full((7,), 1.0 / 7.0, device=device), 49.0 / 48.0
    x = torch.arange(-5, 6, dtype=torch.float64)
    g = torch.exp(-x * x / (2 * 1.5 ** 2))
    return (g / g.sum()).float().to(device), 1.0


def filt(a, taps):
    """the separable window over the positions where it fits, by slicing adds"""
    T, (h, w) = len(taps), a.shape[-2:]
    rows = taps[0] * a[:, :h - T + 1]
    for o in range(1, T):
        rows = rows + taps[o] * a[:, o:o + h - T + 1]
    out = taps[0] * rows[:, :, :w - T + 1]
    for o in range(1, T):
        out = out + taps[o] * rows[:, :, o:o + w - T + 1]
    return out


def torch_cssim(srs, hrs, maps, border, taps, cov_norm, data_range=1.0):
    """(B, nk) fp32 scores, -inf where an offset has no clear pixel: what a user writes today"""
    B, H, W = srs.shape
    h, w, nb = H - 2 * border, W - 2 * border, 2 * border + 1
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    s = srs[:, border:border + h, border:border + w].clamp(0.0, 1.0)
    scores = []
    for u in range(nb):
        for v in range(nb):
            g, m = hrs[:, u:u + h, v:v + w], (maps[:, u:u + h, v:v + w] != 0).float()
            n = m.sum((1, 2))
            bias = (m * (g - s)).sum((1, 2)) / n
            X, Y = m * g, m * (s + bias[:, None, None])
            mx, my = filt(X, taps), filt(Y, taps)
            vx = cov_norm * (filt(X * X, taps) - mx * mx)
            vy = cov_norm * (filt(Y * Y, taps) - my * my)
            vxy = cov_norm * (filt(X * Y, taps) - mx * my)
            ssim = ((2 * mx * my + c1) * (2 * vxy + c2)) / ((mx * mx + my * my + c1) * (vx + vy + c2))
            scores.append(torch.where(n > 0, ssim.mean((1, 2)), torch.full_like(n, float("-inf"))))
    return torch.stack(scores, 1)


def torch_cssim_at(srs, hrs, maps, k, border, taps, cov_norm, data_range=1.0):
    """(B,) fp32 scores at the offsets k (B,) int64, differentiable in srs, no clamp: what a user writes to train on the score once the
    offset is known"""
    B, H, W = srs.shape
    h, w, nb = H - 2 * border, W - 2 * border, 2 * border + 1
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    s = srs[:, border:border + h, border:border + w]
    at = lambda t: torch.stack([t[b, int(k[b]) // nb:int(k[b]) // nb + h, int(k[b]) % nb:int(k[b]) % nb + w] for b in range(B)])
    g, m = at(hrs), (at(maps) != 0).float()
    bias = (m * (g - s)).sum((1, 2)) / m.sum((1, 2))
    X, Y = m * g, m * (s + bias[:, None, None])
    mx, my = filt(X, taps), filt(Y, taps)
    vx = cov_norm * (filt(X * X, taps) - mx * mx)
    vy = cov_norm * (filt(Y * Y, taps) - my * my)
    vxy = cov_norm * (filt(X * Y, taps) - mx * my)
    return (((2 * mx * my + c1) * (2 * vxy + c2)) / ((mx * mx + my * my + c1) * (vx + vy + c2))).mean((1, 2))


def bench_backward(B, S, border, window, rounds, reps, torch_reps):
    dev = torch.device("cuda:0")
    nsets = max(2, -(-2 * LLC_BYTES // (16 * B * S * S)))
    gen = torch.Generator(device=dev).manual_seed(S)
    sets = []
    for _ in range(nsets):
        hrs = torch.rand((B, S, S), device=dev, generator=gen)
        srs = 0.9 * hrs + 0.03 + 0.02 * torch.randn((B, S, S), device=dev, generator=gen)
        maps = (torch.rand((B, S, S), device=dev, generator=gen) > 0.15).float()
        sets.append((srs, hrs, maps))
    taps, cov_norm = taps_of(window, dev)
    T = len(taps)
    d_out = torch.ones((B,), device=dev)
    kw = dict(border_w=border, window=window, clip=False)

    def fused(i):
        x = sets[i % nsets]
        _, stats, _ = binding.shift_cssim(*x, with_scores=False, **kw)
        return stats, binding.cssim_loss_backward(*x, stats, d_out, **kw)

    def composed(i, k):
        srs, hrs, maps = sets[i % nsets]
        s = srs.detach().requires_grad_(True)
        torch_cssim_at(s, hrs, maps, k, border, taps, cov_norm).sum().backward()
        return s.grad

    ks = [fused(i)[0][:, 3].long().cpu() for i in range(nsets)]     # read back once, before anything is timed
    want = composed(0, ks[0])
    worst = float((fused(0)[1] - want).abs().max() / want.abs().max())
    torch.cuda.synchronize()
    names = BWD_FAMILIES + ("cssim_tile",)
    per_round = {f: [] for f in names + ("torch",)}
    for r in range(rounds):
        binding.profile_enable(True)
        spent = []
        for i in range(reps):
            fused(r * reps + i)
            if i < torch_reps:
                spent.append(_common.timed_us(lambda: composed(r * reps + i, ks[(r * reps + i) % nsets]), 1))
        torch.cuda.synchronize()
        rec = binding.profile_read()
        binding.profile_enable(False)
        for f in names:
            per_round[f].append(rec[f]["ms"] * 1e3 / rec[f]["launches"])
        per_round["torch"].append(sum(spent) / len(spent))
    res = {"mode": "backward", "B": B, "S": S, "border": border, "window": window, "taps": T, "input_sets": nsets, "rounds": rounds,
           "reps": reps, "torch_reps": torch_reps, "max_rel_diff_vs_torch": worst}
    print(f"backward B={B} {S}x{S} border {border} {window} ({T} taps): median of {rounds} rounds x {reps} calls over {nsets} input sets "
          f"(fused vs torch autograd: max |difference| {worst:.1e} of the max |gradient|)")
    for f in per_round:
        med, lo, hi = _common.spread(per_round[f])
        res[f] = {"median_us": med, "min_us": lo, "max_us": hi}
        print(f"    {f:17s} {med:11.1f} us   (min {lo:.1f}, max {hi:.1f})")
    total = sum(res[f]["median_us"] for f in BWD_FAMILIES)
    res.update(backward_us=total, backward_over_forward_tile=total / res["cssim_tile"]["median_us"],
               torch_over_backward=res["torch"]["median_us"] / total, ns_per_pixel=total * 1e3 / (B * S * S))
    print(f"    backward total {total:.1f} us = {res['ns_per_pixel'] * 1e3:.1f} ps per pixel = {res['backward_over_forward_tile']:.3f} x the "
          f"forward's cssim_tile;  torch autograd at the selected offset / backward: {res['torch_over_backward']:.1f} x")
    return res


def bench(B, S, border, window, rounds, reps, torch_reps):
    dev = torch.device("cuda:0")
    nsets = max(2, -(-2 * LLC_BYTES // (12 * B * S * S)))
    gen = torch.Generator(device=dev).manual_seed(S)
    sets = []
    for _ in range(nsets):
        hrs = torch.rand((B, S, S), device=dev, generator=gen)
        srs = 0.9 * hrs + 0.03 + 0.02 * torch.randn((B, S, S), device=dev, generator=gen)
        maps = (torch.rand((B, S, S), device=dev, generator=gen) > 0.15).float()
        sets.append((srs, hrs, maps))
    taps, cov_norm = taps_of(window, dev)
    T, nk = len(taps), (2 * border + 1) ** 2
    units = B * (S - 2 * border - T + 1) ** 2 * nk                  # (map pixel, offset) pairs of a call

    fused = lambda i: binding.shift_cssim(*sets[i % nsets], border_w=border, window=window, clip=True)
    composed = lambda i: torch_cssim(*sets[i % nsets], border, taps, cov_norm)

    worst = float((fused(0)[2] - composed(0).double()).abs().max())  # the two paths score alike before either is timed
    for i in range(nsets):
        fused(i)
    composed(1)
    torch.cuda.synchronize()
    per_round = {f: [] for f in FAMILIES + ("torch",)}
    for r in range(rounds):
        binding.profile_enable(True)
        spent = []
        for i in range(reps):
            fused(r * reps + i)
            if i < torch_reps:
                spent.append(_common.timed_us(lambda: composed(r * reps + i), 1))
        torch.cuda.synchronize()
        rec = binding.profile_read()
        binding.profile_enable(False)
        for f in FAMILIES:
            per_round[f].append(rec[f]["ms"] * 1e3 / rec[f]["launches"])
        per_round["torch"].append(sum(spent) / len(spent))
    res = {"B": B, "S": S, "border": border, "window": window, "taps": T, "input_sets": nsets, "rounds": rounds, "reps": reps,
           "torch_reps": torch_reps, "max_abs_diff_vs_torch": worst}
    print(f"B={B} {S}x{S} border {border} {window} ({T} taps): median of {rounds} rounds x {reps} calls over {nsets} input sets "
          f"(fused vs torch composition: max |difference| {worst:.1e})")
    for f in per_round:
        med, lo, hi = _common.spread(per_round[f])
        res[f] = {"median_us": med, "min_us": lo, "max_us": hi}
        print(f"    {f:13s} {med:11.1f} us   (min {lo:.1f}, max {hi:.1f})")
    total = sum(res[f]["median_us"] for f in FAMILIES)
    at_peak = units * (12.0 * T + 40.0) / FP32_VECTOR_PEAK * 1e6
    res.update(fused_us=total, ps_per_pixel_offset=total * 1e6 / units, flops_at_peak_us=at_peak, times_flop_floor=total / at_peak,
               torch_over_fused=res["torch"]["median_us"] / total)
    print(f"    fused total {total:.1f} us = {res['ps_per_pixel_offset']:.2f} ps per (map pixel, offset) = {res['times_flop_floor']:.1f} x the "
          f"{at_peak:.1f} us of its {12 * T + 40} flops at the fp32 vector peak;  torch composition / fused: {res['torch_over_fused']:.1f} x")
    return res


def main():
    o = CLI.parse_args()
    _common.require_gpu("cssim_bench")
    run = bench_backward if o.backward else bench
    _common.emit("cssim_bench", [run(o.B, S, o.border, w, o.rounds, o.reps, o.torch_reps) for S in o.sizes for w in o.windows])


if __name__ == "__main__":
    main()
