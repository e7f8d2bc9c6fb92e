#!/usr/bin/env python3
"""Time the searched loss's kernels against the scorer they generalise, and the searched L1 / Charbonnier loss's
beside them.

At B samples of S x S (default 32 of 192 x 192 and of 384 x 384: the x3 training patch and the evaluation scene), border 3, this times in
ONE process, call by call alternating, after a warm-up:

    shift_loss_fwd   hrn_shift_loss_train      every pixel of srs / hrs / maps once, the 49 offsets out of LDS: 12 B S^2 bytes
    shift_loss_bwd   hrn_shift_loss_backward   one elementwise pass: 16 B S^2 bytes
    shift_cpsnr      hrn_shift_cpsnr           the unchanged scorer: 49 workgroups per sample, each re-reading the sample out of L2
    cl1_fwd          hrn_cl1_loss_train        the two walks of the L1 loss (eps = 0), each reading the three images: 24 B S^2 bytes
    cl1_bwd          hrn_cl1_loss_backward     one elementwise pass: 16 B S^2 bytes

and, in a window of their own in every round, cl1_fwd / cl1_bwd at eps = 1e-3 (Charbonnier: `cl1_fwd_charbonnier`, `cl1_bwd_charbonnier`),
and `torch_cl1` / `torch_cl1_charbonnier`: the same definition's forward composed in torch on the device, one offset at a time in fp32
(what a user writes without the kernel), a pair of device events around each of --torch-reps calls.

In windows of their own in every round, the sub-pixel searched loss (P = 7, 4 levels, radius 3) on the same inputs:

    subpixel_fwd       hrn_subpixel_loss_train     m0, the means, four levels of the scene search's level body and the cMSE finish
    subpixel_bwd       hrn_subpixel_loss_backward  the residual's tile kernel and the sampler's adjoint
    mncc_search_scene  hrn_mncc_search_scene       the masked-NCC search with the same P and levels on the same pixels (V = 1)

and `subpixel_step` / `composed_step`: a forward and a backward of `losses.subpixel_loss` beside the composition it replaces
(`mncc_search_scene`, `warp`, the masked brightness-corrected MSE in torch, autograd), a pair of device events around each of --torch-reps
calls of either, alternating.

Each call's time is the pair of device events the library's profiler (hrn_profile_enable) puts around its launches, so the Python
between two calls is not in it.  The calls walk over enough input sets to exceed the 256 MB last-level cache, so the bytes come from
HBM.  A round is `reps` calls of each; the figure is the median over the rounds, with min and max as the run-to-run spread.  The byte
floors are the algorithmic bytes at the 6.3 TB/s a streaming kernel reaches on an MI355X (8 TB/s peak).  There is no pass / fail
threshold on time.

usage: python tools/shift_loss_bench.py [B] [--sizes S[,S...]] [--border W] [--rounds R] [--reps N] [--torch-reps N]
"""
import _common
import torch

from _common import HBM_ACHIEVABLE, LLC_BYTES
from hrnet_hip import binding

FAMILIES = ("shift_loss_fwd", "shift_loss_bwd", "shift_cpsnr", "cl1_fwd", "cl1_bwd")
CL1 = ("cl1_fwd", "cl1_bwd")
SUBPIXEL = ("subpixel_fwd", "subpixel_bwd", "mncc_search_scene")
SUBPIXEL_SEARCH = dict(points_per_dim=7, levels=4, radius=3.0)
CHARBONNIER_EPS = 1e-3


PARSER = _common.parser(__doc__, positional=dict(B=32), sizes=[192, 384], border=3, rounds=7, reps=20, torch_reps=2)


def floors_us(B, S):
    """the byte floors of the forward (12 B S^2) and the backward (16 B S^2) in microseconds"""
    return 12.0 * B * S * S / HBM_ACHIEVABLE * 1e6, 16.0 * B * S * S / HBM_ACHIEVABLE * 1e6


def torch_cl1(srs, hrs, maps, border, eps):
    """(B,) fp32: the searched L1 / Charbonnier composed in torch, one offset at a time; +inf where an offset has no clear pixel"""
    B, H, W = srs.shape
    h, w, nb = H - 2 * border, W - 2 * border, 2 * border + 1
    s = srs[:, border:border + h, border:border + w].clamp(0.0, 1.0)
    values = []
    for u in range(nb):
        for v in range(nb):
            g, m = hrs[:, u:u + h, v:v + w], maps[:, u:u + h, v:v + w]
            n = m.sum((1, 2))
            e = s + ((m * (g - s)).sum((1, 2)) / n)[:, None, None] - g
            rho = e.abs() if eps == 0 else torch.sqrt(e * e + eps * eps)
            values.append(torch.where(n > 0, (m * rho).sum((1, 2)) / n, torch.full_like(n, float("inf"))))
    return torch.stack(values, 1).min(1).values


def composed_loss(srs, hrs, maps, border):
    """(B,) fp32: -cPSNR of srs registered to hrs, as INTEGRATION.md composed it before hrnet_hip.losses.subpixel_loss: the masked-NCC
    search, `warp`, the brightness-corrected masked MSE in torch; autograd reaches srs through warp"""
    from hrnet_hip import registration
    crop = torch.zeros_like(maps)
    crop[:, border:maps.shape[1] - border, border:maps.shape[2] - border] = 1.0
    m0 = (maps != 0).float() * crop
    shifts = registration.mncc_search_scene(srs.detach()[:, None], None, ref=hrs, ref_mask=m0, **SUBPIXEL_SEARCH)[:, 0]
    warped, valid = registration.warp(srs, shifts)
    m = m0 * valid
    n = m.sum((1, 2))
    b = ((m * (hrs - warped)).sum((1, 2)) / n).detach()
    return 10.0 * torch.log10((m * (warped + b[:, None, None] - hrs) ** 2).sum((1, 2)) / n)


def bench_subpixel(sets, border, rounds, reps, torch_reps):
    """-> {name: [microseconds per call, one per round]} of SUBPIXEL and of the two training tails"""
    from hrnet_hip import losses
    nsets = len(sets)
    B = sets[0][0].shape[0]
    d_out = torch.full((B,), -1.0 / B, device=sets[0][0].device)
    P, levels, radius = SUBPIXEL_SEARCH["points_per_dim"], SUBPIXEL_SEARCH["levels"], SUBPIXEL_SEARCH["radius"]

    def kernels(i):
        s, h, m = sets[i % nsets]
        out, stats, _ = binding.subpixel_loss_train(s, h, m, "cPSNR", border, P, levels, radius)
        binding.subpixel_loss_backward(s, h, m, stats, d_out, "cPSNR", border)
        binding.mncc_search_scene(h, m, s[:, None], None, P, levels, radius)

    def step(fn, i):
        s, h, m = sets[i % nsets]
        x = s.detach().requires_grad_(True)
        fn(x, h, m).mean().backward()

    tails = {"subpixel_step": lambda x, h, m: -losses.subpixel_loss(x, h, m, "cPSNR", border, **SUBPIXEL_SEARCH),
             "composed_step": lambda x, h, m: composed_loss(x, h, m, border)}
    for i in range(2):
        kernels(i)
        for fn in tails.values():
            step(fn, i)
    torch.cuda.synchronize()
    per_round = {f: [] for f in SUBPIXEL + tuple(tails)}
    for r in range(rounds):
        binding.profile_enable(True)
        for i in range(reps):
            kernels(r * reps + i)
        torch.cuda.synchronize()
        rec = binding.profile_read()
        binding.profile_enable(False)
        for f in SUBPIXEL:
            per_round[f].append(rec[f]["ms"] * 1e3 / rec[f]["launches"])
        for name, fn in tails.items():
            spent = [_common.timed_us(lambda: step(fn, r * torch_reps + i), 1) for i in range(torch_reps)]
            per_round[name].append(sum(spent) / len(spent))
    return per_round


def bench(B, S, border, rounds, reps, torch_reps=2):
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
        cl1(i, 0.0)
        return out, old

    def cl1(i, eps):
        s, h, m = sets[i % nsets]
        out, stats = binding.cl1_loss_train(s, h, m, border, True, eps)
        binding.cl1_loss_backward(s, h, m, stats, d_out, border, True, eps)
        return out

    out, old = one(0)
    worst = float(((out - old).abs() / old.abs()).max())        # the two forwards score alike before either is timed
    cl1_worst = max(float(((cl1(0, eps) - torch_cl1(*sets[0], border, eps)).abs() / cl1(0, eps).abs()).max()) for eps in (0.0, CHARBONNIER_EPS))
    for i in range(2 * nsets):
        one(i)
        cl1(i, CHARBONNIER_EPS)
    torch.cuda.synchronize()
    names = FAMILIES + tuple(f + "_charbonnier" for f in CL1) + ("torch_cl1", "torch_cl1_charbonnier")
    per_round = {f: [] for f in names}
    for r in range(rounds):
        binding.profile_enable(True)
        for i in range(reps):
            one(r * reps + i)
        torch.cuda.synchronize()
        rec = binding.profile_read()
        binding.profile_enable(False)
        for f in FAMILIES:
            per_round[f].append(rec[f]["ms"] * 1e3 / rec[f]["launches"])
        binding.profile_enable(True)                            # Charbonnier in a window of its own: the family names are the same
        for i in range(reps):
            cl1(r * reps + i, CHARBONNIER_EPS)
        torch.cuda.synchronize()
        rec = binding.profile_read()
        binding.profile_enable(False)
        for f in CL1:
            per_round[f + "_charbonnier"].append(rec[f]["ms"] * 1e3 / rec[f]["launches"])
        for name, eps in (("torch_cl1", 0.0), ("torch_cl1_charbonnier", CHARBONNIER_EPS)):
            spent = [_common.timed_us(lambda: torch_cl1(*sets[(r * torch_reps + i) % nsets], border, eps), 1) for i in range(torch_reps)]
            per_round[name].append(sum(spent) / len(spent))
    subpixel = bench_subpixel(sets, border, rounds, reps, torch_reps)
    fwd_floor, bwd_floor = floors_us(B, S)
    res = {"B": B, "S": S, "border": border, "input_sets": nsets, "rounds": rounds, "reps": reps, "torch_reps": torch_reps,
           "fwd_vs_shift_cpsnr_rel": worst, "cl1_fwd_vs_torch_rel": cl1_worst, "fwd_floor_us": fwd_floor, "bwd_floor_us": bwd_floor,
           "cl1_fwd_floor_us": 2 * fwd_floor}
    print(f"B={B} {S}x{S} border {border}: median of {rounds} rounds x {reps} calls over {nsets} input sets "
          f"(forward vs hrn_shift_cpsnr: {worst:.1e} relative; hrn_cl1_loss_train vs its fp32 torch composition: {cl1_worst:.1e} relative)")
    for f in names:
        med, lo, hi = _common.spread(per_round[f])
        res[f] = {"median_us": med, "min_us": lo, "max_us": hi}
        if f.startswith("torch"):
            print(f"    {f:22s} {med:9.1f} us   (min {lo:.1f}, max {hi:.1f})")
            continue
        floor = bwd_floor if "_bwd" in f else 2 * fwd_floor if f.startswith("cl1_fwd") else fwd_floor
        print(f"    {f:22s} {med:9.1f} us   (min {lo:.1f}, max {hi:.1f})   byte floor {floor:.1f} us = "
              f"{100 * floor / med:.0f} % of it")
    print(f"    hrn_shift_cpsnr / hrn_shift_loss_train: {res['shift_cpsnr']['median_us'] / res['shift_loss_fwd']['median_us']:.2f} x")
    for tag in ("", "_charbonnier"):
        fwd = res["cl1_fwd" + tag]["median_us"]
        res["cl1_fwd" + tag + "_over_shift_loss_fwd"] = fwd / res["shift_loss_fwd"]["median_us"]
        res["torch_cl1" + tag + "_over_cl1_fwd"] = res["torch_cl1" + tag]["median_us"] / fwd
        print(f"    hrn_cl1_loss_train{' (eps 1e-3)' if tag else ''} / hrn_shift_loss_train: {res['cl1_fwd' + tag + '_over_shift_loss_fwd']:.2f} x;  "
              f"torch composition / hrn_cl1_loss_train: {res['torch_cl1' + tag + '_over_cl1_fwd']:.1f} x")
    for f, values in subpixel.items():
        med, lo, hi = _common.spread(values)
        res[f] = {"median_us": med, "min_us": lo, "max_us": hi}
        print(f"    {f:22s} {med:9.1f} us   (min {lo:.1f}, max {hi:.1f})")
    res["subpixel_fwd_over_mncc_search_scene"] = res["subpixel_fwd"]["median_us"] / res["mncc_search_scene"]["median_us"]
    res["composed_step_over_subpixel_step"] = res["composed_step"]["median_us"] / res["subpixel_step"]["median_us"]
    print(f"    hrn_subpixel_loss_train / hrn_mncc_search_scene: {res['subpixel_fwd_over_mncc_search_scene']:.2f} x;  "
          f"composed forward + backward / subpixel_loss forward + backward: {res['composed_step_over_subpixel_step']:.2f} x")
    return res


def main():
    o = PARSER.parse_args()
    _common.require_gpu("shift_loss_bench")
    _common.emit("shift_loss_bench", [bench(o.B, S, o.border, o.rounds, o.reps, o.torch_reps) for S in o.sizes])


if __name__ == "__main__":
    main()
