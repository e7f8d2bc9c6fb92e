#!/usr/bin/env python3
"""Time shift-and-add: hrn_shift_add and hrn_shift_add_backward.

In ONE process, after a warm-up, at (B, V, H, W) = (32, 32, 128, 128) and at one (1, 32, 2048, 1536) scene, both x3, masks 30 % hidden,
shifts within 1.5 px, a base given, sigma 0.25, prior 0.05:

    forward          hrn_shift_add, weight NULL:    4 (2 BVHW + 2 S^2 BHW) bytes (views and masks in, base in, out written)
    forward_weight   hrn_shift_add with weight:     4 (2 BVHW + 3 S^2 BHW) bytes
    backward         hrn_shift_add_backward, both:  4 (2 BVHW + 3 S^2 BHW) bytes (d_out and weight in, masks in, d_views and d_base out)
    torch_*          the same definition composed in torch on the device: per axis four gathers of every view weighted by the tap
                     weights, a (B,V,SH,SW) intermediate, the sum over the views, the division; the backward is autograd through it

A kernel's time is the pair of device events the library's profiler (hrn_profile_enable) puts around its launches; the calls walk over
enough input sets to exceed the 256 MB last-level cache, so the bytes come from HBM.  The torch calls are timed with a pair of device
events around one call.  A round is `reps` calls of each; the figure is the median over the rounds, with min and max as the run-to-run
spread.  The byte floors are the algorithmic bytes at the 6.3 TB/s a streaming kernel reaches on an MI355X.  Before anything is timed
the kernels' results are compared with the composition's.  There is no pass / fail threshold on time.

usage: python tools/shift_add_bench.py [--rounds R] [--reps N]
"""
import math

import _common
import torch

from _common import HBM_ACHIEVABLE, LLC_BYTES
from hrnet_hip import binding

PARSER = _common.parser(__doc__, rounds=7, reps=10)
CASES = [(32, 32, 128, 128, 3), (1, 32, 2048, 1536, 3)]          # (B, V, H, W, scale)
SIGMA, PRIOR = 0.25, 0.05


def floor_us(B, V, H, W, scale, what):
    """the byte floor in microseconds.  forward: views and masks read once, base read, out written; forward_weight: weight written too;
    backward: d_out and weight read, masks read, d_views and d_base written"""
    lr, sr = B * V * H * W, B * H * W * scale * scale
    return 4.0 * (2 * lr + {"forward": 2, "forward_weight": 3, "backward": 3}[what] * sr) / HBM_ACHIEVABLE * 1e6


def taps(shift, S, sigma):
    """shift (...,) f32 -> (n (..., S) long, w (..., S, 4) f32): the library's tap indices and weights (include/hrnet_hip.h)"""
    t = (torch.arange(S, dtype=torch.float64, device=shift.device) + 0.5) / S - 0.5
    d = (t + shift.double()[..., None]).float().clamp(-256.0, 256.0)
    n = torch.floor(d)
    u = torch.arange(-1, 3, dtype=torch.float64, device=shift.device) - (d.double() - n.double())[..., None]
    k = torch.exp(-(u * u) / (2.0 * float(sigma) ** 2)) * torch.cos(math.pi * u / 4.0) ** 2
    k = torch.where((u.abs() < 2.0) & (k >= 2.0 ** -60), k, torch.zeros_like(k))
    return n.long(), k.float()


def _axis(x, n, w):
    """x (B,V,L,K) -> (B,V,S L,K): the four taps of every output index along dim 2, gathered and weighted"""
    B, V, L, K = x.shape
    S = n.shape[-1]
    rows = torch.arange(L, device=x.device)[:, None] + n[:, :, None, :]                # (B,V,L,S): m + n_p
    out = None
    for o in range(4):
        idx = (rows + (o - 1)).reshape(B, V, L * S)
        ok = (idx >= 0) & (idx < L)
        wv = w[:, :, None, :, o].expand(B, V, L, S).reshape(B, V, L * S) * ok
        term = torch.gather(x, 2, idx.clamp(0, L - 1)[..., None].expand(B, V, L * S, K)) * wv[..., None]
        out = term if out is None else out + term
    return out


def torch_shift_add(views, masks, alphas, shifts, base, S, sigma, prior):
    """-> (out, weight): hrn_shift_add's definition composed in torch, fp32"""
    counts = torch.isfinite(shifts).all(-1)
    if alphas is not None:
        counts = counts & (alphas != 0)
    m = counts[..., None, None].float().expand_as(views) if masks is None else (masks != 0).float() * counts[..., None, None]
    mx = torch.where(m != 0, views, torch.zeros_like(views))
    sh = torch.where(counts[..., None], shifts, torch.zeros_like(shifts))
    (ny, wy), (nx, wx) = taps(sh[..., 0], S, sigma), taps(sh[..., 1], S, sigma)
    both = lambda x: _axis(_axis(x, ny, wy).transpose(2, 3), nx, wx).transpose(2, 3).sum(1)
    N, D = both(mx), both(m)
    den = D + prior
    b = torch.zeros_like(N) if base is None else base
    return torch.where(den >= 2.0 ** -20, (N + prior * b) / den, b), D


def _kernel_us(family, call, nsets, rounds, reps):
    for i in range(nsets):
        call(i)
    torch.cuda.synchronize()
    out = []
    for r in range(rounds):
        binding.profile_enable(True)
        for i in range(reps):
            call(r * reps + i)
        torch.cuda.synchronize()
        rec = binding.profile_read()[family]
        binding.profile_enable(False)
        out.append(rec["ms"] * 1e3 / reps)                  # per call: the backward is two launches inside one pair of events
    return out


def bench_case(B, V, H, W, S, rounds, reps):
    dev = torch.device("cuda:0")
    lr, sr = B * V * H * W, B * H * W * S * S
    per_set = 4 * (2 * lr + 4 * sr)
    nsets = min(16, max(2, -(-2 * LLC_BYTES // per_set)))
    gen = torch.Generator(device=dev).manual_seed(S)
    views = [torch.rand((B, V, H, W), device=dev, generator=gen) for _ in range(nsets)]
    masks = [(torch.rand((B, V, H, W), device=dev, generator=gen) >= 0.3).float() for _ in range(nsets)]
    bases = [torch.rand((B, S * H, S * W), device=dev, generator=gen) for _ in range(nsets)]
    gs = [torch.rand((B, S * H, S * W), device=dev, generator=gen) - 0.5 for _ in range(nsets)]
    shifts = (torch.rand((B, V, 2), device=dev, generator=gen) * 3.0 - 1.5).contiguous()
    outs = [torch.empty((B, S * H, S * W), device=dev) for _ in range(2)]
    fwd = lambda i, w: binding.shift_add(views[i % nsets], masks[i % nsets], None, shifts, bases[i % nsets], S, SIGMA, PRIOR, want_weight=w,
                                         out=outs[i % 2])
    # what is timed computes what the composition computes (fp32 against fp32: 1e-5 of the sums of absolute terms, <= 1 and <= 2^20 / 20)
    vr, br = views[0].clone().requires_grad_(True), bases[0].clone().requires_grad_(True)
    t_out, t_w = torch_shift_add(vr, masks[0], None, shifts, br, S, SIGMA, PRIOR)
    k_out, k_w = fwd(0, True)
    assert torch.allclose(k_out, t_out.detach(), rtol=0, atol=2e-5) and torch.allclose(k_w, t_w.detach(), rtol=1e-5, atol=0)
    weights = [fwd(i, True)[1] for i in range(nsets)]
    bwd = lambda i: binding.shift_add_backward(gs[i % nsets], weights[i % nsets], masks[i % nsets], None, shifts, V, H, W, S, SIGMA, PRIOR)
    t_dv, t_db = torch.autograd.grad(t_out, (vr, br), gs[0], retain_graph=True)
    k_dv, k_db = bwd(0)
    assert torch.allclose(k_dv, t_dv, rtol=0, atol=2e-4) and torch.allclose(k_db, t_db, rtol=0, atol=2e-5)
    res = {"B": B, "V": V, "H": H, "W": W, "scale": S, "input_sets": nsets, "rounds": rounds, "reps": reps}
    t_fwd = lambda i: torch_shift_add(views[i % nsets], masks[i % nsets], None, shifts, bases[i % nsets], S, SIGMA, PRIOR)
    runs = {
        "forward": ("shift_add", lambda i: fwd(i, False), lambda i: t_fwd(i)[0]),
        "forward_weight": ("shift_add", lambda i: fwd(i, True), t_fwd),
        "backward": ("shift_add_backward", bwd, lambda i: torch.autograd.grad(t_out, (vr, br), gs[i % nsets], retain_graph=True)),
    }
    print(f"({B}, {V}, {H}, {W}) -> x{S}: median of {rounds} rounds x {reps} calls over {nsets} input sets")
    for name, (family, call, tcall) in runs.items():
        kern = _kernel_us(family, call, nsets, rounds, reps)
        with torch.no_grad() if name != "backward" else torch.enable_grad():
            for i in range(2):
                tcall(i)
            comp = [_common.timed_us(lambda: tcall(r), 1) for r in range(rounds * 2)]
        floor = floor_us(B, V, H, W, S, name)
        (med, lo, hi), (tmed, tlo, thi) = _common.spread(kern), _common.spread(comp)
        res[name] = {"median_us": med, "min_us": lo, "max_us": hi, "floor_us": floor}
        res["torch_" + name] = {"median_us": tmed, "min_us": tlo, "max_us": thi}
        print(f"    {name:15s} {med:9.1f} us   (min {lo:.1f}, max {hi:.1f})   byte floor {floor:.1f} us = {100 * floor / med:.0f} % of it;"
              f"   torch {tmed:9.1f} us (min {tlo:.1f}, max {thi:.1f}) = {tmed / med:.1f} x")
    return res


def main():
    o = PARSER.parse_args()
    _common.require_gpu("shift_add_bench")
    _common.emit("shift_add_bench", [bench_case(B, V, H, W, S, o.rounds, o.reps) for B, V, H, W, S in CASES])


if __name__ == "__main__":
    main()
