#!/usr/bin/env python3
"""Time the masked composite and the forward that is given its frame.

At B samples of V views of S x S (default 32 x 32 of 128 x 128), in ONE process, call by call alternating, after a warm-up:

    composite_n{9,32}          hrn_masked_composite, ref and count only: 4 B HW (n + n + 2) bytes per sample, n = min(V, n_ref)
    composite_n{9,32}_filled   the same with `filled`: 4 B HW (2 V + V + 2) bytes per sample
    torch_n{9,32}[_filled]     the same definition composed in torch on the device: +inf for the views that do not vote, torch.sort, a
                               gather at (c - 1) // 2, the two fall-backs by torch.where (what a user writes without the kernel)
    forward / forward_ref      HRNet.forward(lrs, alphas) and HRNet.forward(lrs, alphas, ref=ref) of the same batch, per --precision

The composite's time is the pair of device events the library's profiler (hrn_profile_enable) puts around its launch; the calls walk over
enough input sets to exceed the 256 MB last-level cache, so the bytes come from HBM.  The torch composition and the forwards are timed
with a pair of device events around `reps` calls.  A round is `reps` calls of each; the figure is the median over the rounds, with min
and max as the run-to-run spread.  The byte floors are the algorithmic bytes at the 6.3 TB/s a streaming kernel reaches on an MI355X.
Before anything is timed the kernel's ref / count / filled are compared with the torch composition's, bit for bit.  There is no pass /
fail threshold on time.

usage: python tools/composite_bench.py [B V S] [--n-ref N[,N...]] [--precision P[,P...]] [--rounds R] [--reps N] [--torch-reps N]
"""
import _common
import torch

from _common import HBM_ACHIEVABLE, LLC_BYTES
from hrnet_hip import binding

PARSER = _common.parser(__doc__, group=("B V S", (32, 32, 128)), n_ref=[9, 32], precision=["bf16", "bf16x3"], rounds=7, reps=10, torch_reps=2)


def floor_us(B, V, S, n, filled):
    """the byte floor in microseconds: views and masks of the n voters in, ref and count out; with `filled` all V views in and out"""
    per_px = 4.0 * ((2 * V + V + 2) if filled else (n + n + 2))
    return per_px * B * S * S / HBM_ACHIEVABLE * 1e6


def torch_composite(views, masks, alphas, n_ref, fill):
    """(ref, count, filled or None): the definition of hrn_masked_composite composed in torch (sort with +inf fill)"""
    B, V, H, W = views.shape
    n = min(V, n_ref)
    real = (alphas[:, :n] != 0)[:, :, None, None]
    cand = real & (masks[:, :n] != 0)
    c = cand.sum(1)
    vote = torch.where((c > 0)[:, None], cand, torch.where(real.any(1, keepdim=True), real.expand_as(cand), torch.ones_like(cand)))
    keys = torch.where(vote, views[:, :n], torch.full_like(views[:, :n], float("inf"))).sort(1).values
    ref = keys.gather(1, ((vote.sum(1) - 1) // 2)[:, None])[:, 0]
    filled = torch.where((alphas != 0)[:, :, None, None] & (masks == 0), ref[:, None], views) if fill else None
    return ref, c.float(), filled


def bench(B, V, S, n_refs, precisions, rounds, reps, torch_reps):
    dev = torch.device("cuda:0")
    nsets = max(2, -(-2 * LLC_BYTES // (12 * B * V * S * S)))
    gen = torch.Generator(device=dev).manual_seed(S)
    sets = []
    for _ in range(nsets):
        views = torch.floor(torch.rand((B, V, S, S), device=dev, generator=gen) * 16384.0) / 65535.0
        masks = (torch.rand((B, V, S, S), device=dev, generator=gen) < 0.6).float()
        alphas = (torch.arange(V, device=dev)[None] < torch.randint(max(1, V // 2), V + 1, (B, 1), device=dev, generator=gen)).float()
        sets.append((views, masks, alphas))
    res = {"B": B, "V": V, "S": S, "input_sets": nsets, "rounds": rounds, "reps": reps, "torch_reps": torch_reps}
    for n_ref in n_refs:                                         # what is timed computes what the definition says
        got = binding.masked_composite(*sets[0], n_ref, True, True)
        want = torch_composite(*sets[0], n_ref, True)
        assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[1]) and torch.equal(got[1], want[2]), n_ref
    print(f"B={B} V={V} {S}x{S}: median of {rounds} rounds x {reps} calls over {nsets} input sets (kernel == torch composition, bit for bit)")
    for n_ref in n_refs:
        n = min(V, n_ref)
        for fill in (False, True):
            tag = f"n{n_ref}" + ("_filled" if fill else "")
            call = lambda i: binding.masked_composite(*sets[i % nsets], n_ref, True, fill)
            for i in range(nsets):
                call(i)
            torch.cuda.synchronize()
            kern, comp = [], []
            for r in range(rounds):
                binding.profile_enable(True)
                for i in range(reps):
                    call(r * reps + i)
                torch.cuda.synchronize()
                rec = binding.profile_read()["masked_composite"]
                binding.profile_enable(False)
                kern.append(rec["ms"] * 1e3 / rec["launches"])
                spent = [_common.timed_us(lambda: torch_composite(*sets[(r * torch_reps + i) % nsets], n_ref, fill), 1) for i in range(torch_reps)]
                comp.append(sum(spent) / len(spent))
            floor = floor_us(B, V, S, n, fill)
            (med, lo, hi), (tmed, tlo, thi) = _common.spread(kern), _common.spread(comp)
            res["composite_" + tag] = {"median_us": med, "min_us": lo, "max_us": hi, "floor_us": floor}
            res["torch_" + tag] = {"median_us": tmed, "min_us": tlo, "max_us": thi}
            print(f"    composite_{tag:12s} {med:9.1f} us   (min {lo:.1f}, max {hi:.1f})   byte floor {floor:.1f} us = {100 * floor / med:.0f} % of it;"
                  f"   torch composition {tmed:9.1f} us (min {tlo:.1f}, max {thi:.1f}) = {tmed / med:.1f} x")
    # the forward given its frame beside the plain forward of the same batch
    _common.tests_on_path()
    import util
    views, masks, alphas = sets[0]
    ref, filled, _ = binding.masked_composite(views, masks, alphas, 9, False, True)
    for prec in precisions:
        m = util.hip_hrnet(prec)
        with torch.no_grad():
            times = _common.alternate({"forward": lambda: m(filled, alphas), "forward_ref": lambda: m(filled, alphas, ref=ref)}, rounds, reps, 2)
        for name, t in times.items():
            med, lo, hi = _common.spread(t)
            res[f"{name}_{prec}"] = {"median_us": med, "min_us": lo, "max_us": hi}
            print(f"    {name + ' ' + prec:24s} {med / 1e3:9.3f} ms   (min {lo / 1e3:.3f}, max {hi / 1e3:.3f})")
    return res


def main():
    o = PARSER.parse_args()
    _common.require_gpu("composite_bench")
    _common.emit("composite_bench", [bench(o.B, o.V, o.S, o.n_ref, o.precision, o.rounds, o.reps, o.torch_reps)])


if __name__ == "__main__":
    main()
