#!/usr/bin/env python3
"""Time the guarded optimiser step against the plain fused Adam and against its composition in torch.

For the parameters of HRNet + ShiftNet (34.78 M) and of HRNet alone (0.59 M, what a searched loss trains), in ONE process, round by round
alternating, after a warm-up:

    plain        hrn_adam_step                                         16 B read + 12 B written per parameter
    guard        hrn_grad_sumsq + hrn_optim_prepare + hrn_adam_step_ex  + 4 B read (the gradient, once more): 32 / 28 of plain
    clip         the same with max_grad_norm below the gradient's norm (the coefficient is printed)
    decoupled    clip + decoupled weight decay (AdamW)
    ema          decoupled + the EMA of the weights                    + 4 B read + 4 B written: 40 / 28 of plain
    torch        torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW (foreach) + torch.optim.swa_utils' EMA, tensor by tensor over the same shapes

The first five run through the dispatcher ops, as FusedAdam.step() calls them, on flat buffers; `torch` on one tensor per parameter.  Every
candidate walks over enough copies of its buffers to exceed the 256 MB last-level cache, as the buffers of a training step do that has
run a forward and a backward pass since the last update.  A round is `reps` steps of each, timed by one pair of device events (the Python
between the launches is in it, as it is in training); the figure is the median over the rounds, with min and max as the run-to-run
spread.  There is no pass / fail threshold on time.

usage: python tools/optim_bench.py [--models both,hrnet] [--rounds R] [--reps N] [--warmup N]
"""
import _common
import torch

from _common import HBM_ACHIEVABLE, LLC_BYTES

PARSER = _common.parser(__doc__, models=["both", "hrnet"], rounds=7, reps=10, warmup=3)
LR, BETAS, EPS, WD, MAX_NORM, DECAY = 1e-4, (0.9, 0.999), 1e-8, 1e-2, 1.0, 0.999
BYTES = {"plain": 28, "guard": 32, "clip": 32, "decoupled": 32, "ema": 40}          # per parameter


def options(argv=None):
    o = PARSER.parse_args(argv)
    for m in o.models:
        if m not in ("both", "hrnet"):
            PARSER.error(f"--models: both, hrnet (got {m!r})")
    return o


def shapes(models):
    """the parameter shapes of HRNet (+ ShiftNet for "both"), in the optimiser's order"""
    from DeepNetworks.HRNet import HRNet
    from DeepNetworks.ShiftNet import ShiftNet
    from oracle import weights
    mods = [HRNet(weights.HRNET_CONFIG)] + ([ShiftNet()] if models == "both" else [])
    return [tuple(p.shape) for m in mods for p in m.parameters()]


def bench(models, rounds, reps, warmup):
    from hrnet_hip import binding
    ops, dev = torch.ops.hrnet_hip, torch.device("cuda:0")
    shp = shapes(models)
    n = sum(int(torch.Size(s).numel()) for s in shp)
    n_pad = (n + 3) // 4 * 4
    nsets = max(1, -(-2 * LLC_BYTES // (20 * n_pad)))
    gen = torch.Generator(device=dev).manual_seed(n % 1000)
    b1, b2 = BETAS

    def flat_set():
        p = torch.randn(n_pad, device=dev, generator=gen)
        return dict(p=p, g=torch.randn(n_pad, device=dev, generator=gen) * 3e-3, m=torch.zeros_like(p), v=torch.zeros_like(p), e=p.clone(),
                    ctl=torch.zeros((1, binding.OPTIM_CTL_WORDS), dtype=torch.int64, device=dev))

    flats = {name: [flat_set() for _ in range(nsets)] for name in BYTES}
    count = {name: 0 for name in (*BYTES, "torch")}

    def plain():
        f = flats["plain"][count["plain"] % nsets]
        count["plain"] += 1
        ops.adam_step(f["p"], f["g"], f["m"], f["v"], LR, b1, b2, EPS, WD, count["plain"])

    def extended(name, max_norm, decoupled, ema):
        def run():
            f = flats[name][count[name] % nsets]
            count[name] += 1
            sums = ops.grad_sumsq(f["g"]).view(1, 2)
            ops.optim_prepare(sums, f["ctl"], 0, max_norm, LR, b1, b2)
            ops.adam_step_ex(f["p"], f["g"], f["m"], f["v"], f["e"] if ema else None, f["ctl"], 0, b1, b2, EPS, WD, decoupled, DECAY if ema else 0.0)
        return run

    torch_sets = []
    for _ in range(nsets):
        ps = [torch.nn.Parameter(torch.randn(s, device=dev, generator=gen)) for s in shp]
        for p in ps:
            p.grad = torch.randn(p.shape, device=dev, generator=gen) * 3e-3
        torch_sets.append((ps, torch.optim.AdamW(ps, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD), [p.detach().clone() for p in ps]))
    ema_update = torch.optim.swa_utils.get_ema_multi_avg_fn(DECAY)

    def composed():
        ps, opt, ema = torch_sets[count["torch"] % nsets]
        count["torch"] += 1
        torch.nn.utils.clip_grad_norm_(ps, MAX_NORM)
        opt.step()
        with torch.no_grad():
            ema_update(ema, ps, count["torch"])

    runs = {"plain": plain, "guard": extended("guard", 0.0, False, False), "clip": extended("clip", MAX_NORM, False, False),
            "decoupled": extended("decoupled", MAX_NORM, True, False), "ema": extended("ema", MAX_NORM, True, True), "torch": composed}
    times = _common.alternate(runs, rounds, reps, warmup * nsets)
    res = {"models": models, "parameters": n, "tensors": len(shp), "buffer_sets": nsets, "rounds": rounds, "reps": reps,
           "clip_coef": float(binding.optim_ctl_field(flats["clip"][0]["ctl"], 0, "coef"))}
    print(f"{models}: {n / 1e6:.2f} M parameters in {len(shp)} tensors, median of {rounds} rounds x {reps} steps over {nsets} buffer sets "
          f"(clip coefficient {res['clip_coef']:.3f})")
    base = _common.spread(times["plain"])[0]
    for name in runs:
        med, lo, hi = _common.spread(times[name])
        res[name] = {"median_us": med, "min_us": lo, "max_us": hi, "over_plain": med / base}
        line = f"    {name:10s} {med:9.1f} us   (min {lo:.1f}, max {hi:.1f})   {med / base:5.2f} x plain"
        if name in BYTES:
            floor = BYTES[name] * n_pad / HBM_ACHIEVABLE * 1e6
            res[name].update(floor_us=floor, predicted_over_plain=BYTES[name] / BYTES["plain"])
            line += f" (bytes predict {BYTES[name] / BYTES['plain']:.2f});  byte floor {floor:.1f} us = {100 * floor / med:.0f} % of it"
        print(line)
    res["torch_over_ema"] = res["torch"]["median_us"] / res["ema"]["median_us"]
    print(f"    torch composition / extended step with everything on: {res['torch_over_ema']:.2f} x")
    return res


def main():
    o = options()
    _common.require_gpu("optim_bench")
    _common.emit("optim_bench", [bench(m, o.rounds, o.reps, o.warmup) for m in o.models])


if __name__ == "__main__":
    main()
