#!/usr/bin/env python3
"""Time one optimisation step of src/train.py:164-191 on the HIP modules:

    srs = fusion_model(lrs, alphas); shifts = register_batch(regis_model, crops, reference); srs_shifted = apply_shifts(...);
    loss = -cPSNR(srs_shifted, hrs, mask) + lambda mean(shifts)^2; loss.backward(); optimizer.step()

at the reference's training shape (config/config.json: batch 32, up to 32 views, 64 x 64 patches) with synthetic data.
usage: python tools/train_step_bench.py [B V S steps] [--torch-adam] [--precision P[,P...]] [--shiftnet-precision P[,P...]] [--repeats R]
                                        [--freeze F[,F...]] [--scale K] [--loss L[,L...]]

--precision sets HRNet.train_precision (fp32, bf16x3 or bf16; default: not set, i.e. the module's default rules), --shiftnet-precision
ShiftNet.train_precision (fp32 or bf16; default: not set).  With several values, one pair of models per combination is built and their
timing rounds alternate, R rounds each (--repeats, default 1).  --freeze times the step with part of the models frozen
(requires_grad_(False) before the optimiser is built, as in fine-tuning): none (default), encoder (HRNet's encoder), encoder+fuse (HRNet's
encoder and fusion block: only the decoder trains) or shiftnet (a fixed ShiftNet that only passes d x back into HRNet); several values
alternate in one process like the precisions.  --scale K (2, 3 or 4; default 3) times the x2 / x4 step: a stride-K decoder (freshly
initialised for K != 3, on the seeded x3 encoder and fusion block) and K S x K S targets; K * S must reach ShiftNet's 128-pixel window.
--loss picks the tail of the step: shiftnet (default) is the reference's ShiftNet -> Lanczos -> cPSNR above; shift is the searched loss,
loss = -shift_loss(srs, hrs, hr_maps) (hrnet_hip.losses): no ShiftNet is built, the optimiser holds HRNet's parameters
only, and the 128-pixel window does not apply; cssim is the second score as a loss, loss = mean(cssim_loss(srs, hrs, hr_maps)) (DESIGN.md
section 7l), HRNet alone as for shift; l1 is the searched L1, loss = mean(cl1_loss(srs, hrs, hr_maps)), likewise;
subpixel is the cPSNR registered at a sub-pixel shift, loss = -subpixel_loss(srs, hrs, hr_maps), likewise;
consistency is the loss without an HR target, loss = mean(consistency_loss(srs, lrs, shifts, alphas=alphas)) (hrnet_hip.observation,
DESIGN.md section 7t), HRNet alone again: it is timed twice, with shifts = mncc_search_scene(lrs) found under no_grad inside the step
("consistency") and with the shifts given ("consistency, shifts given").  Several values alternate in one process like the precisions.
"""
import copy
import time

import _common
import numpy as np
import torch

from oracle import synth, weights            # seeded weights / synthetic inputs only (no oracle arithmetic on the path)
from DeepNetworks.HRNet import HRNet
from DeepNetworks.ShiftNet import ShiftNet
from hrnet_hip import registration
from hrnet_hip.losses import cl1_loss, cssim_loss, shift_loss, subpixel_loss
from hrnet_hip.observation import consistency_loss
from hrnet_hip.optim import FusedAdam


def register_batch(shiftNet, lrs, reference):                 # train.py:26-44
    return torch.stack([shiftNet(torch.cat([reference, lrs[:, i:i + 1]], 1)) for i in range(lrs.size(1))], 1)


def apply_shifts(shiftNet, images, thetas, device):           # train.py:47-63
    b, n, h, w = images.shape
    return shiftNet.transform(thetas.view(-1, 2), images.view(-1, 1, h, w), device=device).view(-1, n, h, w)


def get_loss_cpsnr(srs, hrs, hr_maps):                        # train.py:66-87
    nclear = torch.sum(hr_maps, dim=(1, 2))
    bright = torch.sum(hr_maps * (hrs - srs), dim=(1, 2)).clone().detach() / nclear
    return -10 * torch.log10(torch.sum(hr_maps * (srs + bright.view(-1, 1, 1) - hrs) ** 2, dim=(1, 2)) / nclear)


FREEZE = {"none": lambda k: False, "encoder": lambda k: k.startswith("fusion.encode."),
          "encoder+fuse": lambda k: k.startswith(("fusion.encode.", "fusion.fuse.")), "shiftnet": lambda k: k.startswith("regis.")}


def _label(key):
    p, sp, fr, ls = key
    return (f"train_precision={p}" + (f" shiftnet_train_precision={sp}" if sp is not None else "") + (f" freeze={fr}" if fr != "none" else "")
            + (f" loss={CONSISTENCY.get(ls, ls)}" if ls != "shiftnet" else ""))


SEARCHED = {"shift": lambda srs, hrs, maps: -shift_loss(srs, hrs, maps), "cssim": cssim_loss, "l1": cl1_loss,
            "subpixel": lambda srs, hrs, maps: -subpixel_loss(srs, hrs, maps)}                                       # --loss -> the loss per sample

# --loss consistency is two runs: the tail's key -> its label
CONSISTENCY = {"consistency": "consistency", "consistency-given": "consistency, shifts given"}

PARSER = _common.parser(__doc__, group=("B V S steps", (32, 32, 64, 5)), torch_adam=False, precision=[None], shiftnet_precision=[None], repeats=1,
                        freeze=["none"], scale=3, loss=["shiftnet"])      # scale: decoder stride and HR / LR ratio of the targets


def options(argv=None):
    o = PARSER.parse_args(argv)
    for flag, got, allowed in (("--freeze", o.freeze, tuple(FREEZE)), ("--precision", o.precision, (None, "fp32", "bf16x3", "bf16")),
                               ("--shiftnet-precision", o.shiftnet_precision, (None, "fp32", "bf16")), ("--loss", o.loss, ("shiftnet", "shift", "cssim", "l1", "subpixel", "consistency"))):
        for v in got:
            if v not in allowed:
                PARSER.error(f"{flag}: {', '.join(a for a in allowed if a)} (got {v!r})")
    if o.scale not in (2, 3, 4) or ("shiftnet" in o.loss and o.scale * o.S < 128):
        PARSER.error(f"--scale: 2, 3 or 4, and with --loss shiftnet scale * S >= 128, ShiftNet's window (got {o.scale}, S = {o.S})")
    return o


def main():
    o = options()
    B, V, S, steps, scale, repeats = o.B, o.V, o.S, o.steps, o.scale, o.repeats
    precs, sprecs, freezes, tails = o.precision, o.shiftnet_precision, o.freeze, o.loss
    adam = torch.optim.Adam if o.torch_adam else FusedAdam
    _common.require_gpu("train_step_bench")
    dev = torch.device("cuda:0")
    lrs, alphas = synth.fast_batch(3, B, V, S)
    rng = np.random.Generator(np.random.PCG64(1))
    hrs = torch.from_numpy((rng.random((B, scale * S, scale * S), dtype=np.float32) * 0.25)).to(dev)
    maps = torch.ones((B, scale * S, scale * S), device=dev)
    maps[:, :3] = 0; maps[:, -3:] = 0; maps[:, :, :3] = 0; maps[:, :, -3:] = 0
    x, a = torch.from_numpy(lrs).to(dev), torch.from_numpy(alphas).to(dev)
    off = (scale * S - 128) // 2
    searched = dict(SEARCHED)
    if "consistency" in tails:                               # the views are the data: no hrs, no maps
        with torch.no_grad():
            given = registration.mncc_search_scene(x)

        def searching(srs, hrs, maps):
            with torch.no_grad():
                shifts = registration.mncc_search_scene(x)
            return consistency_loss(srs, x, shifts, alphas=a, scale=scale)
        searched.update({"consistency": searching, "consistency-given": lambda srs, hrs, maps: consistency_loss(srs, x, given, alphas=a, scale=scale)})
        tails = [t for tail in tails for t in (tuple(CONSISTENCY) if tail == "consistency" else (tail,))]

    def setup(prec, sprec, freeze, tail):
        cfg = copy.deepcopy(weights.HRNET_CONFIG)
        cfg["decoder"]["deconv"]["kernel_size"] = cfg["decoder"]["deconv"]["stride"] = scale
        fusion = HRNet(cfg)
        state = weights.to_torch_state(weights.hrnet_state(1234))
        if scale != 3:                                       # the x3 -> x2 / x4 recipe: a freshly initialised decoder on the x3 body
            state = {k: v for k, v in state.items() if not k.startswith("decode.")}
        fusion.load_state_dict(state, strict=scale == 3)
        fusion.train_precision = prec
        if tail in searched:                                 # a searched loss has no parameters: HRNet alone is built and optimised
            fusion = fusion.to(dev).train()
            for k, p in fusion.named_parameters():
                p.requires_grad_(not FREEZE[freeze]("fusion." + k))
            params = list(fusion.parameters())
            return fusion, searched[tail], adam(params, lr=1e-4)
        regis = ShiftNet()
        if sprec is not None:
            regis.train_precision = sprec
        regis.load_state_dict(weights.to_torch_state(weights.shiftnet_state(4321)))
        fusion, regis = fusion.to(dev).train(), regis.to(dev).train()
        for prefix, mod in (("fusion.", fusion), ("regis.", regis)):
            for k, p in mod.named_parameters():
                p.requires_grad_(not FREEZE[freeze](prefix + k))
        params = list(fusion.parameters()) + list(regis.parameters())
        return fusion, regis, adam(params, lr=1e-4)

    def step(fusion, regis, opt):
        opt.zero_grad()
        srs = fusion(x, a)
        if not isinstance(regis, torch.nn.Module):           # a searched loss: `regis` is the function of (srs, hrs, maps)
            loss = torch.mean(regis(srs, hrs, maps))
            loss.backward()
            opt.step()
            return loss
        shifts = register_batch(regis, srs[:, :, off:off + 128, off:off + 128], hrs[:, off:off + 128, off:off + 128].reshape(-1, 1, 128, 128))
        shifted = apply_shifts(regis, srs, shifts, dev)[:, 0]
        loss = -get_loss_cpsnr(shifted, hrs, maps)
        loss = torch.mean(loss) + 1e-6 * torch.mean(shifts) ** 2
        loss.backward()
        opt.step()
        return loss

    runs = {(p, sp, f, t): setup(p, sp, f, t) for p in precs for t in tails for sp in (sprecs if t == "shiftnet" else [None]) for f in freezes
            if not (t in searched and f == "shiftnet")}
    for r in runs.values():
        for _ in range(2):
            step(*r)
    times = {k: [] for k in runs}
    for _ in range(repeats):
        for p, r in runs.items():
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()             # the round's own peak (every run's models and optimiser state stay resident)
            t0 = time.time()
            for _ in range(steps):
                loss = step(*r)
            torch.cuda.synchronize()
            dt = (time.time() - t0) / steps
            times[p].append(dt)
            print(f"train step B={B} V={V} S={S}{f' scale={scale}' if scale != 3 else ''} {_label(p)}: {dt * 1e3:.1f} ms/step ({B / dt:.0f} samples/s, {1 / dt:.2f} steps/s), "
                  f"loss {float(loss.detach()):.3f}, peak memory {torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB, "
                  f"optimiser {type(r[2]).__name__} over {sum(q.numel() for g in r[2].param_groups for q in g['params']) / 1e6:.2f} M parameters")
    if repeats > 1 or len(runs) > 1:
        for p, t in times.items():
            med, lo, hi = _common.spread(dt * 1e3 for dt in t)
            print(f"summary {_label(p)}: median {med:.1f} ms/step, min {lo:.1f}, max {hi:.1f} over {len(t)} rounds")


if __name__ == "__main__":
    main()
