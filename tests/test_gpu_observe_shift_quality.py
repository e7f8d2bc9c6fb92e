"""GPU (-m gpu): what the joint refinement of the shifts is for, on the scene of tests/test_gpu_observe_quality.py (tests/shift_add_scene.py:
nine aliased x3 views of 64 x 64, noise 0.005, two masked cloud discs per view; the interior PSNR 12 HR pixels off every side).  Views
1..8 start at the true shifts plus uniform +-0.3 px from PCG64(7); every run starts from the shift-and-add of the shifts it is given
(sigma 0.25, prior 0.05, base = the bicubic of the clearest view) and takes 30 plain iterations of step 1; the joint run updates the shifts
beside every data step from iteration 1 on (refine_every = 1, refine_from = 1, damping 1e-3, max_step 0.5, view 0 fixed).

The yardstick is the fp64 restatement of the same schedule (tests/observe_shift_ref.py), on the CPU:
    true shifts 33.30 dB;  the bad shifts held fixed 23.78 dB (0.297 px off);  joint 32.30 dB, the largest shift error 0.028 px
so the restatement gains 8.52 dB over the bad shifts and stays 1.00 dB below the true ones.  The device must equal the restatement's PSNR
to 0.01 dB and its largest shift error to 1e-3 px, beat the fixed-bad-shifts result by at least half the restatement's gain, stay below
the true-shift result by at most twice the restatement's gap plus 0.05 dB, and end with a shift error under twice the restatement's.
Control: with every view fixed the shifts come back bit-identical and the frame is `reconstruct`'s.  `refine_shifts` alone, two steps
against the true-shift frame, must end within 1e-3 px of the restatement's shift error."""
import numpy as np
import pytest
import torch

import observe_ref as O
import observe_shift_ref as R
import shift_add_ref as SA
import shift_add_scene as SS
import upsample_ref as U
import util
from hrnet_hip import observation

pytestmark = pytest.mark.gpu

SCALE, SIGMA, PRIOR, BORDER, ITERS = 3, 0.25, 0.05, 12, 30
JOINT = dict(refine_every=1, refine_from=1, damping=1e-3, max_step=0.5, fixed=0)
PLAIN = dict(step=1.0, brightness=True, robust=None, lam=0.0)
_made = {}


def _scene():
    """the scene, the starts and the restatement's three results, made once"""
    if not _made:
        sc = SS.make(n_lr=64, scale=SCALE, views=9, band=0.25, limit=1.5, noise=0.005, clouds=2, margin=3.0, seed=1)
        bad = sc["shifts"].copy()
        bad[:, 1:] += np.random.Generator(np.random.PCG64(7)).uniform(-0.3, 0.3, (1, 8, 2)).astype(np.float32)
        bic = U.forward(sc["lrs"][0, 0], SCALE, -0.75).astype(np.float32)[None]
        start = lambda sh: SA.forward(sc["lrs"], sc["masks"], None, sh, SCALE, SIGMA, PRIOR, bic)[0].astype(np.float32)
        s_true, s_bad = start(sc["shifts"]), start(bad)
        ps = lambda x: SS.psnr(x[0], sc["hr"], BORDER)
        x_true, _ = O.back_project(s_true, sc["lrs"], sc["masks"], None, sc["shifts"], SCALE, ITERS)
        x_bad, _ = O.back_project(s_bad, sc["lrs"], sc["masks"], None, bad, SCALE, ITERS)
        x_joint, sh_joint = R.reconstruct_joint(s_bad, sc["lrs"], sc["masks"], None, bad, SCALE, iters=ITERS, robust=False, lam=0.0, **JOINT)
        back = R.refine_shifts(x_true, sc["lrs"], sc["masks"], None, bad, SCALE, iters=2)
        _made.update(sc, e_refine=float(np.abs(back - sc["shifts"]).max()), bad=bad, s_true=s_true, s_bad=s_bad, p_true=ps(x_true), p_bad=ps(x_bad), p_joint=ps(x_joint),
                     e_joint=float(np.abs(sh_joint - sc["shifts"]).max()))
    return _made


def _psnr(sr, s):
    return SS.psnr(sr[0].cpu().double().numpy(), s["hr"], BORDER)


def test_joint_refinement_repairs_rough_shifts_as_the_restatement_does():
    s = _scene()
    gain, gap = s["p_joint"] - s["p_bad"], s["p_true"] - s["p_joint"]
    print(f"restatement: true shifts {s['p_true']:.2f} dB, bad shifts held {s['p_bad']:.2f} dB, joint {s['p_joint']:.2f} dB (gain {gain:.2f} dB, "
          f"gap {gap:.2f} dB); shift error {np.abs(s['bad'] - s['shifts']).max():.3f} -> {s['e_joint']:.4f} px")
    assert gain >= 6.0 and gap <= 2.0 and s["e_joint"] <= 0.05              # the scene and the schedule are the docstring's
    lrs, masks = util.dev(s["lrs"]), util.dev(s["masks"])
    true, bad = util.dev(s["shifts"]), util.dev(s["bad"])
    p_true = _psnr(observation.reconstruct(util.dev(s["s_true"]), lrs, true, masks, None, SCALE, iters=ITERS, **PLAIN), s)
    held = observation.reconstruct(util.dev(s["s_bad"]), lrs, bad, masks, None, SCALE, iters=ITERS, **PLAIN)
    sr, shifts = observation.reconstruct_joint(util.dev(s["s_bad"]), lrs, bad, masks, None, SCALE, iters=ITERS, **JOINT, **PLAIN)
    p_bad, p_joint = _psnr(held, s), _psnr(sr, s)
    err = float(np.abs(shifts.cpu().numpy() - s["shifts"]).max())
    print(f"device: true shifts {p_true:.2f} dB, bad shifts held {p_bad:.2f} dB, joint {p_joint:.3f} dB ({p_joint - s['p_joint']:+.4f} dB of the "
          f"restatement); shift error {err:.4f} px ({err - s['e_joint']:+.5f} px)")
    assert abs(p_joint - s["p_joint"]) <= 0.01 and abs(err - s["e_joint"]) <= 1e-3
    assert p_joint - p_bad >= 0.5 * gain and p_true - p_joint <= 2.0 * gap + 0.05 and err < 2.0 * s["e_joint"]
    assert torch.equal(shifts[:, 0], bad[:, 0])                             # the gauge
    # the control: with every view fixed nothing moves and the frame is reconstruct's
    every = torch.ones((1, 9), dtype=torch.bool, device="cuda")
    sr_c, shifts_c = observation.reconstruct_joint(util.dev(s["s_bad"]), lrs, bad, masks, None, SCALE, iters=ITERS, **{**JOINT, "fixed": every}, **PLAIN)
    assert torch.equal(shifts_c.view(torch.int32), bad.view(torch.int32)) and torch.equal(sr_c.view(torch.int32), held.view(torch.int32))
    # refine_shifts alone, against the true-shift frame: two steps bring the bad shifts back
    frame = observation.reconstruct(util.dev(s["s_true"]), lrs, true, masks, None, SCALE, iters=ITERS, **PLAIN)
    back = observation.refine_shifts(frame, lrs, bad, masks, None, SCALE, iters=2)
    e2 = float(np.abs(back.cpu().numpy() - s["shifts"]).max())
    print(f"refine_shifts, two steps against the true-shift frame: {np.abs(s['bad'] - s['shifts']).max():.3f} -> {e2:.4f} px "
          f"(restatement {s['e_refine']:.4f} px)")
    assert abs(e2 - s["e_refine"]) <= 1e-3 and s["e_refine"] < 0.05
