"""GPU (-m gpu): what shift-and-add is for.  A synthetic scene (tests/shift_add_scene.py): a periodic HR image of 192 x 192 band-limited at
0.25 cycles per HR pixel (the LR Nyquist is 0.167: the views alias), nine x3 views of 64 x 64 - Fourier-shifted by known shifts of up to
1.5 px, 3 x 3 box-averaged, noise 0.005, two cloud discs per view masked with a margin - scored by the interior PSNR (12 HR pixels off
every side, where the periodic scene and the frame's border disagree).

On the CPU the fp64 restatement from the true shifts (sigma 0.25, prior 0.05, base = the bicubic of the clearest view) reaches 26.28 dB
where that bicubic reaches 25.23 dB: a margin of 1.05 dB for this scene (the issue's prototype scene had 1.5 dB).  The device result from
the true shifts equals the restatement within the project's bound and must keep at least half that margin; `register_and_add` must find
the shifts to the registration tests' own 0.02 px and beat the bicubic too.  Its gap to the true-shift result is printed, not asserted
(DESIGN.md section 7s records it)."""
import numpy as np
import pytest
import torch

import kernel_bounds as KB
import shift_add_ref as R
import shift_add_scene as SS
import upsample_ref as U
import util
from hrnet_hip import shiftadd, upsample

pytestmark = pytest.mark.gpu

SCALE, SIGMA, PRIOR, BORDER = 3, 0.25, 0.05, 12
RECOVERY_PX = 0.02           # the project's bound on every component of a recovered shift (tests/test_gpu_registration_scene.py)
SEARCH = dict(points_per_dim=5, levels=8, radius=2.0)      # a reach of 2 px for shifts of up to 1.5; the last level's step is 0.0005 px
_made = {}


def _scene():
    """the scene, the restatement's result from the true shifts and the two CPU PSNRs, made once"""
    if not _made:
        sc = SS.make(n_lr=64, scale=SCALE, views=9, band=0.25, limit=1.5, noise=0.005, clouds=2, margin=3.0, seed=1)
        bic = U.forward(sc["lrs"][0, 0], SCALE, -0.75).astype(np.float32)[None]
        out, D, T, den = R.forward(sc["lrs"], sc["masks"], None, sc["shifts"], SCALE, SIGMA, PRIOR, bic)
        _made.update(sc, bic=bic, out=out, T=T, keep=~R.excluded(den), psnr_ref=SS.psnr(out[0], sc["hr"], BORDER),
                     psnr_bic=SS.psnr(bic[0].astype(np.float64), sc["hr"], BORDER))
    return _made


def test_true_shifts_give_the_restatement_and_beat_the_bicubic_of_the_clearest_view():
    s = _scene()
    margin = s["psnr_ref"] - s["psnr_bic"]
    print(f"restatement {s['psnr_ref']:.2f} dB, bicubic of the clearest view {s['psnr_bic']:.2f} dB: margin {margin:.2f} dB")
    assert margin >= 0.9                                           # the scene is the one the docstring describes (1.05 dB)
    lrs, masks, shifts = util.dev(s["lrs"]), util.dev(s["masks"]), util.dev(s["shifts"])
    base = upsample.upsample(lrs[:, 0], SCALE)
    assert float((base.cpu().double() - torch.from_numpy(s["bic"]).double()).abs().max()) <= 1e-5
    sr, weight = shiftadd.shift_and_add(lrs, shifts, masks, None, SCALE, SIGMA, PRIOR, base=util.dev(s["bic"]), return_weight=True)
    got = sr.cpu().double()
    want, T = torch.from_numpy(s["out"]), torch.from_numpy(s["T"])
    got = torch.where(torch.from_numpy(s["keep"]), got, want)
    KB._assert_close("quality scene, true shifts", "f32", got, want, T, layout="b y x")
    psnr = SS.psnr(sr[0].cpu().double().numpy(), s["hr"], BORDER)
    print(f"device {psnr:.2f} dB: {psnr - s['psnr_bic']:.2f} dB over the bicubic")
    assert psnr - s["psnr_bic"] >= 0.5 * margin
    assert bool((weight > 0).all())                                # nine views: every HR pixel is reached


def test_register_and_add_finds_the_shifts_and_beats_the_bicubic():
    s = _scene()
    lrs, masks = util.dev(s["lrs"]), util.dev(s["masks"])
    sr, weight, shifts = shiftadd.register_and_add(lrs, masks, None, scale=SCALE, sigma=SIGMA, prior=PRIOR, base=util.dev(s["bic"]), **SEARCH)
    err = np.abs(shifts.cpu().numpy() - s["shifts"])
    print(f"worst component error of the recovered shifts {err.max():.4f} px")
    assert tuple(shifts.shape) == (1, 9, 2) and err.max() <= RECOVERY_PX and bool((shifts[:, 0] == 0).all())
    psnr = SS.psnr(sr[0].cpu().double().numpy(), s["hr"], BORDER)
    print(f"register_and_add {psnr:.2f} dB: {psnr - s['psnr_bic']:.2f} dB over the bicubic, {s['psnr_ref'] - psnr:+.2f} dB below the true-shift restatement")
    assert psnr > s["psnr_bic"]
    # the default base is the library's own bicubic baseline (the composite of the unregistered views): finite, and still above it
    auto = shiftadd.register_and_add(lrs, masks, None, scale=SCALE, **SEARCH)[0]
    print(f"with base=\"bicubic\": {SS.psnr(auto[0].cpu().double().numpy(), s['hr'], BORDER):.2f} dB")
    assert bool(torch.isfinite(auto).all())
