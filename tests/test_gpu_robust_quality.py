"""GPU (-m gpu): the quality table of the robust, regularised reconstruction on the device: the three scenes of
tests/robust_scenes.py - noise 0.02 with every cloud masked, noise 0.005 and noise 0.02 with the clouds of two views NOT in their masks -
from the device's own shift-and-add start (sigma 0.25, no prior, no base), plain back-projection, Welsch weights, the bilateral-TV prior
and both, at 10 and 30 iterations.  Each figure must be within 0.02 dB of the restatement's (tests/robust_ref.py), and the three
orderings the table is built for must hold on the device as they do on the CPU (tests/test_robust_host.py)."""
import pytest
import torch

import robust_scenes as Q
import util
from hrnet_hip import observation, shiftadd

pytestmark = pytest.mark.gpu

_got = {}


def _device(sc, method, iters):
    """the device's PSNR of one cell, computed once"""
    key = (sc, method, iters)
    if key not in _got:
        s = Q.scene(*sc)
        lrs, masks, shifts = util.dev(s["lrs"]), util.dev(s["masks"]), util.dev(s["shifts"])
        start = shiftadd.shift_and_add(lrs, shifts, masks, None, Q.SCALE, Q.SIGMA, 0.0, base=None)
        kw = Q.METHODS[method]
        sr = observation.reconstruct(start, lrs, shifts, masks, None, Q.SCALE, iters=iters, step=Q.STEP, robust="welsch" if kw["robust"] else None,
                                     delta=Q.DELTA, lam=kw["lam"], P=Q.P, alpha=Q.ALPHA, eps=Q.EPS)
        assert bool(torch.isfinite(sr).all())
        _got[key] = (Q.psnr(start.cpu().double().numpy(), s), Q.psnr(sr.cpu().double().numpy(), s))
    return _got[key]


@pytest.mark.parametrize("sc", Q.SCENES, ids=lambda sc: f"noise{sc[0]}-unmasked{sc[1]}")
def test_every_figure_is_the_restatements(sc):
    s = Q.scene(*sc)
    worst, cells = 0.0, []
    for method in Q.METHODS:
        pair = []
        for iters in (10, 30):
            start, got = _device(sc, method, iters)
            want = Q.restated(*sc, method, iters)[1]
            worst = max(worst, abs(got - want), abs(start - Q.psnr(s["start"], s)))
            pair.append(f"{got:.2f}")
        cells.append(f"{method} {' / '.join(pair)}")
    print(f"noise {sc[0]}, {sc[1]} unmasked: start {_device(sc, 'plain', 10)[0]:.2f} dB | " + " | ".join(cells) +
          f" | largest difference to the restatement {worst:.4f} dB")
    assert worst <= 0.02


def test_the_three_orderings_hold_on_the_device():
    for sc, method, iters, margin in Q.ORDERINGS:
        got, plain = _device(sc, method, iters)[1], _device(sc, "plain", iters)[1]
        print(f"{sc} {method} at {iters}: {got:.2f} dB against plain {plain:.2f} dB ({got - plain:+.2f} dB)")
        assert got >= plain + margin
