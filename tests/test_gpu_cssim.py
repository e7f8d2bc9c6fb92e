"""GPU: the shift-searched SSIM (hrnet_hip.losses.shift_cssim over hrn_shift_cssim) against its fp64 restatement in
the direct form (tests/cssim_ref.py), at every offset.

Scenes (cssim_ref.scene): a smoothed random field as HR; SR the same field displaced by (+1, -2), x 0.9 + 0.03 plus noise of sigma 0.02;
a map with 15 % holes and a rectangular blob.  The restatement's own gap between the best and the second-best offset is asserted to be
>= 1e-3 before k* is compared.

Shapes: the kernel's tile is TH x TW = 16 x (64 - T + 1) map pixels, T = 11 (gaussian) or 7 (uniform) taps, the map is (H - 2 border -
T + 1) x (W - 2 border - T + 1).  (2,24,24): an 8 x 8 map, far smaller than a tile.  (1,17,40): a map of one row, both windows.
(3,49,71) gaussian and (1,45,71) uniform at border 3: maps of 33 x 55 and 33 x 59, one pixel more than 2 x 1 tiles along each axis - the
remainder tile and the halo across the seams.  Border 0 (one offset), 1, and 8 on (1,43,81): a 17 x 55 map, 2 x 2 tiles, 289 offsets.

Tolerance on a score: the largest |GPU - fp64 restatement| measured on an MI355X over all the cases below (every offset, both windows,
clip and bias on and off, the edge samples) is MEASURED = 2.9e-7, at (1,17,40) gaussian, whose map is a single row of 24 pixels; the
larger maps sit at 4e-8 .. 2e-7.  The bound TOL is four times that, rounded up to one digit: 2e-6, the margin being for seeds and
shapes not listed; the issue caps it at 1e-5.  A dropped tap or a neighbouring offset moves a score by >= 4.6e-3 on these scenes.
(These figures are the kernel's as it shipped; since it centres its fields per tile - tests/test_gpu_cssim_pin.py, whose clear scenes
these maps' holes hid - the same cases measure at most 4.1e-8, at the same one-row map.  The bound stays.)"""
import numpy as np
import pytest
import torch

import cssim_ref as R
import util
from cssim_cases import SHIFT, TH, TOL, TW
from cssim_cases import compare as _compare, gpu as _gpu, ref as _ref, scene_batch as _scene

pytestmark = pytest.mark.gpu

MEASURED = 2.9e-7                                     # see the module docstring

# (B, H, W, border, window)
CASES = [(2, 24, 24, 3, "gaussian"), (1, 17, 40, 3, "gaussian"), (1, 17, 40, 3, "uniform"), (3, 49, 71, 3, "gaussian"),
         (1, 45, 71, 3, "uniform"), (2, 24, 30, 0, "gaussian"), (2, 30, 24, 1, "uniform"), (1, 43, 81, 8, "gaussian")]


def test_seam_shapes_follow_the_kernels_tile():
    """the tile constants stated above are the source's, and the two seam cases are one map pixel more than 2 x 1 tiles"""
    import os
    import re
    src = open(os.path.join(os.path.dirname(util.GOLDEN), "..", "highres-net_amd", "hrnet_hip", "csrc", "cssim.hip")).read()
    const = lambda name: int(re.search(rf"constexpr int {name} = (\d+);", src).group(1))
    assert const("CS_TH") == TH and all(const("CS_WIN") - R.TAPS[w] + 1 == TW[w] for w in TW)
    for window in TW:
        T = R.TAPS[window]
        assert (3 if window == "gaussian" else 1, 2 * TH + 1 + T - 1 + 6, TW[window] + 1 + T - 1 + 6, 3, window) in CASES
    assert (1, TH + 1 + 10 + 16, TW["gaussian"] + 1 + 10 + 16, 8, "gaussian") in CASES            # border 8: 2 x 2 tiles


@pytest.mark.parametrize("B,H,W,border,window", CASES)
def test_every_offset_matches_the_restatement(B, H, W, border, window):
    assert MEASURED <= TOL <= 1e-5
    x = _scene(B, H, W)
    _compare(x, border, window, f"{(B, H, W)} border {border} {window}", key=(B, H, W, 0))
    if border >= 2:        # the planted displacement is found: k* = 29 at border 3
        nb = 2 * border + 1
        assert list(_ref(x, border, window, key=(B, H, W, 0))[1]) == [(border + SHIFT[0]) * nb + border + SHIFT[1]] * B


@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("correct_bias", [True, False])
def test_clip_and_bias_switches(clip, correct_bias):
    """SR values outside [0, 1] present: clip changes the scores, and both ways match; the same for the bias."""
    s, h, m = _scene(2, 24, 40)
    s = s.copy()
    s[:, 5:9, 7:20] += 0.9
    s[:, 14:17, 20:30] -= 0.8
    assert (s > 1).any() and (s < 0).any()
    x = (s, h, m)
    for window in ("gaussian", "uniform"):
        _compare(x, 3, window, f"clip {clip} bias {correct_bias} {window}", key=("clip", 24, 40), clip=clip, correct_bias=correct_bias)
    a = _ref(x, 3, "gaussian", key=("clip", 24, 40), clip=clip, correct_bias=correct_bias)[0]
    b = _ref(x, 3, "gaussian", key=("clip", 24, 40), clip=not clip, correct_bias=correct_bias)[0]
    assert np.abs(a - b).max() > 1e-3


def test_data_range_enters_the_constants():
    x = _scene(1, 24, 30)
    _compare(x, 2, "uniform", "data_range 2.5", key=(1, 24, 30, 0), data_range=2.5)
    assert np.abs(_ref(x, 2, "uniform", key=(1, 24, 30, 0), data_range=2.5)[0] - _ref(x, 2, "uniform", key=(1, 24, 30, 0))[0]).max() > 1e-3


def _edge_batch():
    """sample 0: no clear pixel; 1: clear pixels in the top-left corner only; 2: a NaN inside the SR crop; 3: an ordinary scene"""
    s, h, m = (a.copy() for a in _scene(4, 30, 34))
    m[0] = 0.0
    m[1] = 0.0
    m[1, :3, :3] = 1.0
    s[2, 12, 13] = np.nan
    return s, h, m


def test_edge_samples():
    from hrnet_hip import losses
    x = _edge_batch()
    scores, k, _, n = _ref(x, 3, "gaussian", key="edge")
    assert k[0] == -1 and k[2] == -1 and k[1] >= 0 and k[3] == 29
    assert (n[1] == 0).any() and (n[1] > 0).any() and np.isnan(scores[2]).all()
    out, stats, got = _gpu(x, 3, "gaussian")
    assert np.isneginf(got[0]).all() and np.array_equal(np.isneginf(got[1]), n[1] == 0) and np.isnan(got[2]).all()
    assert np.isnan(out[0]) and np.isnan(out[2]) and stats[0, 3] == -1 and stats[2, 3] == -1
    fin = np.isfinite(scores)
    print(f"cssim edge samples: max |gpu - fp64| over {fin.sum()} scores = {np.abs(got[fin] - scores[fin]).max():.3e}")
    assert np.abs(got[fin] - scores[fin]).max() <= TOL
    # sample 1: the clear corner is in the crop only at offsets u, v <= 2; every one of them scores alike to within the bias, so
    # only the selected score is compared
    assert stats[1, 3] == k[1] or abs(scores[1, int(stats[1, 3])] - scores[1, k[1]]) <= TOL
    assert stats[3, 3] == 29
    val, shift, sc = losses.shift_cssim(*(util.dev(a) for a in x), return_shift=True, return_scores=True)
    assert np.array_equal(sc.cpu().numpy(), got, equal_nan=True) and np.array_equal(val.cpu().numpy(), out, equal_nan=True)
    assert shift.dtype == torch.int64 and shift[0].tolist() == [-4, 3] and shift[2].tolist() == [-4, 3]      # k = -1, as shift_loss
    assert shift[3].tolist() == list(SHIFT)


def test_two_runs_are_bit_identical_and_a_sample_does_not_see_its_batch():
    x = _scene(3, 49, 71)
    a, b = _gpu(x, 3, "gaussian"), _gpu(x, 3, "gaussian")
    for p, q in zip(a, b):
        assert np.array_equal(p, q, equal_nan=True)
    for i in range(3):
        alone = _gpu(tuple(t[i:i + 1] for t in x), 3, "gaussian")
        for p, q in zip(alone, a):
            assert np.array_equal(p[0], q[i], equal_nan=True), i


def test_wrapper_takes_a_channel_axis_and_strided_input():
    from hrnet_hip import losses
    s, h, m = (util.dev(a) for a in _scene(2, 24, 24))
    want = losses.shift_cssim(s, h, m)
    assert want.shape == (2,) and want.dtype == torch.float32
    assert torch.equal(losses.shift_cssim(s[:, None], h, m), want)
    st = s.transpose(1, 2).contiguous().transpose(1, 2)
    assert not st.is_contiguous() and torch.equal(losses.shift_cssim(st, h, m), want)
    s.requires_grad_(True)
    assert not losses.shift_cssim(s, h, m).requires_grad           # a score: no gradient


def test_opcheck():
    s, h, m = (util.dev(a) for a in _scene(2, 24, 24))
    torch.library.opcheck(torch.ops.hrnet_hip.shift_cssim.default, (s, h, m, 3, "gaussian", True, True, 1.0),
                          test_utils=("test_schema", "test_faketensor"))


def test_evaluate_with_cssim():
    from hrnet_hip import losses, validate
    model = util.hip_hrnet("fp32")
    rng = np.random.Generator(np.random.PCG64(77))
    sets = []
    for i in range(2):
        lrs, alphas = util.dev(rng.random((2, 4, 16, 16), dtype=np.float32)), util.dev(np.ones((2, 4), np.float32))
        hrs, maps = util.dev(rng.random((2, 48, 48), dtype=np.float32)), util.dev((rng.random((2, 48, 48)) > 0.1).astype(np.float32))
        sets.append((lrs, alphas, hrs, maps, [f"imgset{2 * i + j:04d}" for j in range(2)]))
    plain = validate.evaluate(model, sets)
    ev = validate.evaluate(model, sets, cssim=True)
    assert type(plain).__name__ == "Evaluation" and plain._fields == ("names", "cpsnr", "score")
    assert ev._fields == ("names", "cpsnr", "score", "cssim") and ev.names == plain.names
    assert np.array_equal(ev.cpsnr, plain.cpsnr) and ev.score == plain.score
    with torch.no_grad():
        want = torch.cat([losses.shift_cssim(model(l, a), h, m) for l, a, h, m, _ in sets])
    assert ev.cssim.dtype == np.float64 and np.array_equal(ev.cssim, want.double().cpu().numpy())
    assert np.isfinite(ev.cssim).all() and (np.abs(ev.cssim) <= 1).all()
    got = validate.sharded_val_score(model, sets, metric="cSSIM")
    assert abs(got - ev.cssim.mean()) <= 1e-15
