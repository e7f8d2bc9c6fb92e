"""CPU: what tests/test_gpu_cssim_pin.py relies on, shown without a GPU.

- The finding.  A float32 model of the kernel's algebra (cssim_ref.shift_cssim_f32: a model, not a reference and not the kernel) in the
  uncentred form the kernel shipped with misses the fp64 restatement by more than the project's cap of 1e-5 on bright, clear,
  low-contrast frames and stays inside the shipped tests' 2e-6 on their scenes, whose 15 % holes give every window a large variance;
  the centred form the kernel has now stays inside 2e-6 on all of them.
- The gaps.  On every case of the GPU test where k* is compared, the restatement's best offset leads the runner-up by >= 10 x the cap.
- The controls.  Every wrong variant of the restatement (cssim_ref.CONTROLS) moves a score of its case by >= 10 x the cap; the ratios
  are printed.
- The restatement is exactly invariant under (s, g, L) -> (2^p s, 2^p g, 2^p L) without the clip."""
import numpy as np
import pytest

import cssim_cases as C
import cssim_ref as R
from kernel_bounds import CSSIM_BOUND, CSSIM_TOL_PIN

CASE = {c[0]: c for c in C.PIN_CASES}


def test_the_cases_are_the_ones_named():
    assert R.MODEL_TH == C.TH and all(R.MODEL_WIN - R.TAPS[w] + 1 == C.TW[w] for w in C.TW)
    assert CSSIM_TOL_PIN <= CSSIM_BOUND == 1e-5 and C.PIN_GAP == 10 * CSSIM_BOUND
    fam = lambda f: [c for c in C.PIN_CASES if c[1] == f]
    assert len(fam("conditioning")) == 2 * 2 * 10 and {c[6] for c in fam("conditioning")} == {3}
    assert sorted((c[6], c[7]) for c in fam("instances")) == sorted((b, w) for b in (4, 5, 6, 7) for w in C.TW)
    for _, _, _, B, H, W, border, window in fam("instances"):          # one map pixel more than one tile along both axes
        T = R.TAPS[window]
        assert (H, W) == (17 + T - 1 + 2 * border, C.TW[window] + 1 + T - 1 + 2 * border)
    assert max(c[4] * c[5] for c in C.PIN_CASES) == 41 * 79 or max(c[5] for c in fam("instances")) == 79
    assert {(c[4], c[5], c[7]) for c in fam("seams")} == {(49, 125, "gaussian"), (45, 2 * 58 + 1 + 6 + 6, "uniform")}
    assert sorted({(c[4] - 6) * (c[5] - 6) for c in fam("runs")}) == [2047, 2048, 2050]
    assert set(C.PIN_SEEDS) <= set(CASE)


# ----------------------------------------------------------------------------- the finding
MODEL_SCENES = [(H, W, window, name) for H, W in ((24, 24), (49, 71)) for window in ("gaussian", "uniform")
                for name in ("holes", "bright-holes", "clear", "blob")]


@pytest.mark.parametrize("H,W,window,name", MODEL_SCENES)
def test_the_uncentred_model_breaks_the_cap_on_clear_frames_and_the_centred_one_does_not(H, W, window, name):
    if name == "holes":
        x = R.scene(17 * H + W, H, W)
    elif name == "bright-holes":                                # the shipped scene made bright and flat: the holes alone hide the cancellation
        s, h, m = R.scene(17 * H + W, H, W)
        x = ((0.9 + 0.05 * (s - 0.5)).astype(np.float32), (0.9 + 0.05 * (h - 0.5)).astype(np.float32), m)
    else:
        x = R.scene_clear(17 * H + W, H, W, 0.9, 0.05, name)
    want = R.shift_cssim(*x, 3, window)[0]
    unc = float(np.abs(R.shift_cssim_f32(*x, 3, window, form="uncentred") - want).max())
    cen = float(np.abs(R.shift_cssim_f32(*x, 3, window, form="centred") - want).max())
    print(f"cssim float32 model {H}x{W} {window} {name}: uncentred {unc:.2e}, centred {cen:.2e}")
    assert cen <= C.TOL
    if name in ("clear", "blob"):
        assert unc > CSSIM_BOUND
    else:
        assert unc <= C.TOL


# ----------------------------------------------------------------------------- the gaps
@pytest.mark.parametrize("case", C.PIN_CASES, ids=[c[0] for c in C.PIN_CASES])
def test_the_best_offset_leads_by_ten_bounds(case):
    scores, k, _, _ = C.pin_ref(case)
    for b in range(len(k)):
        assert k[b] >= 0 and R.gap(scores[b]) >= C.PIN_GAP, (case[0], b, R.gap(scores[b]), "replace the seed")


def test_the_other_compared_inputs_lead_by_ten_bounds():
    """the frames of the GPU test's data_range and +inf cases"""
    s, h, m = C.scene_batch(2, 24, 30)
    quarter = ((0.25 * np.clip(s, 0, 1)).astype(np.float32), (0.25 * h).astype(np.float32), m)
    inf = s.copy()
    inf[0, 12, 13] = np.inf
    for window in ("gaussian", "uniform"):
        for x, kw in ((quarter, dict(data_range=0.25)), ((inf, h, m), dict(clip=True))):
            scores, k, _, _ = C.ref(x, 3, window, **kw)
            assert all(R.gap(sc) >= C.PIN_GAP for sc in scores) and (k >= 0).all()


# ----------------------------------------------------------------------------- the controls
# (control, the case it is shown on).  bias_left_out is shown on a holes scene (sr = 0.9 hr + 0.03: a bias of about 0.02; scene_clear's
# gain is about its level, so its bias is near 0); pixel_left_out at the largest map, 33 x 109, where one SSIM value of about 0.7 is
# 0.7 / 3597 = 2e-4 of the mean.
CONTROL_CASES = [("tap_dropped", "cond-49x71-gaussian-L0.9-c0.05-clear"), ("tap_dropped", "inst-b5-uniform-clear"),
                 ("neighbouring_offset", "cond-49x71-uniform-L0.9-c0.05-blob"), ("neighbouring_offset", "inst-b6-gaussian-holes"),
                 ("neighbouring_offset", "cond-24x24-gaussian-L0.9-c0.005-clear"),
                 ("cov_norm_one", "cond-24x24-uniform-L0.9-c0.05-edge"), ("cov_norm_one", "inst-b7-uniform-clear"),
                 ("bias_left_out", "runs-2050-gaussian"), ("bias_left_out", "seam-45x129-uniform-holes"),
                 ("pixel_left_out", "seam-49x125-gaussian-clear"), ("pixel_left_out", "seam-49x125-gaussian-holes"),
                 ("pixel_left_out", "seam-45x129-uniform-clear"),
                 ("row_left_out", "seam-49x125-gaussian-clear"), ("row_left_out", "inst-b4-gaussian-holes")]


@pytest.mark.parametrize("control,cid", CONTROL_CASES)
def test_a_control_moves_a_score_by_ten_bounds(control, cid):
    case = CASE[cid]
    x = C.pin_input(case)
    want = C.pin_ref(case)[0]
    for b in range(case[3]):
        got = R.shift_cssim_control(control, x[0][b], x[1][b], x[2][b], case[6], case[7])
        fin = np.isfinite(want[b])
        ratio = float(np.abs(got[fin] - want[b][fin]).max() / CSSIM_BOUND)
        print(f"cssim control {control} on {cid}[{b}]: moves a score by {ratio:.1f} x the cap")
        assert ratio >= 10.0, (control, cid, b, ratio)


@pytest.mark.parametrize("value", [0.25, 3.0])
def test_the_map_as_a_weight_moves_a_score_by_ten_bounds(value):
    """the frames of the GPU test's map-semantics case: a kernel that weighted by the map's value would not pass them.  (A weight of -1
    is no control: it flips the sign of X and Y alike, and n_k, the bias and the SSIM are even in that; the GPU case keeps it for != 0.)"""
    s, h, m = C.scene_batch(2, 24, 30)
    m2 = np.where(m != 0, np.float32(value), np.float32(0.0)).astype(np.float32)
    for b in range(2):
        want = R.shift_cssim(s[b], h[b], m2[b], 3)[0]
        assert np.array_equal(want, R.shift_cssim(s[b], h[b], m[b], 3)[0])
        got = R.shift_cssim_control("map_as_weight", s[b], h[b], m2[b], 3)
        ratio = float(np.abs(got - want).max() / CSSIM_BOUND)
        print(f"cssim control map_as_weight at {value}[{b}]: moves a score by {ratio:.1f} x the cap")
        assert ratio >= 10.0
    assert np.array_equal(R.shift_cssim_control("map_as_weight", s[0], h[0], m[0], 3), R.shift_cssim(s[0], h[0], m[0], 3)[0])


def test_every_control_is_shown():
    assert {c for c, _ in CONTROL_CASES} | {"map_as_weight"} == set(R.CONTROLS)


# ----------------------------------------------------------------------------- scale invariance of the definition
@pytest.mark.parametrize("p", [-2, 3])
@pytest.mark.parametrize("window", ["gaussian", "uniform"])
def test_the_restatement_is_exactly_scale_invariant(p, window):
    for s, h, m in (R.scene(3, 24, 30), R.scene_clear(3, 24, 30, 0.9, 0.05, "blob")):
        f = np.float32(2.0 ** p)
        a = R.shift_cssim(s * f, h * f, m, 3, window, clip=False, data_range=2.0 ** p)
        b = R.shift_cssim(s, h, m, 3, window, clip=False, data_range=1.0)
        assert np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2] * 2.0 ** p) and np.array_equal(a[3], b[3])


def test_ties_of_the_gpu_cases_are_exact_in_the_restatement():
    """hr constant: the offsets of one row of offsets see identical data"""
    rng = np.random.default_rng(61)
    s, h = rng.random((30, 34)).astype(np.float32), np.full((30, 34), 0.5, np.float32)
    for rows, want in (("none", 0), ("first", 0), ("all but the last", 7)):
        m = np.ones((30, 34), np.float32)
        if rows == "first":
            m[:6] = 0.0
        elif rows != "none":
            m[:-6] = 0.0
        scores, k, _, n = R.shift_cssim(s, h, m, 3)
        assert k == want and all(np.all(scores[7 * u:7 * u + 7] == scores[7 * u]) for u in range(7))
        groups = np.unique(scores[np.isfinite(scores)])
        assert len(groups) == 1 if rows == "none" else groups[-1] - groups[-2] >= C.PIN_GAP
