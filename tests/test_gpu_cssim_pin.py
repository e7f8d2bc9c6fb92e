"""GPU: the pinning pass of the shift-searched SSIM (hrn_shift_cssim through binding.shift_cssim) - what the tests it
shipped with (tests/test_gpu_cssim.py) could not see.  Every offset's score, `out` and `stats` against the fp64 restatement in the direct
form (tests/cssim_ref.py), by the comparison the shipped tests use (cssim_cases.compare).

1. Conditioning.  The shipped scenes' maps have 15 % holes: masked pixels are zeros in X and Y, every window has a large variance and
   v = cov_norm (G X^2 - mu^2) never cancels.  cssim_ref.scene_clear is a bright (0.9), grey (0.5) or dark (0.05) frame of contrast 0.05
   (0.005 once), all clear, with one 5 x 6 blob, or with the left third masked.  The kernel as shipped missed these by up to
   1.04e-4 on the MI355X (kernel_bounds.CSSIM_MEASURED_UNCENTRED); it centres its fields per tile since, and measures 4.4e-8.
2. Every instance.  cssim_tile_kernel<T, BETA> has its own LDS layout per border; the shipped tests ran borders 0, 1, 2, 3, 8.  Borders 4,
   5, 6, 7 in both windows, the map one pixel more than one tile along both axes, on a holes scene or a clear one.
3. A tile interior along x: 3 x 3 tiles with remainders of 1.
4. The pre-pass's run of 2048 crop pixels: crops of 2047, 2048 and 2050 pixels.
5. A map is 0 / non-zero: 0.25, 3.0, -1.0, 1e-40 for 1.0 and -0.0 for 0.0 change no bit.
6. Exact ties: the lowest k of maximal score.
7. data_range: powers of two change no bit without the clip; data_range = 0.25 with the clip on data in [0, 0.25].
8. A +inf in SR: clamped to 1 under the clip; without it NaN scores exactly where the restatement has them, and no k*.
9. Cases 1 - 3 run twice, bit for bit.

Bound on a score: kernel_bounds.CSSIM_TOL_PIN = 4e-7, four times the largest value measured on the MI355X (9.73e-8, the 3 x 5 map at
border 8, uniform) rounded up to one digit, never above the project's cap CSSIM_BOUND = 1e-5 (absolute, data in [0, 1], data_range 1); the
measured values are beside it.  k* is compared where the restatement's best offset leads the runner-up by >= 10 x the cap, which
tests/test_cssim_pin_host.py asserts of every case here; the same file shows that every wrong variant of the restatement
(cssim_ref.CONTROLS) moves a score by >= 10 x the cap on these cases.

Shapes: the smallest that reach the thing named; the largest frame is 49 x 129, the most offsets 225.  The shipped tests run borders
0, 1, 2 and 8 in one window each, so test_all_eighteen_instances_launch runs every border 0 .. 8 in both windows on a 3 x 5 map."""
import numpy as np
import pytest

import cssim_cases as C
import cssim_ref as R
from kernel_bounds import CSSIM_BOUND, CSSIM_MEASURED, CSSIM_TOL_PIN

pytestmark = pytest.mark.gpu

TOL_PIN = CSSIM_TOL_PIN          # 4e-7: four times the largest measured value (9.73e-8), rounded up to one digit; kernel_bounds.py holds both


def _bits(a, b, what):
    for p, q in zip(a, b):
        assert np.array_equal(p, q, equal_nan=True) and np.array_equal(np.signbit(p), np.signbit(q)), what


def test_the_bound_is_inside_the_cap():
    assert CSSIM_MEASURED and max(v for v, _ in CSSIM_MEASURED.values()) <= TOL_PIN <= CSSIM_BOUND == 1e-5
    assert set(CSSIM_MEASURED) == set(C.FAMILIES)


@pytest.mark.parametrize("case", C.PIN_CASES, ids=[c[0] for c in C.PIN_CASES])
def test_every_offset_matches_the_restatement(case):
    """cases 1 - 4 and 9"""
    cid, family, scene, B, H, W, border, window = case
    x = C.pin_input(case)
    first = C.gpu(x, border, window)
    err = C.compare(x, border, window, f"[{family}] {cid}", key=("pin", cid), tol=TOL_PIN, min_gap=C.PIN_GAP, got=first)
    print(f"cssim pin {family} {cid}: measured {err:.3e}, / TOL_PIN {err / TOL_PIN:.3f}")
    if family != "runs":
        _bits(first, C.gpu(x, border, window), cid)


def test_all_eighteen_instances_launch():
    """borders 0 .. 8 x both windows on the smallest frame each takes; a border that fell through the launcher's switch to another
    instance would read its windows at the wrong stride, so each is also compared"""
    for window in ("gaussian", "uniform"):
        for border in range(9):
            H, W = C.map_frame(window, border, 3, 5)
            x = C.scene_batch(1, H, W)
            scores = C.ref(x, border, window, key=("inst18", H, W))[0]
            got = C.gpu(x, border, window)[2]
            fin = np.isfinite(scores)
            err = float(np.abs(got[fin] - scores[fin]).max())
            print(f"cssim pin instance border {border} {window} ({H} x {W}): measured {err:.3e}")
            assert got.shape == (1, (2 * border + 1) ** 2) and np.array_equal(np.isfinite(got), fin) and err <= TOL_PIN, (window, border)


# ----------------------------------------------------------------------------- 5. a map is 0 / non-zero
@pytest.mark.parametrize("value", [0.25, 3.0, -1.0, 1e-40, "-0.0"])
def test_a_map_is_zero_or_non_zero(value):
    s, h, m = C.scene_batch(2, 24, 30)
    assert set(np.unique(m)) == {0.0, 1.0}
    if value == "-0.0":
        m2 = np.where(m != 0, np.float32(1.0), np.float32(-0.0)).astype(np.float32)           # -0.0 counts as masked
        assert np.signbit(m2).any()
    else:
        m2 = np.where(m != 0, np.float32(value), np.float32(0.0)).astype(np.float32)
        assert (m2 != 0).sum() == (m != 0).sum() and np.abs(m2).max() == abs(np.float32(value)) != 0         # 1e-40 stays a float32 denormal
    for window in ("gaussian", "uniform"):
        _bits(C.gpu((s, h, m2), 3, window), C.gpu((s, h, m), 3, window), (value, window))


# ----------------------------------------------------------------------------- 6. exact ties
def _tie_frames(H=30, W=34):
    rng = np.random.default_rng(61)
    return rng.random((1, H, W)).astype(np.float32), np.full((1, H, W), 0.5, np.float32), np.ones((1, H, W), np.float32)


@pytest.mark.parametrize("window", ["gaussian", "uniform"])
def test_an_exact_tie_goes_to_the_lowest_k(window):
    """hr constant under a full map: every offset sees identical data, so all scores are the same bits and k* = 0"""
    x = _tie_frames()
    out, stats, got = C.gpu(x, 3, window)
    scores, k, _, _ = C.ref(x, 3, window, key=("tie", window))
    assert k[0] == 0 and np.all(scores[0] == scores[0, 0])
    assert np.all(got[0] == got[0, 0]) and stats[0, 3] == 0.0 and stats[0, 2] == got[0, 0] and abs(got[0, 0] - scores[0, 0]) <= TOL_PIN


@pytest.mark.parametrize("rows", ["first", "all but the last"])
def test_a_tie_among_the_eligible_goes_to_the_lowest_eligible_k(rows):
    """the same with the map's first 2 beta rows zero: the offsets of one u still tie exactly, and the lowest wins.  With every row but
    the last 2 beta zero, u = 0 has no clear pixel: k* is the first offset of u = 1."""
    border, nb = 3, 7
    s, h, m = _tie_frames()
    m = m.copy()
    if rows == "first":
        m[:, :2 * border] = 0.0
    else:
        m[:, :-2 * border] = 0.0
    x = (s, h, m)
    out, stats, got = C.gpu(x, border, "gaussian")
    scores, k, _, n = C.ref(x, border, "gaussian", key=("tie", rows))
    want = 0 if rows == "first" else nb
    groups = np.unique(scores[0][np.isfinite(scores[0])])
    assert k[0] == want and groups[-1] - groups[-2] >= C.PIN_GAP            # the u that wins leads the next by far more than the bound
    assert np.array_equal(np.isneginf(got[0]), n[0] == 0) and (rows == "first" or np.isneginf(got[0, :nb]).all())
    for u in range(nb):
        assert np.all(got[0, u * nb:(u + 1) * nb] == got[0, u * nb]), u
    assert stats[0, 3] == want and stats[0, 0] == n[0, want]
    fin = np.isfinite(scores[0])
    assert np.abs(got[0][fin] - scores[0][fin]).max() <= TOL_PIN


# ----------------------------------------------------------------------------- 7. data_range
@pytest.mark.parametrize("p", [-2, 3])
def test_powers_of_two_change_no_bit(p):
    for x in (C.scene_batch(1, 24, 30), C.clear_batch(1, 24, 30, 0.9, 0.05, "blob")):
        s, h, m = x
        f = np.float32(2.0 ** p)
        for window in ("gaussian", "uniform"):
            a = C.gpu((s * f, h * f, m), 3, window, clip=False, data_range=2.0 ** p)
            b = C.gpu(x, 3, window, clip=False, data_range=1.0)
            assert np.array_equal(a[2], b[2]) and np.array_equal(a[0], b[0]), (p, window)
            assert np.array_equal(a[1][:, [0, 2, 3]], b[1][:, [0, 2, 3]]) and np.array_equal(a[1][:, 1], b[1][:, 1] * 2.0 ** p), (p, window)


def test_data_range_a_quarter_with_the_clip():
    """data in [0, 0.25]: the clip to [0, 1] is idle, C1 and C2 are those of data_range 0.25; by scale invariance the error is that of the
    same frame at four times the values under data_range 1, so the bound holds as it is"""
    s, h, m = C.scene_batch(2, 24, 30)
    x = ((0.25 * np.clip(s, 0, 1)).astype(np.float32), (0.25 * h).astype(np.float32), m)
    assert x[0].max() <= 0.25 and x[1].max() <= 0.25
    C.compare(x, 3, "gaussian", "data_range 0.25", key="quarter", tol=TOL_PIN, min_gap=C.PIN_GAP, data_range=0.25)
    C.compare(x, 3, "uniform", "data_range 0.25", key="quarter", tol=TOL_PIN, min_gap=C.PIN_GAP, data_range=0.25)


# ----------------------------------------------------------------------------- 8. non-finite SR
def _inf_batch():
    s, h, m = (a.copy() for a in C.scene_batch(2, 24, 30))
    assert m[0, 12, 13] == 1.0
    s[0, 12, 13] = np.inf                      # inside the crop, under a clear pixel at the centre offset
    return s, h, m


def test_an_infinite_sr_pixel_is_clamped_to_one():
    x = _inf_batch()
    for window in ("gaussian", "uniform"):
        C.compare(x, 3, window, f"+inf clip {window}", key="inf", tol=TOL_PIN, min_gap=C.PIN_GAP, clip=True)
    clamped = (np.where(np.isinf(x[0]), np.float32(1.0), x[0]), x[1], x[2])
    _bits(C.gpu(x, 3, "gaussian"), C.gpu(clamped, 3, "gaussian"), "inf == 1")
    assert np.isfinite(C.gpu(x, 3, "gaussian")[2]).all()


def test_an_infinite_sr_pixel_without_the_clip():
    """the restatement's bias is -inf (or NaN where the pixel is masked), so every window of every offset is NaN: no offset is eligible"""
    x = _inf_batch()
    scores, k, _, _ = C.ref(x, 3, "gaussian", key="inf", clip=False)
    assert not np.isfinite(scores[0]).any() and np.isnan(scores[0]).all() and k[0] == -1 and k[1] >= 0
    out, stats, got = C.gpu(x, 3, "gaussian", clip=False)
    assert np.array_equal(np.isfinite(got), np.isfinite(scores))
    assert np.isnan(out[0]) and stats[0, 3] == -1.0 and np.isfinite(out[1]) and stats[1, 3] == k[1]
    C.compare(x, 3, "gaussian", "+inf no clip", key="inf", tol=TOL_PIN, min_gap=C.PIN_GAP, clip=False)
