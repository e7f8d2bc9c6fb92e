"""CPU: what tests/test_gpu_registration_pin.py relies on, shown without a GPU on a float32 model of the kernels' arithmetic (`model`
below: a model, not a reference and not the kernel - fp32 means, fp32 taps, the written-out fmaf chains of the two passes on the centred
view, then the five sums either per thread in fp32 in the kernels' own layout, runs of 8 rows of a column, 16 pixels a thread on the tiled
paths and 32 on the resident one, or in fp64).

The points of a case are the ones its GPU tests compare (registration_cases.py holds the grids and the searches' parameters for both):

- resident, scene: every point of the four grids (P = 7 and 4, widths 2 and 0.03, each around the centres the GPU test gives it), and
  every point of every level of the search (P = 7, five levels of radius 1) along the path the fp64 restatement takes;
- local: per view the fp64 global search, then every point of the four local levels (P = 6, radius 0.5) of every block along the fp64
  path from it;
- pyramid: every point of the last level of each of the three octaves along the fp64 pyramid's path, on frames reduced in fp64 and
  rounded to fp32 (the GPU test compares an octave's last chosen point).

A device search chooses among the points of the same grids as long as it chooses the point fp64 does; where two fp64 scores of a level
lie within the bound of each other it may take the other, and its later grids are then shifted by less than a spacing of that level
from the ones walked here.  That is the one thing this test cannot show about the points compared on the GPU.

At every such point of every case:

- the admission rule: with fp64 sums the model is within 1e-7 of the fp64 restatement - a quarter of the project's 4e-7 - so that what
  a case measures on the device beyond that is a summation's, not the fp32 resampling's that the definition allows;
- on a control (registration_ref.scene's own contrast and no step) the model with per-thread fp32 sums is within 4e-7 as well;

and on a conditioning case the model with per-thread fp32 sums misses the restatement by more than 4e-7 at one point at least: the case
pins something.  The figures are printed.  Nothing here is measured on a GPU: tests/kernel_bounds.py records what the kernels gave."""
import functools

import numpy as np
import pytest

import registration_cases as C
import registration_local_ref as L
import registration_pyramid_ref as Y
import registration_ref as R

# ----------------------------------------------------------------------------- a float32 model of the kernels' arithmetic
# The operations are the kernels' own: the images centred on the fp32 means of their own masks over the whole frame, fp32 taps, the
# written-out fmaf chains of the two passes, then the five sums.  fmaf(a, b, c) is a b + c in fp64 (the product is exact there) rounded
# to fp32.
F32 = np.float32
RESIDENT_THREADS, SCENE_TILE, RUN = 512, 64, 8


def _fma32(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def _masked_mean32(x, mask):
    m = np.ones(x.shape, bool) if mask is None else np.asarray(mask) != 0
    return F32(np.asarray(x, np.float64)[m].sum() / m.sum()) if m.any() else F32(0.0)


def sample_f32(T, shift):
    """registration_ref.sample as the kernels do it, on an fp32 plane: (H, W) float32; 0 where the footprint leaves the frame."""
    T = np.asarray(T, F32)
    H, W = T.shape
    (ny, fy), (nx, fx) = R.split(shift[0]), R.split(shift[1])
    ky, kx = R.taps(fy).astype(F32), R.taps(fx).astype(F32)
    out = np.zeros((H, W), F32)
    (y0, y1), (x0, x1) = R._axis(ny, H), R._axis(nx, W)
    if y0 >= y1 or x0 >= x1:
        return out
    cols = lambda o: T[:, x0 + nx + o:x1 + nx + o]
    A = kx[0] * cols(R.TAPS[0])
    for o, k in zip(R.TAPS[1:], kx[1:]):
        A = _fma32(np.broadcast_to(k, A.shape), cols(o), A)
    rows = lambda o: A[y0 + ny + o:y1 + ny + o]
    t = ky[0] * rows(R.TAPS[0])
    for o, k in zip(R.TAPS[1:], ky[1:]):
        t = _fma32(np.broadcast_to(k, t.shape), rows(o), t)
    out[y0:y1, x0:x1] = t
    return out


@functools.lru_cache(maxsize=None)
def thread_pixels(H, W, path):
    """(threads, pixels a thread) flat pixel indices in the order a thread of the kernels adds them, -1 where it has none.  "resident":
    registration.hip, 512 threads of four runs of 8 rows of a column, run `item` = tid + 512 k at column item % W, rows 8 (item // W);
    "scene": mncc_scene.h's scene_level, per tile of 64 x 64 a thread (wave, lane) takes rows 8 (wave + 4 k) .. + 7, k < 2, of column lane."""
    p = np.arange(RUN)
    if path == "resident":
        item = np.arange(RESIDENT_THREADS)[:, None] + RESIDENT_THREADS * np.arange(4)[None, :]
        x, y = (item % W)[..., None], (item // W * RUN)[..., None] + p
        idx = np.where((item[..., None] < W * ((H + RUN - 1) // RUN)) & (y < H), y * W + x, -1)
        return idx.reshape(RESIDENT_THREADS, 4 * RUN)
    out = []
    for ty0 in range(0, H, SCENE_TILE):
        for tx0 in range(0, W, SCENE_TILE):
            wave, lane = np.arange(4)[:, None, None, None], np.arange(64)[None, :, None, None]
            y = ty0 + (wave + 4 * np.arange(2)[None, None, :, None]) * RUN + p
            x = np.broadcast_to(tx0 + lane, np.broadcast_shapes(y.shape, lane.shape))
            y = np.broadcast_to(y, x.shape)
            out.append(np.where((y < H) & (x < W), y * W + x, -1).reshape(4 * 64, 2 * RUN))
    return np.concatenate(out)


def _finish(s):
    n = s[0]
    if n == 0:
        return -np.inf
    mt, mr = s[1] / n, s[2] / n
    vt, vr = s[3] / n - mt * mt, s[4] / n - mr * mr
    if not (vt > 0.0 and vr > 0.0):
        return -np.inf
    return float(F32((s[5] / n - mr * mt) / (np.sqrt(vr) * np.sqrt(vt))))


def model(ref, ref_mask, view, view_mask, shift, path, mean_mask="same"):
    """The model's two scores at one point -> (ideal, shipped), fp32 scores as floats.  Both add the same fp32 values t, r, t^2, r^2,
    r t of the common pixels: `ideal` in fp64 (what the definition allows the fp32 resampling to cost), `shipped` a thread's in fp32 in
    its order and the threads in fp64 (what the kernels shipped with); path "resident" or "scene" lays the pixels out over the threads.
    mean_mask: the reference mask its mean is taken under, where that is not ref_mask - the local search restricts ref_mask to a block
    and keeps the frame's mean."""
    ref, view = np.asarray(ref, F32), np.asarray(view, F32)
    H, W = ref.shape
    rm = np.ones(ref.shape, bool) if ref_mask is None else np.asarray(ref_mask) != 0
    vm = np.ones(ref.shape) if view_mask is None else (np.asarray(view_mask) != 0).astype(np.float64)
    c = (rm & R.shifted_mask(vm, shift)).ravel()
    t = sample_f32(view - _masked_mean32(view, view_mask), shift).ravel()
    r = (ref - _masked_mean32(ref, ref_mask if isinstance(mean_mask, str) else mean_mask)).ravel()
    t64, r64 = t[c].astype(np.float64), r[c].astype(np.float64)
    ideal = _finish([float(c.sum()), t64.sum(), r64.sum(), (t64 * t64).sum(), (r64 * r64).sum(), (r64 * t64).sum()])
    idx = thread_pixels(H, W, path)
    at = np.maximum(idx, 0)
    on = (idx >= 0) & c[at]
    tm, rmv = np.where(on, t[at], F32(0.0)), np.where(on, r[at], F32(0.0))
    acc = [np.zeros(len(idx), F32) for _ in range(5)]
    for j in range(idx.shape[1]):
        a, b = tm[:, j], rmv[:, j]
        acc[0], acc[1] = acc[0] + a, acc[1] + b
        acc[2], acc[3], acc[4] = _fma32(a, a, acc[2]), _fma32(b, b, acc[3]), _fma32(b, a, acc[4])
    return ideal, _finish([float(on.sum())] + [float(v.astype(np.float64).sum()) for v in acc])


# ----------------------------------------------------------------------------- the cases and their points
def test_the_cases_are_the_ones_named():
    assert C.SCORE_BOUND == 4e-7 and C.DEVICE_BOUND == 8e-7 and C.ADMIT == C.SCORE_BOUND / 4
    assert C.PAIRS == {"control": (0.1, 0.0), "c0.01-s0.3": (0.01, 0.3), "c0.01-s0.6": (0.01, 0.6)}
    assert C.GRIDS == [(7, 2.0), (7, 0.03), (4, 2.0), (4, 0.03)] and C.SEARCH == (7, 5, 1.0) and C.LOCAL == (6, 4, 0.5)
    assert len({c[0] for c in C.CASES}) == len(C.CASES) and set(C.SEEDS) <= {c[0] for c in C.CASES}
    res = C.family("resident")
    assert len(res) == 3 * 3 * 2 * 2
    assert {(c[2], c[4]) for c in res if c[0] not in C.SPLITS} <= {((1, 2, 24, 40), 20), ((1, 3, 33, 47), 24), ((1, 2, 128, 128), 64)}
    assert {c[2] for c in res} == {(1, 2, 24, 40), (1, 3, 33, 47), (1, 2, 128, 128)}
    for cid, split in C.SPLITS.items():                          # a replaced split keeps the band inside the frame and both sides scored
        case = next(c for c in res if c[0] == cid)
        assert case[4] == split and split - R.STEP_BAND - 3 >= 0 and split + R.STEP_BAND + 3 <= case[2][3 if case[5] else 2]
    assert {c[2:6] for c in C.family("scene")} == {(s, p, sp, a) for p in C.PAIRS for s, sp, a in C.SCENE_SHAPES + [((1, 2, 128, 128), 64, 1)]}
    assert all(sp % SCENE_TILE == 0 for _, sp, _, _ in C.LOCAL_SHAPES) and [sp % SCENE_TILE for _, sp, _ in C.SCENE_SHAPES] == [0, 36, 0]
    assert all(c[6] == "ref-hides" for c in C.family("scene") + C.family("pyramid")) and all(c[6] == "both-sides" for c in C.family("local"))


def test_the_band_keeps_every_footprint_on_its_side_of_the_step():
    """for shifts within +-2 pixels: the footprint of a common pixel p is p + n - 2 .. p + n + 3, n = floor(d) in -2 .. 1 (and 2 at d = 2)"""
    for axis, (H, W, split) in ((1, (24, 40, 20)), (0, (33, 47, 24))):
        band = R.scene_stepped(H, W, [(0.0, 0.0)], 0, 0.01, 0.3, split, axis)[4]
        line = band[0] if axis == 1 else band[:, 0]
        assert np.flatnonzero(line == 0).tolist() == list(range(split - 6, split + 6))
        for p in np.flatnonzero(line):
            for n in (-2, -1, 0, 1, 2):
                assert (p + n + 3 < split) if p < split else (p + n - 2 >= split)


def _walk(ref, rm, view, vm, init, P, levels, radius, keep=None):
    """The fp64 search from `init`: -> ([((dy, dx), fp64 score)] of every grid point of the levels in `keep` (None: all), the shift)"""
    centre, out = (np.float32(init[0]), np.float32(init[1])), []
    for k, w in enumerate(R.level_widths(P, levels, radius)):
        s, dys, dxs = R.grid(ref, rm, view, vm, centre, w, P)
        if keep is None or k in keep:
            out += [((dy, dx), s[i, j]) for i, dy in enumerate(dys) for j, dx in enumerate(dxs)]
        centre, _ = R.best_of(s, dys, dxs, centre)
    return out, centre


def points(case, sub):
    """[(what, ref, ref_mask, view, view_mask, shift, path, mean_mask, restatement)] of a case's compared points"""
    _, fam, (B, V, H, W), *_ = case
    ref, rm, views, vm = C.inputs(case, sub)
    rm0 = None if rm is None else rm[0]
    masks = [None if vm is None else vm[0, v] for v in range(V)]
    path = "resident" if fam == "resident" else "scene"
    out = []
    if fam in ("resident", "scene"):
        for rotation, (P, width) in enumerate(C.GRIDS):
            centres = C.centres(V, rotation)
            want = C.grid_ref(case, sub, centres, width, P)
            for v in range(V):
                dys, dxs = R.grid_coords(centres[0, v, 0], width, P), R.grid_coords(centres[0, v, 1], width, P)
                out += [(f"grid P={P} view {v} ({dy}, {dx})", ref[0], rm0, views[0, v], masks[v], (dy, dx), path, "same", want[0, v, i, j])
                        for i, dy in enumerate(dys) for j, dx in enumerate(dxs)]
        for v in range(V):
            walked, _ = _walk(ref[0], rm0, views[0, v], masks[v], (0.0, 0.0), *C.SEARCH)
            out += [(f"search view {v} {at}", ref[0], rm0, views[0, v], masks[v], at, path, "same", want) for at, want in walked]
    if fam == "pyramid":
        K = C.PYRAMID["octaves"]
        refs = Y.octaves_of(ref[0], rm0, K)
        for v in range(V):
            octs, shift = Y.octaves_of(views[0, v], masks[v], K), np.zeros(2, np.float32)
            for k in range(K, -1, -1):
                levels = C.PYRAMID["levels"] if k == 0 else C.PYRAMID["coarse_levels"]
                a = (refs[k][0], refs[k][1], octs[k][0], octs[k][1])
                walked, shift = _walk(*a, (0.0, 0.0) if k == K else np.float32(2.0) * np.asarray(shift, np.float32), C.PYRAMID["P"], levels,
                                      C.PYRAMID["radius"] if k == K else C.PYRAMID["refine_radius"], keep=(levels - 1,))
                out += [(f"octave {k} view {v} {at}",) + a + (at, "scene", "same", want) for at, want in walked]
    if fam == "local":
        block = C.BLOCK[(H, W)]
        for v in range(V):
            _, init = _walk(ref[0], rm0, views[0, v], masks[v], (0.0, 0.0), *C.LOCAL_INIT, keep=())
            for rows in L.bounds(H, block):
                for cols in L.bounds(W, block):
                    restricted = L.restricted(rm0, (H, W), rows, cols)
                    walked, _ = _walk(ref[0], restricted, views[0, v], masks[v], init, *C.LOCAL)
                    out += [(f"block {rows} x {cols} view {v} {at}", ref[0], restricted, views[0, v], masks[v], at, "scene", rm0, want)
                            for at, want in walked]
    return out


def measure(case):
    """-> (ideal, where, shipped, compared): the largest |model with fp64 sums - restatement| over a case's points and where, the largest
    |model with per-thread fp32 sums - restatement|, the number of finite points"""
    ideal, where, shipped, compared = 0.0, "", 0.0, 0
    for sub in C.SUBS:
        for what, ref, rm, view, view_mask, shift, path, mean_mask, want in points(case, sub):
            a, b = model(ref, rm, view, view_mask, shift, path, mean_mask)
            assert np.isneginf(a) == np.isneginf(want) and np.isneginf(b) == np.isneginf(want), (case[0], sub, what)
            if np.isfinite(want):
                if abs(a - want) >= ideal:
                    ideal, where = abs(a - want), f"{sub} {what}"
                shipped, compared = max(shipped, abs(b - want)), compared + 1
    return ideal, where, shipped, compared


@pytest.mark.parametrize("case", C.CASES, ids=C.ids(C.CASES))
def test_a_case_is_admitted_and_pins_the_summation(case):
    ideal, where, shipped, compared = measure(case)
    print(f"registration float32 model {case[0]}: over {compared} points, fp64 sums {ideal:.2e} ({where}), per-thread fp32 sums {shipped:.2e}")
    assert compared > 0
    assert ideal <= C.ADMIT, (case[0], where, ideal, "not admitted: replace the seed or the split (registration_cases.SEEDS, SPLITS)")
    if case[3] == C.CONTROL:
        assert shipped <= C.SCORE_BOUND
    else:
        assert shipped > C.SCORE_BOUND, (case[0], shipped, "pins nothing: replace the seed (registration_cases.SEEDS)")
