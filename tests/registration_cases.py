"""What the registration pinning tests share (tests/test_gpu_registration_pin.py on the GPU, tests/test_registration_pin_host.py on the
CPU): the cases - frames whose scored pixels do not have the frame's mean (tests/registration_ref.py's scene_stepped) - their masks, the
bounds, and the comparison of a device array with the fp64 restatement.  The CPU test shows about each GPU case what the GPU test
relies on - at every point of the grids, and of the searches along the paths the fp64 restatements take - so both read the cases, the grids and the searches' parameters from here.  Nothing here needs the compiled package.

A case is (id, family, (B, V, H, W), pair, split, axis, variant).  pair names (contrast, step) in PAIRS.  variant names the masks:

    ref-hides    ref_mask = speckle x band x [dark side]; the view's mask is NULL ("null") or its speckle ("speckle")
    view-hides   view_mask = speckle x band x [dark side]; the reference's mask is NULL or its speckle
    both-sides   ref_mask = band ("null", the view's mask NULL) or speckle x band ("speckle", the view's mask its speckle): both sides
                 of the step stay clear, so every block of a local search is off the frame's mean in both images

The dark side is p < split.  The views lie at SHIFTS[:V] from the reference; the seed is the case's axis unless SEEDS replaces it."""
import functools

import numpy as np

import registration_ref as R

SCORE_BOUND = 4e-7           # DESIGN.md sections 7f / 7g: a device score against fp64 (GRID_BOUND, SCORE_BOUND of the existing tests)
DEVICE_BOUND = 8e-7          # section 7g: two device paths against each other
# tests/test_gpu_registration_scene.py's two bounds (tests/test_gpu_large_offsets_scene.py holds its alone launches to APPLY_BOUND too)
GRID_BOUND = 4e-7            # measured 8.04e-8 there, times 4; this path on an MI355X: 8.04e-8 (16 x 16), 4.3e-8 beyond
APPLY_BOUND = 8e-7           # section 7f: measured 1.77e-7 there, times 4; this path on an MI355X: 1.77e-7 (257 x 144)
ADMIT = 1e-7                 # a quarter of SCORE_BOUND: what the fp32 resampling alone may cost on a case (the admission rule)

PAIRS = {"control": (0.1, 0.0), "c0.01-s0.3": (0.01, 0.3), "c0.01-s0.6": (0.01, 0.6)}
CONTROL = "control"
SHIFTS = [(0.37, -0.62), (-1.3, 0.7), (0.0, 0.0)]
CENTRES = [(0.0, 0.0), (-1.3, 0.7), (1.75, -0.5)]               # tests/test_gpu_registration.py's
SUBS = ("null", "speckle")
GRIDS = [(7, 2.0), (7, 0.03), (4, 2.0), (4, 0.03)]              # (P, width) of the grids compared; grid k is centred on centres(V, k)
SEARCH = (7, 5, 1.0)                                            # (P, levels, radius) of the resident and the scene search compared
LOCAL_INIT = (7, 5, 1.0)                                        # tests/test_gpu_registration_local.py's searched(): the global search, then
LOCAL = (6, 4, 0.5)                                             # the local levels from its shifts
PYRAMID = dict(octaves=2, P=7, levels=6, radius=4.0, coarse_levels=3, refine_radius=1.0)
FAMILIES = ("resident", "scene", "local", "pyramid")

RESIDENT_SHAPES = [((1, 2, 24, 40), 20), ((1, 3, 33, 47), 24), ((1, 2, 128, 128), 64)]
SCENE_SHAPES = [((1, 2, 130, 203), 128, 1), ((1, 2, 130, 203), 100, 1), ((1, 2, 257, 144), 128, 0)]     # a tile seam, inside a tile, a seam
LOCAL_SHAPES = [((1, 2, 130, 203), 128, 1, 64), ((1, 2, 257, 144), 128, 0, 128)]                         # ..., block
# Where no seed admits a case, its dark side is too narrow: at 14 (24 x 40) and 18 (33 x 47) columns under the reference's mask a score is
# taken over 130 .. 360 pixels, and the fp32 resampling alone costs more than ADMIT at some point of the grids or of the search
# (tests/test_registration_pin_host.py's rule, over every compared point).  SPLITS: id -> the split that replaces the one in its name: the
# step moves right, two columns at a time, until a seed meets the rule.  SEEDS: id -> the seed that replaces the default, chosen on the
# CPU model alone for the most room under the rule among seeds 0 .. 31, or 0 .. 127 where none of those met it.
SPLITS = {"resident-24x40-c0.01-s0.3-col20-ref-hides": 26, "resident-24x40-c0.01-s0.6-col20-ref-hides": 30,
          "resident-33x47-c0.01-s0.3-col24-ref-hides": 28, "resident-33x47-c0.01-s0.6-col24-ref-hides": 32}
SEEDS = {"resident-24x40-c0.01-s0.3-col20-ref-hides": 4, "resident-24x40-c0.01-s0.3-row20-view-hides": 30,
         "resident-24x40-c0.01-s0.6-row20-ref-hides": 29, "resident-24x40-c0.01-s0.6-col20-ref-hides": 69,
         "resident-24x40-c0.01-s0.6-col20-view-hides": 127, "resident-33x47-c0.01-s0.3-col24-ref-hides": 3,
         "resident-33x47-c0.01-s0.6-row24-ref-hides": 69, "resident-33x47-c0.01-s0.6-col24-ref-hides": 30,
         "resident-33x47-c0.01-s0.6-col24-view-hides": 27, "resident-128x128-c0.01-s0.6-col64-ref-hides": 24,
         "scene-128x128-c0.01-s0.6-col64-ref-hides": 24, "pyramid-130x203-c0.01-s0.3-col128-ref-hides": 9,
         "pyramid-130x203-c0.01-s0.6-col128-ref-hides": 4}


def _cases():
    cases = []
    name = lambda fam, shape, pair, split, axis, variant: f"{fam}-{shape[2]}x{shape[3]}-{pair}-{'col' if axis else 'row'}{split}-{variant}"
    for shape, split in RESIDENT_SHAPES:
        for pair in PAIRS:
            for variant in ("ref-hides", "view-hides"):
                for axis in (0, 1):
                    cid = name("resident", shape, pair, split, axis, variant)
                    cases.append((cid, "resident", shape, pair, SPLITS.get(cid, split), axis, variant))
    for shape, split, axis in SCENE_SHAPES:
        for pair in PAIRS:
            cases.append((name("scene", shape, pair, split, axis, "ref-hides"), "scene", shape, pair, split, axis, "ref-hides"))
    for pair in PAIRS:                                           # where both paths run: the scene path against the resident one
        cases.append((name("scene", (1, 2, 128, 128), pair, 64, 1, "ref-hides"), "scene", (1, 2, 128, 128), pair, 64, 1, "ref-hides"))
    for shape, split, axis, _ in LOCAL_SHAPES:
        for pair in PAIRS:
            cases.append((name("local", shape, pair, split, axis, "both-sides"), "local", shape, pair, split, axis, "both-sides"))
    for pair in PAIRS:
        cases.append((name("pyramid", (1, 2, 130, 203), pair, 128, 1, "ref-hides"), "pyramid", (1, 2, 130, 203), pair, 128, 1, "ref-hides"))
    return cases


CASES = _cases()
BLOCK = {(shape[2], shape[3]): block for shape, _, _, block in LOCAL_SHAPES}


def family(fam):
    return [c for c in CASES if c[1] == fam]


def ids(cases):
    return [c[0] for c in cases]


@functools.lru_cache(maxsize=None)
def _frames(H, W, V, seed, pair, split, axis):
    return R.scene_stepped(H, W, SHIFTS[:V], seed, *PAIRS[pair], split, axis)


def inputs(case, sub):
    """-> (ref (1,H,W), ref_mask (1,H,W) or None, views (1,V,H,W), view_masks (1,V,H,W) or None), float32; computed once, not to be
    written to."""
    cid, _, (B, V, H, W), pair, split, axis, variant = case
    assert B == 1 and sub in SUBS
    ref, speckle, views, view_speckle, band = _frames(H, W, V, SEEDS.get(cid, axis), pair, split, axis)
    p = np.arange(W)[None, :] if axis == 1 else np.arange(H)[:, None]
    dark = np.broadcast_to(p < split, (H, W)).astype(np.float32)
    if variant == "ref-hides":
        rm, vm = speckle * band * dark, view_speckle if sub == "speckle" else None
    elif variant == "view-hides":
        rm, vm = speckle if sub == "speckle" else None, view_speckle * (band * dark)[None]
    else:
        rm, vm = (speckle * band, view_speckle) if sub == "speckle" else (band.copy(), None)
    return ref[None], None if rm is None else rm[None], views[None], None if vm is None else vm[None]


def centres(V, rotation=0):
    return np.array([[CENTRES[(v + rotation) % 3] for v in range(V)]], np.float32)


# ----------------------------------------------------------------------------- fp64, computed once
_grids = {}


def grid_ref(case, sub, centre_of_view, width, P):
    """fp64 scores (1, V, P, P) of one grid level around centre_of_view (1, V, 2)"""
    key = (case[0], case[4], SEEDS.get(case[0]), sub, np.asarray(centre_of_view, np.float32).tobytes(), float(width), P)
    if key not in _grids:
        ref, rm, views, vm = inputs(case, sub)
        V = views.shape[1]
        _grids[key] = np.stack([R.grid(ref[0], None if rm is None else rm[0], views[0, v], None if vm is None else vm[0, v],
                                       centre_of_view[0, v], np.float32(width), P)[0] for v in range(V)])[None]
    return _grids[key]


# ----------------------------------------------------------------------------- device against fp64
def in_range(got, what):
    """every finite device score is a correlation: within SCORE_BOUND of [-1, 1]"""
    got = np.asarray(got, np.float64)
    fin = np.isfinite(got)
    assert not np.isnan(got).any() and not np.isposinf(got).any(), what
    assert np.all(np.abs(got[fin]) <= 1.0 + SCORE_BOUND), (what, float(np.abs(got[fin]).max()))


def worst(got, want, what):
    """-inf entries coincide, the finite ones lie in [-1, 1]: -> the largest |device - fp64| of a finite entry (printed)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.array_equal(np.isneginf(got), np.isneginf(want)), f"{what}: -inf entries differ"
    in_range(got, what)
    fin = ~np.isneginf(want)
    w = float(np.abs(got[fin] - want[fin]).max()) if fin.any() else 0.0
    print(f"{what}: max |device - fp64| = {w:.3e} over {int(fin.sum())} finite entries, {int((~fin).sum())} of -inf")
    return w


def follow(case, sub, trace, P, levels, radius, init=None):
    """tests/test_gpu_registration.py's test_search_follows_the_fp64_scores_level_by_level along a device trace (1, V, levels, 3):
    -> (max |trace score - fp64 at the chosen point|, max (fp64 maximum of the level - fp64 at the chosen point))"""
    ref, rm, views, vm = inputs(case, sub)
    V = views.shape[1]
    in_range(trace[..., 2], case[0])
    widths = R.level_widths(P, levels, radius)
    worst_score, worst_gap = 0.0, 0.0
    for v in range(V):
        centre = (np.float32(0.0), np.float32(0.0)) if init is None else (np.float32(init[0, v, 0]), np.float32(init[0, v, 1]))
        for k in range(levels):
            want, dys, dxs = R.grid(ref[0], None if rm is None else rm[0], views[0, v], None if vm is None else vm[0, v], centre, widths[k], P)
            dy, dx, got = trace[0, v, k]
            if not np.isfinite(want).any():
                assert (dy, dx) == centre and np.isneginf(got)
                continue
            i, j = np.flatnonzero(dys == dy), np.flatnonzero(dxs == dx)
            assert len(i) and len(j), f"{case[0]} view {v} level {k}: ({dy}, {dx}) is no point of the grid {dys} x {dxs}"
            at = want[i[0], j[0]]
            assert np.isfinite(got) and np.isfinite(at), (case[0], v, k)
            worst_score, worst_gap = max(worst_score, abs(float(got) - at)), max(worst_gap, float(want.max() - at))
            centre = (dy, dx)
    return worst_score, worst_gap
