"""GPU: the masked-NCC registration for frames of any size (hrnet_hip.registration's *_scene functions over hrn_mncc_grid_scene /
hrn_mncc_search_scene / hrn_mncc_apply_scene) against the fp64 restatement (tests/registration_ref.py), which has no
size limit and is used as it is: one grid level per element, the resampled views per element, the search level by level along the
device's own path, recovery of known shifts, the LDS-resident kernels of section 7f where both run, bit-reproducibility, the independence
of a view from its batch, the custom ops, and the composition with HRNet.forward_tiled.

The tile of the scene path is 64 x 64.  The shapes give every axis one tile (16, 33, 47), exactly two (128), two with a ragged remainder
(130, 144), three or more (203, 257, 300: four, five and five) and a remainder of one pixel (257 = 4 x 64 + 1).

The bounds are section 7f's, carried over and not re-derived from this code: the arithmetic per pixel is the same (fp32 on centred data
for at most 32 pixels of a thread - 16 here - and fp64 above)."""
import functools

import numpy as np
import pytest
import torch

import registration_ref as R
from registration_cases import APPLY_BOUND, GRID_BOUND        # the bounds of this file; tests/registration_cases.py holds them

pytestmark = pytest.mark.gpu

RECOVERY_PX = 0.02           # the project's bound on every component of a recovered shift

SHAPES = [(2, 3, 16, 16), (1, 2, 33, 47), (1, 2, 128, 128), (1, 2, 130, 203), (1, 2, 257, 144), (1, 2, 16, 300)]
IDS = ["x".join(map(str, s)) for s in SHAPES]
# per rotation of the centres over the views, the (width, with masks) pairs: every width and both kinds of mask meet every centre
GRID_RUNS = [((2.0, True), (2.0, False)), ((0.03, True), (8.0, True)), ((8.0, True), (2.0, False)), ((2.0, True), (0.03, True))]
SMALL = [s for s in SHAPES if max(s[2:]) <= 128]                 # where the LDS-resident kernels run too
CENTRES = [(0.0, 0.0), (-1.3, 0.7), (1.75, -0.5), (-37.25, 41.5)]        # the last moves the window's origin far beyond any halo


@functools.lru_cache(maxsize=None)
def case(B, V, H, W, limit=0.9):
    """-> (true shifts (B,V,2), ref (B,H,W), ref_mask, views (B,V,H,W), view_masks) as numpy float32, one seeded scene per sample."""
    parts = []
    for b in range(B):
        shifts = R.random_shifts(V, limit, seed=7000 + 13 * b + H * W)
        parts.append((shifts,) + R.scene(H, W, shifts, seed=100 * b + H * W))
    return tuple(np.stack([p[i] for p in parts]) for i in range(5))


def _cuda(*arrays):
    return tuple(None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays)


def _worst(got, want, what):
    """Compare a device array with its fp64 restatement: -inf entries alike, the finite ones -> their largest difference (printed)."""
    got = np.asarray(got, np.float64)
    assert np.array_equal(np.isneginf(got), np.isneginf(want)), f"{what}: -inf entries differ"
    fin = ~np.isneginf(want)
    assert np.all(np.isfinite(got[fin]))
    worst = float(np.abs(got[fin] - want[fin]).max()) if fin.any() else 0.0
    print(f"{what}: max |device - fp64| = {worst:.3e} over {int(fin.sum())} finite entries, {int((~fin).sum())} of -inf")
    return worst


def _grid_ref(ref, ref_mask, views, view_masks, centres, width, P):
    B, V = views.shape[:2]
    return np.stack([np.stack([R.grid(ref[b], None if ref_mask is None else ref_mask[b], views[b, v],
                                      None if view_masks is None else view_masks[b, v], centres[b, v], np.float32(width), P)[0]
                               for v in range(V)]) for b in range(B)])


# ----------------------------------------------------------------------------- one grid level, per element
@pytest.mark.parametrize("P", [7, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_grid_level_matches_fp64_per_element(shape, P):
    """Every view meets every centre: rotation c0 gives view (b, v) the centre (b + v + c0) % 4."""
    from hrnet_hip import registration as G
    B, V, H, W = shape
    _, ref, ref_mask, views, view_masks = (a.copy() for a in case(*shape))
    view_masks[0, V - 1] = 0.0                                   # a fully masked view
    if B > 1:
        ref_mask[1] = 0.0                                        # a fully masked reference
    worst = 0.0
    for c0 in range(4):
        centres = np.array([[CENTRES[(b + v + c0) % 4] for v in range(V)] for b in range(B)], np.float32)
        far = np.all(centres == np.float32(CENTRES[3]), axis=-1)
        for width, masks in GRID_RUNS[c0]:
            rm, vm = (ref_mask, view_masks) if masks else (None, None)
            got = G.mncc_grid_scene(*_cuda(views, vm, ref, rm, centres), points_per_dim=P, width=width).cpu().numpy()
            assert got.shape == (B, V, P, P)
            want = _grid_ref(ref, rm, views, vm, centres, width, P)
            if masks:
                assert np.all(np.isneginf(want[0, V - 1])) and (B == 1 or np.all(np.isneginf(want[1])))
            if H <= 36 or W <= 40:                               # rows y - 34 - 2 >= 0 or columns x + 37 + 3 <= W - 1: there are none
                assert np.all(np.isneginf(want[far])) and np.all(np.isneginf(got[far]))
            worst = max(worst, _worst(got, want, f"grid_scene {shape} P={P} rotation {c0} width={width} masks={masks}"))
    print(f"grid_scene {shape} P={P}: worst {worst:.3e}")
    assert worst <= GRID_BOUND


@pytest.mark.parametrize("shape", SMALL, ids=["x".join(map(str, s)) for s in SMALL])
def test_scene_path_agrees_with_the_lds_kernels(shape):
    """Where both run: the scores within twice the bound (both are within it of fp64), the resampled views bit for bit."""
    from hrnet_hip import registration as G
    B, V, H, W = shape
    _, ref, ref_mask, views, view_masks = case(*shape)
    worst = 0.0
    for c0 in range(3):
        centres = np.array([[CENTRES[(b + v + c0) % 3] for v in range(V)] for b in range(B)], np.float32)
        for masks in (True, False):
            d = _cuda(views, view_masks if masks else None, ref, ref_mask if masks else None, centres)
            for P, width in ((7, 2.0), (4, 0.03), (5, 8.0)):
                a, b = G.mncc_grid_scene(*d, points_per_dim=P, width=width), G.mncc_grid(*d, points_per_dim=P, width=width)
                assert torch.equal(torch.isneginf(a), torch.isneginf(b))
                fin = ~torch.isneginf(b)
                worst = max(worst, float((a[fin].double() - b[fin].double()).abs().max()) if fin.any() else 0.0)
            shifts = torch.from_numpy(centres).cuda() * 1.7
            got, want = G.shift_scene(d[0], d[1], shifts), G.shift_views(d[0], d[1], shifts)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    print(f"scene against LDS {shape}: max |grid_scene - grid| = {worst:.3e}")
    assert worst <= 2 * GRID_BOUND


# ----------------------------------------------------------------------------- the resampled views, per element
APPLY_SHIFTS = [(0.37, -1.62), (-3.5, 2.25)]


@functools.lru_cache(maxsize=None)
def searched(shape):
    """The device's own shifts for a case: P = 7, 5 levels, radius 1 -> (shifts, trace) as numpy."""
    from hrnet_hip import registration as G
    _, ref, ref_mask, views, view_masks = case(*shape)
    shifts, trace = G.mncc_search_scene(*_cuda(views, view_masks, ref, ref_mask), points_per_dim=7, levels=5, radius=1.0, return_trace=True)
    return shifts.cpu().numpy(), trace.cpu().numpy()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_shift_scene_matches_fp64_per_element(shape):
    """`valid` is compared at every pixel.  Where the bilinear mask sample is exactly 0.5 - the half-pixel shift -3.5 puts every
    horizontal mask edge and the frame's own edge there - the definition decides (> is strict) and the device's fp64 table decides alike;
    what would make the comparison a matter of rounding is a sample within 1e-9 of 0.5 and not on it: the shifts have none, asserted."""
    from hrnet_hip import registration as G
    B, V, H, W = shape
    _, _, _, views, view_masks = case(*shape)
    fixed = [np.array([[APPLY_SHIFTS[(b + v + k) % 2] for v in range(V)] for b in range(B)], np.float32) for k in range(2)]
    worst, near = 0.0, 0
    for shifts in fixed + [searched(shape)[0]]:
        for masks in (view_masks, None):
            out, valid = G.shift_scene(*_cuda(views, masks, shifts))
            out, valid = out.cpu().numpy(), valid.cpu().numpy()
            for b in range(B):
                for v in range(V):
                    m = np.ones((H, W)) if masks is None else masks[b, v]
                    off = np.abs(R.mask_bilinear(m, shifts[b, v]) - 0.5)
                    near += int(((off > 0.0) & (off <= 1e-9)).sum())
                    want_valid = R.shifted_mask(m, shifts[b, v])
                    assert np.array_equal(valid[b, v], want_valid.astype(np.float32))
                    assert np.all(out[b, v][~want_valid] == 0.0)
                    want = R.sample(views[b, v], shifts[b, v])
                    worst = max(worst, float(np.abs(out[b, v] - want)[want_valid].max()) if want_valid.any() else 0.0)
    print(f"shift_scene {shape}: max |device - fp64| = {worst:.3e}; {near} pixels with the fp64 bilinear mask within 1e-9 of 0.5 and off it")
    assert near == 0
    assert worst <= APPLY_BOUND


# ----------------------------------------------------------------------------- the search, level by level along the device's own path
def _follow(shape, P, levels, radius, zero_last=True):
    from hrnet_hip import registration as G
    B, V, H, W = shape
    _, ref, ref_mask, views, view_masks = (a.copy() for a in case(*shape))
    if zero_last:
        views[0, V - 1] = 0.0                                    # a padded view: shift (0, 0), score -inf
    shifts, trace = G.mncc_search_scene(*_cuda(views, view_masks, ref, ref_mask), points_per_dim=P, levels=levels, radius=radius,
                                        return_trace=True)
    shifts, trace = shifts.cpu().numpy(), trace.cpu().numpy()
    assert shifts.shape == (B, V, 2) and trace.shape == (B, V, levels, 3)
    assert np.array_equal(shifts, trace[:, :, -1, :2])
    if zero_last:
        assert np.all(shifts[0, V - 1] == 0.0) and np.all(trace[0, V - 1, :, :2] == 0.0) and np.all(np.isneginf(trace[0, V - 1, :, 2]))
    widths = R.level_widths(P, levels, radius)
    worst_score, worst_gap, reach = 0.0, 0.0, 0.0
    for b in range(B):
        for v in range(V):
            centre = (np.float32(0.0), np.float32(0.0))
            for k in range(levels):
                want, dys, dxs = R.grid(ref[b], ref_mask[b], views[b, v], view_masks[b, v], centre, widths[k], P)
                dy, dx, got = trace[b, v, k]
                if not np.isfinite(want).any():
                    assert (dy, dx) == centre and np.isneginf(got)
                    continue
                i, j = np.flatnonzero(dys == dy), np.flatnonzero(dxs == dx)
                assert len(i) and len(j), f"view {b},{v} level {k}: ({dy}, {dx}) is no point of the grid {dys} x {dxs}"
                at = want[i[0], j[0]]
                worst_score, worst_gap = max(worst_score, abs(got - at)), max(worst_gap, want.max() - at)
                centre = (dy, dx)
                reach = max(reach, abs(float(dy)), abs(float(dx)))
    print(f"search_scene {shape} P={P} levels={levels} radius {radius}: max |trace score - fp64 at the chosen point| = {worst_score:.3e}, "
          f"max (fp64 maximum - fp64 at the chosen point) = {worst_gap:.3e}, farthest centre {reach:.2f} px")
    assert worst_score <= GRID_BOUND and worst_gap <= 2 * GRID_BOUND


@pytest.mark.parametrize("radius", [1.0, 4.0])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_search_follows_the_fp64_scores_level_by_level(shape, radius):
    _follow(shape, 7, 5, radius)


@pytest.mark.parametrize("shape", [(1, 2, 33, 47), (1, 2, 130, 203)], ids=["1x2x33x47", "1x2x130x203"])
def test_search_that_wanders_follows_the_fp64_scores(shape):
    """P = 3 narrows by 0.9 a level: sixteen levels of radius 4 may carry the centre tens of pixels away, and the window goes with it."""
    _follow(shape, 3, 16, 4.0, zero_last=False)


# ----------------------------------------------------------------------------- known shifts
RECOVERY = [((1, 2, 130, 203), 0.9, 1.0, 5), ((1, 2, 257, 144), 0.9, 1.0, 5), ((1, 2, 16, 300), 0.9, 1.0, 5), ((1, 2, 200, 136), 3.5, 4.0, 7),
            ((1, 2, 130, 203), 1.8, 2.0, 6)]


@pytest.mark.parametrize("shape,limit,radius,levels", RECOVERY, ids=[f"{s[2]}x{s[3]}_r{int(r)}" for s, _, r, _ in RECOVERY])
def test_search_recovers_known_shifts(shape, limit, radius, levels):
    from hrnet_hip import registration as G
    true, ref, ref_mask, views, view_masks = case(*shape, limit=limit)
    got = G.mncc_search_scene(*_cuda(views, view_masks, ref, ref_mask), points_per_dim=7, levels=levels, radius=radius).cpu().numpy()
    err = np.abs(got - true)
    print(f"recovery {shape} shifts +-{limit} radius {radius} levels {levels}: worst component error {err.max():.4f} px")
    assert err.max() <= RECOVERY_PX


# ----------------------------------------------------------------------------- reproducibility and independence
def test_search_is_bit_reproducible_and_every_level_is_the_grid():
    """P = 4 and P = 6 halve and quarter the width, so every level's width is an fp32 value and mncc_grid_scene can be given it."""
    from hrnet_hip import registration as G
    shape = (2, 3, 70, 90)
    _, ref, ref_mask, views, view_masks = case(*shape)
    d = _cuda(views, view_masks, ref, ref_mask)
    for P, levels, radius in ((4, 4, 1.0), (6, 3, 1.5), (7, 1, 4.0)):
        runs = [G.mncc_search_scene(*d, points_per_dim=P, levels=levels, radius=radius, return_trace=True) for _ in range(2)]
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
        trace = runs[0][1].cpu().numpy()
        centres = np.zeros(shape[:2] + (2,), np.float32)
        for k, width in enumerate(R.level_widths(P, levels, radius)):
            assert float(np.float32(width)) == width
            scores = G.mncc_grid_scene(*d, centres=torch.from_numpy(centres).cuda(), points_per_dim=P, width=width).cpu().numpy()
            for b in range(shape[0]):
                for v in range(shape[1]):
                    dys, dxs = R.grid_coords(centres[b, v, 0], width, P), R.grid_coords(centres[b, v, 1], width, P)
                    at, best = R.best_of(scores[b, v], dys, dxs, centres[b, v])
                    assert (trace[b, v, k, 0], trace[b, v, k, 1]) == at, (P, k, b, v)
                    assert np.float32(best).tobytes() == trace[b, v, k, 2].tobytes(), (P, k, b, v)
            centres = trace[:, :, k, :2].copy()


def test_a_view_searched_alone_gives_what_it_gives_in_its_batch():
    """The workspace is indexed by view and tile: a view's sums must not meet another's."""
    from hrnet_hip import registration as G
    shape = (2, 3, 70, 90)
    _, ref, ref_mask, views, view_masks = case(*shape)
    d = _cuda(views, view_masks, ref, ref_mask)
    shifts, trace = G.mncc_search_scene(*d, levels=4, radius=2.0, return_trace=True)
    scores = G.mncc_grid_scene(*d, points_per_dim=5, width=3.0)
    applied = G.shift_scene(d[0], d[1], shifts)
    for b, v in ((1, 2), (0, 1), (1, 0)):
        one = (d[0][b:b + 1, v:v + 1], d[1][b:b + 1, v:v + 1], d[2][b:b + 1], d[3][b:b + 1])
        s1, t1 = G.mncc_search_scene(*one, levels=4, radius=2.0, return_trace=True)
        assert torch.equal(s1[0, 0], shifts[b, v]) and torch.equal(t1[0, 0], trace[b, v])
        assert torch.equal(G.mncc_grid_scene(*one, points_per_dim=5, width=3.0)[0, 0], scores[b, v])
        a1 = G.shift_scene(one[0], one[1], s1)
        assert torch.equal(a1[0][0, 0], applied[0][b, v]) and torch.equal(a1[1][0, 0], applied[1][b, v])


def test_register_scene_is_search_then_shift():
    from hrnet_hip import registration as G
    _, ref, ref_mask, views, view_masks = case(1, 2, 130, 203)
    d = _cuda(views, view_masks)
    kw = dict(ref=torch.from_numpy(ref).cuda(), ref_mask=torch.from_numpy(ref_mask).cuda(), points_per_dim=5, levels=3, radius=1.5)
    registered, valid, shifts = G.register_scene(*d, **kw)
    assert torch.equal(shifts, G.mncc_search_scene(*d, **kw))
    want = G.shift_scene(*d, shifts)
    assert torch.equal(registered, want[0]) and torch.equal(valid, want[1])
    assert set(valid.unique().tolist()) == {0.0, 1.0}


# ----------------------------------------------------------------------------- the custom ops
def test_ops_are_the_binding_calls_and_pass_opcheck():
    from hrnet_hip import binding
    ops = torch.ops.hrnet_hip
    _, ref, ref_mask, views, view_masks = case(1, 2, 70, 90)
    views, view_masks, ref, ref_mask = _cuda(views, view_masks, ref, ref_mask)
    centres = torch.tensor([[[0.25, -0.5], [0.0, 0.0]]], device="cuda")
    assert torch.equal(ops.mncc_grid_scene(ref, ref_mask, views, view_masks, centres, 5, 0.5),
                       binding.mncc_grid_scene(ref, ref_mask, views, view_masks, centres, 5, 0.5))
    got = ops.mncc_search_scene(ref, None, views, view_masks, 4, 3, 1.0)
    want = binding.mncc_search_scene(ref, None, views, view_masks, 4, 3, 1.0)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    got, want = ops.shift_scene(views, view_masks, centres), binding.mncc_apply_scene(views, view_masks, centres)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    checks = ("test_schema", "test_faketensor")
    torch.library.opcheck(ops.mncc_grid_scene.default, (ref, ref_mask, views, view_masks, centres, 5, 0.5), test_utils=checks)
    torch.library.opcheck(ops.mncc_grid_scene.default, (ref, None, views, None, centres, 3, 2.0), test_utils=checks)
    torch.library.opcheck(ops.mncc_search_scene.default, (ref, ref_mask, views, view_masks, 4, 3, 1.0), test_utils=checks)
    torch.library.opcheck(ops.mncc_search_scene.default, (ref, None, views, None, 4, 3, 1.0), test_utils=checks)
    torch.library.opcheck(ops.shift_scene.default, (views, view_masks, centres), test_utils=checks)
    torch.library.opcheck(ops.shift_scene.default, (views, None, centres), test_utils=checks)


# ----------------------------------------------------------------------------- composition with tiled inference
def test_register_scene_then_forward_tiled():
    """A 144 x 200 scene of 4 views, registered and super-resolved at tile 32, the smallest the tiled tests use; and the tiled forward of
    the unregistered scene does not notice a registration in the process."""
    from DeepNetworks.HRNet import HRNet
    from hrnet_hip import registration as G
    from oracle import weights
    net = HRNet(weights.HRNET_CONFIG)
    net.load_state_dict(weights.to_torch_state(weights.hrnet_state(1234)))
    net = net.cuda().eval()
    true, ref, ref_mask, views, view_masks = case(1, 3, 144, 200)
    lrs = torch.from_numpy(np.concatenate([ref[:, None], views], 1)).cuda()
    masks = torch.from_numpy(np.concatenate([ref_mask[:, None], view_masks], 1)).cuda()
    alphas = torch.ones(1, 4, device="cuda")
    with torch.no_grad():
        before = net.forward_tiled(lrs, alphas, 32).clone()
        registered, valid, shifts = G.register_scene(lrs, masks, levels=5)
        assert torch.all(shifts[0, 0] == 0.0) and np.abs(shifts[0, 1:].cpu().numpy() - true[0]).max() <= RECOVERY_PX
        sr = net.forward_tiled(registered, alphas, 32)
        after = net.forward_tiled(lrs, alphas, 32)
    assert tuple(sr.shape) == (1, 1, 432, 600) and bool(torch.isfinite(sr).all())
    assert torch.equal(before, after)
