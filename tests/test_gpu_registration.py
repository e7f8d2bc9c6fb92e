"""GPU: the masked-NCC registration search (hrnet_hip.registration over hrn_mncc_grid / hrn_mncc_search / hrn_mncc_apply, DESIGN.md section
7f) against its fp64 restatement (tests/registration_ref.py): one grid level per element, the search level by level around the device's
own path, recovery of known shifts, bit-reproducibility, the resampled views per element, the custom ops, and that HRNet.forward does
not notice any of it.

The two bounds below were measured, not assumed (DESIGN.md section 7f records the figures): the largest |device - fp64| over the cases of
the grid test and of the apply test on an MI355X, times 4 for the variation between seeds, rounded up to one significant digit."""
import functools

import numpy as np
import pytest
import torch

import registration_ref as R

pytestmark = pytest.mark.gpu

GRID_BOUND = 4e-7            # measured 8.04e-8 over the cases of test_grid_level_matches_fp64_per_element (a score near 1 is rounded to fp32: 6e-8)
APPLY_BOUND = 8e-7           # measured 1.77e-7 over the cases of test_shift_views_matches_fp64_per_element (values up to 0.7 in fp32)
RECOVERY_PX = 0.02           # the issue's bound on every component of a recovered shift

SHAPES = [(2, 3, 16, 16), (1, 2, 24, 40), (1, 3, 33, 47), (1, 2, 128, 128)]
IDS = ["x".join(map(str, s)) for s in SHAPES]
CENTRES = [(0.0, 0.0), (-1.3, 0.7), (1.75, -0.5)]


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


# ----------------------------------------------------------------------------- one grid level, per element
@pytest.mark.parametrize("P", [7, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_grid_level_matches_fp64_per_element(shape, P):
    from hrnet_hip import registration as G
    B, V, H, W = shape
    _, ref, ref_mask, views, view_masks = (a.copy() for a in case(*shape))
    view_masks[0, V - 1] = 0.0                                   # a fully masked view
    if B > 1:
        ref_mask[1] = 0.0                                        # a fully masked reference
    centres = np.array([[CENTRES[(b + v) % 3] for v in range(V)] for b in range(B)], np.float32)
    worst = 0.0
    for width in (2.0, 0.03):
        got = G.mncc_grid(*_cuda(views, view_masks, ref, ref_mask, centres), points_per_dim=P, width=width).cpu().numpy()
        assert got.shape == (B, V, P, P)
        want = np.stack([np.stack([R.grid(ref[b], ref_mask[b], views[b, v], view_masks[b, v], centres[b, v], np.float32(width), P)[0]
                                   for v in range(V)]) for b in range(B)])
        assert np.all(np.isneginf(want[0, V - 1])) and (B == 1 or np.all(np.isneginf(want[1])))
        worst = max(worst, _worst(got, want, f"grid {shape} P={P} width={width}"))
    # no masks at all: NULL pointers
    got = G.mncc_grid(*_cuda(views, None, ref, None, centres), points_per_dim=P, width=2.0).cpu().numpy()
    want = np.stack([np.stack([R.grid(ref[b], None, views[b, v], None, centres[b, v], 2.0, P)[0] for v in range(V)]) for b in range(B)])
    worst = max(worst, _worst(got, want, f"grid {shape} P={P} no masks"))
    assert worst <= GRID_BOUND


def test_grid_takes_the_first_view_as_reference_and_scores_it_one():
    from hrnet_hip import registration as G
    _, _, _, views, view_masks = case(1, 3, 33, 47)
    d = _cuda(views, view_masks)
    got = G.mncc_grid(*d, points_per_dim=3, width=1.0)
    assert torch.equal(got, G.mncc_grid(*d, ref=d[0][:, 0], ref_mask=d[1][:, 0], points_per_dim=3, width=1.0))
    assert abs(float(got[0, 0, 1, 1]) - 1.0) <= GRID_BOUND and float(got[0, 0].max()) == float(got[0, 0, 1, 1])
    far = torch.full((1, 3, 2), 300.0, device="cuda")            # no footprint left inside the frame
    assert torch.all(torch.isneginf(G.mncc_grid(*d, centres=far, points_per_dim=3, width=1.0)))


# ----------------------------------------------------------------------------- the search, level by level along the device's own path
@pytest.mark.parametrize("radius", [1.0, 2.0])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_search_follows_the_fp64_scores_level_by_level(shape, radius):
    from hrnet_hip import registration as G
    B, V, H, W = shape
    P, levels = 7, 5
    _, ref, ref_mask, views, view_masks = (a.copy() for a in case(*shape))
    views[0, V - 1] = 0.0                                        # a padded view: shift (0, 0), score -inf
    shifts, trace = G.mncc_search(*_cuda(views, view_masks, ref, ref_mask), points_per_dim=P, levels=levels, radius=radius, return_trace=True)
    shifts, trace = shifts.cpu().numpy(), trace.cpu().numpy()
    assert shifts.shape == (B, V, 2) and trace.shape == (B, V, levels, 3)
    assert np.array_equal(shifts, trace[:, :, -1, :2])
    assert np.all(shifts[0, V - 1] == 0.0) and np.all(trace[0, V - 1, :, :2] == 0.0) and np.all(np.isneginf(trace[0, V - 1, :, 2]))
    widths = R.level_widths(P, levels, radius)
    worst_score, worst_gap = 0.0, 0.0
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
    print(f"search {shape} radius {radius}: max |trace score - fp64 at the chosen point| = {worst_score:.3e}, "
          f"max (fp64 maximum - fp64 at the chosen point) = {worst_gap:.3e}")
    assert worst_score <= GRID_BOUND and worst_gap <= 2 * GRID_BOUND


# ----------------------------------------------------------------------------- known shifts
@pytest.mark.parametrize("shape", [(1, 4, 16, 16), (1, 4, 24, 40), (1, 4, 33, 47), (1, 4, 64, 64), (1, 4, 128, 128)],
                         ids=["16x16", "24x40", "33x47", "64x64", "128x128"])
def test_search_recovers_known_shifts(shape):
    from hrnet_hip import registration as G
    true, ref, ref_mask, views, view_masks = case(*shape)
    got = G.mncc_search(*_cuda(views, view_masks, ref, ref_mask), points_per_dim=7, levels=5, radius=1.0).cpu().numpy()
    err = np.abs(got - true)
    print(f"recovery {shape}: worst component error {err.max():.4f} px")
    assert err.max() <= RECOVERY_PX


def test_register_views_brings_the_views_onto_the_first():
    """The default reference is view 0; the registered views then agree with it where all are valid."""
    from hrnet_hip import registration as G
    true, ref, ref_mask, views, view_masks = case(1, 4, 64, 64)
    lrs, masks = np.concatenate([ref[:, None], views], 1), np.concatenate([ref_mask[:, None], view_masks], 1)
    registered, valid, shifts = G.register_views(*_cuda(lrs, masks), levels=5)
    assert torch.all(shifts[0, 0] == 0.0) and np.abs(shifts[0, 1:].cpu().numpy() - true[0]).max() <= RECOVERY_PX
    both = (valid[0, 1:] * valid[0, :1]).bool()
    gain = torch.tensor(0.1 / 0.11, device="cuda")               # the generator's template is 0.32 + 0.11 z against 0.3 + 0.1 z
    resid = ((registered[0, 1:] - 0.32) * gain + 0.3 - registered[0, :1])[both]
    raw = ((torch.from_numpy(views[0]).cuda() - 0.32) * gain + 0.3 - registered[0, :1])[both]
    # what is left is the generator's noise, 0.002 N(0, 1) times the gain: a mean magnitude of 0.0015; twice that allows for the sampler
    print(f"mean |registered - reference| {float(resid.abs().mean()):.5f}, unregistered {float(raw.abs().mean()):.5f}")
    assert float(resid.abs().mean()) < 0.003 and float(resid.abs().mean()) < float(raw.abs().mean())


# ----------------------------------------------------------------------------- reproducibility
def test_search_is_bit_reproducible_and_its_first_level_is_the_grid():
    from hrnet_hip import registration as G
    shape = (2, 3, 33, 47)
    _, ref, ref_mask, views, view_masks = case(*shape)
    d = _cuda(views, view_masks, ref, ref_mask)
    for radius in (1.0, 1.5):
        runs = [G.mncc_search(*d, points_per_dim=7, levels=4, radius=radius, return_trace=True) for _ in range(2)]
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
        scores = G.mncc_grid(*d, points_per_dim=7, width=2.0 * radius)
        assert torch.equal(scores, G.mncc_grid(*d, points_per_dim=7, width=2.0 * radius))
        scores, trace = scores.cpu().numpy(), runs[0][1].cpu().numpy()
        coords = R.grid_coords(0.0, 2.0 * radius, 7)
        for b in range(shape[0]):
            for v in range(shape[1]):
                at, best = R.best_of(scores[b, v], coords, coords, (0.0, 0.0))
                assert (trace[b, v, 0, 0], trace[b, v, 0, 1]) == at
                assert np.float32(best).tobytes() == trace[b, v, 0, 2].tobytes()


# ----------------------------------------------------------------------------- the resampled views
APPLY_SHIFTS = [(0.3, -0.7), (-1.25, 2.6), (0.0, 0.0), (1.0, -2.0), (3.7, 0.9), (200.0, 0.0)]


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_shift_views_matches_fp64_per_element(shape):
    from hrnet_hip import registration as G
    B, V, H, W = shape
    _, _, _, views, view_masks = case(*shape)
    shifts = np.array([[APPLY_SHIFTS[(3 * b + v) % len(APPLY_SHIFTS)] for v in range(V)] for b in range(B)], np.float32)
    worst, near = 0.0, 0
    for masks in (view_masks, None):
        out, valid = G.shift_views(*_cuda(views, masks, shifts))
        out, valid = out.cpu().numpy(), valid.cpu().numpy()
        for b in range(B):
            for v in range(V):
                m = np.ones((H, W)) if masks is None else masks[b, v]
                near += int((np.abs(R.mask_bilinear(m, shifts[b, v]) - 0.5) <= 1e-6).sum())
                want_valid = R.shifted_mask(m, shifts[b, v])
                assert np.array_equal(valid[b, v], want_valid.astype(np.float32))
                assert np.all(out[b, v][~want_valid] == 0.0)
                want = R.sample(views[b, v], shifts[b, v])
                worst = max(worst, float(np.abs(out[b, v] - want)[want_valid].max()) if want_valid.any() else 0.0)
    print(f"apply {shape}: max |device - fp64| = {worst:.3e}; {near} pixels with the fp64 bilinear mask within 1e-6 of 0.5")
    assert near == 0                                             # the shifts are chosen so: `valid` is compared everywhere
    assert worst <= APPLY_BOUND


def test_register_views_is_search_then_shift():
    from hrnet_hip import registration as G
    _, ref, ref_mask, views, view_masks = case(2, 3, 16, 16)
    d = _cuda(views, view_masks)
    kw = dict(ref=torch.from_numpy(ref).cuda(), ref_mask=torch.from_numpy(ref_mask).cuda(), points_per_dim=5, levels=3, radius=1.5)
    registered, valid, shifts = G.register_views(*d, **kw)
    assert torch.equal(shifts, G.mncc_search(*d, **kw))
    want = G.shift_views(*d, shifts)
    assert torch.equal(registered, want[0]) and torch.equal(valid, want[1])
    assert set(valid.unique().tolist()) == {0.0, 1.0}


# ----------------------------------------------------------------------------- the custom ops
def test_ops_are_the_binding_calls_and_pass_opcheck():
    from hrnet_hip import binding
    ops = torch.ops.hrnet_hip
    _, ref, ref_mask, views, view_masks = case(1, 2, 24, 40)
    views, view_masks, ref, ref_mask = _cuda(views, view_masks, ref, ref_mask)
    centres = torch.tensor([[[0.25, -0.5], [0.0, 0.0]]], device="cuda")
    assert torch.equal(ops.mncc_grid(ref, ref_mask, views, view_masks, centres, 5, 0.5),
                       binding.mncc_grid(ref, ref_mask, views, view_masks, centres, 5, 0.5))
    got, want = ops.mncc_search(ref, None, views, view_masks, 4, 3, 1.0), binding.mncc_search(ref, None, views, view_masks, 4, 3, 1.0)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    got, want = ops.shift_views(views, view_masks, centres), binding.mncc_apply(views, view_masks, centres)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    checks = ("test_schema", "test_faketensor")
    torch.library.opcheck(ops.mncc_grid.default, (ref, ref_mask, views, view_masks, centres, 5, 0.5), test_utils=checks)
    torch.library.opcheck(ops.mncc_grid.default, (ref, None, views, None, centres, 3, 2.0), test_utils=checks)
    torch.library.opcheck(ops.mncc_search.default, (ref, ref_mask, views, view_masks, 4, 3, 1.0), test_utils=checks)
    torch.library.opcheck(ops.shift_views.default, (views, view_masks, centres), test_utils=checks)
    torch.library.opcheck(ops.shift_views.default, (views, None, centres), test_utils=checks)


# ----------------------------------------------------------------------------- the paths it must not touch
def test_hrnet_forward_does_not_change_around_a_registration():
    from DeepNetworks.HRNet import HRNet
    from hrnet_hip import registration as G
    from oracle import synth, weights
    net = HRNet(weights.HRNET_CONFIG)
    net.load_state_dict(weights.to_torch_state(weights.hrnet_state(1234)))
    net = net.cuda().eval()
    lrs, alphas, _ = synth.make_batch(3, 2, 5, 32, [5, 3])
    lrs, alphas = torch.from_numpy(lrs).cuda(), torch.from_numpy(alphas).cuda()
    with torch.no_grad():
        before = net(lrs, alphas).clone()
        registered, valid, shifts = G.register_views(lrs, levels=3)
        assert registered.shape == lrs.shape and torch.all(shifts[:, 0] == 0.0)
        G.mncc_grid(lrs, points_per_dim=9, width=8.0)
        after = net(lrs, alphas)
    assert torch.equal(before, after)
