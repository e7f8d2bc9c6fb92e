"""GPU: the masked-NCC scores of every registration path where the pixels a score is taken over do not have the frame's mean
(tests/registration_cases.py: a level step across the frame, a mask that hides one side of it in one image only, a contrast of a
hundredth against levels of 0.2 and 0.5 .. 0.8) - the resident kernels (mncc_grid, mncc_search), the tiled ones (mncc_grid_scene,
mncc_search_scene), the shift field (mncc_search_local) and the pyramid (mncc_search_pyramid) - per element against the fp64
restatements (tests/registration_ref.py, registration_local_ref.py, registration_pyramid_ref.py).  Every other registration test draws
its frames from registration_ref.scene, where any set of common pixels has the frame's mean and a contrast of 0.1: there the sums of
images centred on frame means lose nothing in fp32, and these tests are where they would.

The bounds are the project's, unchanged: 4e-7 of a device score against fp64, 8e-7 between two device paths (DESIGN.md sections 7f,
7g).  tests/test_registration_pin_host.py shows on the CPU that each case here is admitted - fp32 resampling alone costs it at most 1e-7 at
every point of the grids compared here and of every level a search walks here, along the path the fp64 restatement takes (a device
search that takes another point where two fp64 scores of a level lie within the bound walks grids shifted by less than a spacing) -
and that per-thread fp32 sums would break the bound on every case but the controls.  tests/kernel_bounds.py records what was measured.

On every case: a finite score lies within the bound of [-1, 1], -inf entries are fp64's, two runs agree bit for bit, and a view
computed alone gives what it gives in its batch."""
import functools

import numpy as np
import pytest
import torch

import registration_cases as C
import registration_local_ref as L
import registration_ref as R

pytestmark = pytest.mark.gpu

WORST = {f: (0.0, "") for f in C.FAMILIES}


def _cuda(*arrays):
    return tuple(None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays)


def _note(fam, value, what):
    if value >= WORST[fam][0]:
        WORST[fam] = (value, what)
    print(f"pin {what}: {value:.3e}; worst of {fam} so far {WORST[fam][0]:.3e} ({WORST[fam][1]})")


def _same(a, b):
    a, b = (a, b) if isinstance(a, (tuple, list)) else ((a,), (b,))
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _twice_and_alone(fn, d, extra=()):
    """fn(views, view_masks, ref, ref_mask, *extra) -> a tensor or a tuple of tensors with the views along dim 1; every `extra` is
    per view along dim 1.  Two runs agree bit for bit, and so does every view computed alone with its place in the batch.  -> the result"""
    views, vm, ref, rm = d
    first, again = fn(views, vm, ref, rm, *extra), fn(views, vm, ref, rm, *extra)
    assert _same(first, again), "two runs differ"
    for v in range(views.shape[1]):
        one = fn(views[:, v:v + 1], None if vm is None else vm[:, v:v + 1], ref, rm, *(e[:, v:v + 1] for e in extra))
        want = tuple(t[:, v:v + 1] for t in first) if isinstance(first, (tuple, list)) else first[:, v:v + 1]
        assert _same(one, want), f"view {v} alone differs from its place in the batch"
    return first


def device(case, sub):
    ref, rm, views, vm = C.inputs(case, sub)
    return _cuda(views, vm, ref, rm)


# ----------------------------------------------------------------------------- the resident kernels
def _grid(case, sub, fn, what):
    V = case[2][1]
    worst = 0.0
    for rotation, (P, width) in enumerate(C.GRIDS):
        centres = C.centres(V, rotation)
        got = _twice_and_alone(lambda v, vm, r, rm, c: fn(v, vm, r, rm, centres=c, points_per_dim=P, width=width), device(case, sub),
                               _cuda(centres))
        assert got.shape == (1, V, P, P)
        worst = max(worst, C.worst(got.cpu().numpy(), C.grid_ref(case, sub, centres, width, P), f"{what} {case[0]} {sub} P={P} width={width}"))
    return worst


@pytest.mark.parametrize("case", C.family("resident"), ids=C.ids(C.family("resident")))
def test_resident_grid_matches_fp64_per_element(case):
    from hrnet_hip import registration as G
    worst = max(_grid(case, sub, G.mncc_grid, "grid") for sub in C.SUBS)
    _note("resident", worst, f"grid {case[0]}")
    assert worst <= C.SCORE_BOUND


def _search(case, sub, fn):
    V = case[2][1]
    P, levels, radius = C.SEARCH
    shifts, trace = _twice_and_alone(lambda v, vm, r, rm: fn(v, vm, r, rm, points_per_dim=P, levels=levels, radius=radius, return_trace=True),
                                     device(case, sub))
    shifts, trace = shifts.cpu().numpy(), trace.cpu().numpy()
    assert shifts.shape == (1, V, 2) and trace.shape == (1, V, levels, 3) and np.array_equal(shifts, trace[:, :, -1, :2])
    return C.follow(case, sub, trace, P, levels, radius)


@pytest.mark.parametrize("case", C.family("resident"), ids=C.ids(C.family("resident")))
def test_resident_search_follows_the_fp64_scores_level_by_level(case):
    from hrnet_hip import registration as G
    score, gap = (max(x) for x in zip(*(_search(case, sub, G.mncc_search) for sub in C.SUBS)))
    _note("resident", score, f"search {case[0]}")
    print(f"pin search {case[0]}: max (fp64 maximum - fp64 at the chosen point) = {gap:.3e}")
    assert score <= C.SCORE_BOUND and gap <= 2 * C.SCORE_BOUND


# ----------------------------------------------------------------------------- the tiled kernels
@pytest.mark.parametrize("sub", C.SUBS)
@pytest.mark.parametrize("case", C.family("scene"), ids=C.ids(C.family("scene")))
def test_scene_grid_matches_fp64_per_element(case, sub):
    from hrnet_hip import registration as G
    worst = _grid(case, sub, G.mncc_grid_scene, "grid_scene")
    _note("scene", worst, f"grid_scene {case[0]} {sub}")
    assert worst <= C.SCORE_BOUND
    if max(case[2][2:]) <= 128:                                  # where both run: the tiled path against the resident one
        between = 0.0
        for rotation, (P, width) in enumerate(C.GRIDS):
            d = device(case, sub) + _cuda(C.centres(case[2][1], rotation))
            a, b = G.mncc_grid_scene(*d, points_per_dim=P, width=width), G.mncc_grid(*d, points_per_dim=P, width=width)
            assert torch.equal(torch.isneginf(a), torch.isneginf(b))
            fin = ~torch.isneginf(b)
            between = max(between, float((a[fin].double() - b[fin].double()).abs().max()) if fin.any() else 0.0)
        print(f"pin scene against resident {case[0]} {sub}: max |grid_scene - grid| = {between:.3e}")
        assert between <= C.DEVICE_BOUND


@pytest.mark.parametrize("sub", C.SUBS)
@pytest.mark.parametrize("case", C.family("scene"), ids=C.ids(C.family("scene")))
def test_scene_search_follows_the_fp64_scores_level_by_level(case, sub):
    from hrnet_hip import registration as G
    score, gap = _search(case, sub, G.mncc_search_scene)
    _note("scene", score, f"search_scene {case[0]} {sub}")
    print(f"pin search_scene {case[0]} {sub}: max (fp64 maximum - fp64 at the chosen point) = {gap:.3e}")
    assert score <= C.SCORE_BOUND and gap <= 2 * C.SCORE_BOUND


# ----------------------------------------------------------------------------- the shift field
(LOCAL_P, LOCAL_LEVELS, LOCAL_RADIUS), MIN_VALID = C.LOCAL, 0.25        # tests/test_gpu_registration_local.py's searched()


@functools.lru_cache(maxsize=None)
def local_searched(cid, sub):
    """the device's own path, as tests/test_gpu_registration_local.py takes it: the global shifts (P = 7, five levels of radius 1), then
    four local levels at P = 6 from them -> (init, field, trace, ok) as numpy"""
    from hrnet_hip import registration as G
    case = next(c for c in C.CASES if c[0] == cid)
    block = C.BLOCK[case[2][2:]]
    d = device(case, sub)
    init = _twice_and_alone(lambda v, vm, r, rm: G.mncc_search_scene(v, vm, r, rm, points_per_dim=C.LOCAL_INIT[0], levels=C.LOCAL_INIT[1],
                                                                         radius=C.LOCAL_INIT[2]), d)
    local = lambda v, vm, r, rm, i: G.mncc_search_local(v, vm, r, rm, block=block, init=i, points_per_dim=LOCAL_P, levels=LOCAL_LEVELS,
                                                        radius=LOCAL_RADIUS, min_valid=MIN_VALID, return_trace=True)
    field, trace, ok = _twice_and_alone(local, d, (init,))
    return tuple(t.cpu().numpy() for t in (init, field, trace, ok))


@pytest.mark.parametrize("sub", C.SUBS)
@pytest.mark.parametrize("case", C.family("local"), ids=C.ids(C.family("local")))
def test_local_trace_scores_match_fp64_at_the_chosen_points(case, sub):
    """every block's every level against registration_local_ref.block_score, and `ok` by the existing test's rule"""
    _, _, (B, V, H, W), *_ = case
    block = C.BLOCK[(H, W)]
    ref, rm, views, vm = C.inputs(case, sub)
    init, field, trace, ok = local_searched(case[0], sub)
    assert trace.shape == (1, V, L.blocks(H, block), L.blocks(W, block), LOCAL_LEVELS, 3)
    C.in_range(trace[..., 2], case[0])
    worst = 0.0
    for v in range(V):
        view_mask = None if vm is None else vm[0, v]
        for i, rows in enumerate(L.bounds(H, block)):
            for j, cols in enumerate(L.bounds(W, block)):
                for k in range(LOCAL_LEVELS):
                    dy, dx, got = trace[0, v, i, j, k]
                    want = L.block_score(ref[0], rm[0], views[0, v], view_mask, (dy, dx), rows, cols)
                    assert np.isneginf(got) == np.isneginf(want), (case[0], sub, v, i, j, k)
                    if np.isfinite(want):
                        worst = max(worst, abs(float(got) - want))
                n = L.common_valid(rm[0], view_mask, (H, W), trace[0, v, i, j, -1, :2], rows, cols)
                area = (rows[1] - rows[0]) * (cols[1] - cols[0])
                assert abs(n - MIN_VALID * area) > 0.0025 * area, "a block within 1 % of the threshold"
                assert bool(ok[0, v, i, j]) == (np.isfinite(trace[0, v, i, j, -1, 2]) and n >= MIN_VALID * area)
                assert np.array_equal(field[0, v, i, j], trace[0, v, i, j, -1, :2] if ok[0, v, i, j] else init[0, v])
    _note("local", worst, f"local trace {case[0]} {sub}")
    assert worst <= C.SCORE_BOUND


@pytest.mark.parametrize("sub", C.SUBS)
@pytest.mark.parametrize("case", C.family("local"), ids=C.ids(C.family("local")))
def test_local_levels_are_the_grid_of_the_restricted_reference(case, sub):
    """tests/test_gpu_registration_local.py's comparison of two device paths on these frames: mncc_grid_scene with the reference mask
    restricted to the block centres the reference on the block's mean, the local search on the frame's"""
    from hrnet_hip import registration as G
    _, _, (B, V, H, W), *_ = case
    block = C.BLOCK[(H, W)]
    ref, rm, views, vm = C.inputs(case, sub)
    init, field, trace, ok = local_searched(case[0], sub)
    d_views, d_masks, d_ref = _cuda(views, vm, ref)
    worst_at, worst_gap = 0.0, 0.0
    for i, rows in enumerate(L.bounds(H, block)):
        for j, cols in enumerate(L.bounds(W, block)):
            restricted = torch.from_numpy(L.restricted(rm[0], (H, W), rows, cols)[None]).cuda()
            centres = init.copy()
            for k, width in enumerate(R.level_widths(LOCAL_P, LOCAL_LEVELS, LOCAL_RADIUS)):
                assert float(np.float32(width)) == width
                scores = G.mncc_grid_scene(d_views, d_masks, d_ref, restricted, centres=torch.from_numpy(centres).cuda(), points_per_dim=LOCAL_P,
                                           width=width).cpu().numpy()
                for v in range(V):
                    dy, dx, got = trace[0, v, i, j, k]
                    if not np.isfinite(scores[0, v]).any():
                        assert (dy, dx) == tuple(centres[0, v]) and np.isneginf(got)
                        continue
                    dys, dxs = R.grid_coords(centres[0, v, 0], width, LOCAL_P), R.grid_coords(centres[0, v, 1], width, LOCAL_P)
                    ii, jj = np.flatnonzero(dys == dy), np.flatnonzero(dxs == dx)
                    assert len(ii) and len(jj), f"view {v} block {i},{j} level {k}: ({dy}, {dx}) is no point of {dys} x {dxs}"
                    at = float(scores[0, v, ii[0], jj[0]])
                    assert np.isfinite(got) and np.isfinite(at)
                    worst_at, worst_gap = max(worst_at, abs(float(got) - at)), max(worst_gap, float(scores[0, v].max()) - float(got))
                centres = np.ascontiguousarray(trace[:, :, i, j, k, :2])
    print(f"pin local levels {case[0]} {sub}: max |trace score - grid_scene at the point| = {worst_at:.3e}, max (grid_scene maximum - trace "
          f"score) = {worst_gap:.3e}")
    assert worst_at <= C.DEVICE_BOUND and worst_gap <= C.DEVICE_BOUND


# ----------------------------------------------------------------------------- the pyramid
@pytest.mark.parametrize("sub", C.SUBS)
@pytest.mark.parametrize("case", C.family("pyramid"), ids=C.ids(C.family("pyramid")))
def test_pyramid_is_its_parts_and_every_octave_matches_fp64(case, sub):
    """tests/test_gpu_registration_pyramid.py's composition (reduce2, mncc_search_scene(init=...), twice the shift) bit for bit, and one
    fp64 score per view and octave on the planes the device reduced"""
    from hrnet_hip import registration as G
    K, P, levels, radius, coarse_levels, refine_radius = (C.PYRAMID[k] for k in ("octaves", "P", "levels", "radius", "coarse_levels",
                                                                                  "refine_radius"))
    V = case[2][1]
    d = device(case, sub)
    shifts, trace = _twice_and_alone(lambda v, vm, r, rm: G.mncc_search_pyramid(v, vm, r, rm, octaves=K, points_per_dim=P, levels=levels,
                                                                                radius=radius, coarse_levels=coarse_levels,
                                                                                refine_radius=refine_radius, return_trace=True), d)
    assert trace.shape == (1, V, K + 1, 3)
    octs = [d]
    for _ in range(K):
        v, vm, r, rm = octs[-1]
        octs.append(G.reduce2(v, vm) + G.reduce2(r, rm))
    s, rows = None, []
    for k in range(K, -1, -1):
        v, vm, r, rm = octs[k]
        s, t = G.mncc_search_scene(v, vm, r, rm, points_per_dim=P, levels=levels if k == 0 else coarse_levels,
                                   radius=radius if k == K else refine_radius, return_trace=True, init=None if k == K else s * 2)
        rows.append(t[:, :, -1])
    assert torch.equal(shifts, s) and torch.equal(trace, torch.stack(rows, dim=2)) and torch.equal(trace[:, :, K, :2], shifts)
    trace = trace.cpu().numpy()
    C.in_range(trace[..., 2], case[0])
    worst = 0.0
    for j in range(K + 1):
        v, vm, r, rm = (None if t is None else t.cpu().numpy() for t in octs[K - j])
        for i in range(V):
            dy, dx, got = trace[0, i, j]
            want = R.score(r[0], None if rm is None else rm[0], v[0, i], None if vm is None else vm[0, i], (dy, dx))
            assert np.isneginf(got) == np.isneginf(want), (case[0], sub, i, j)
            if np.isfinite(want):
                worst = max(worst, abs(float(got) - want))
    _note("pyramid", worst, f"pyramid trace {case[0]} {sub}")
    assert worst <= C.SCORE_BOUND
