"""GPU: the coarse-to-fine registration search (hrnet_hip.registration's reduce2 / mncc_search_scene(init=...) / mncc_search_pyramid /
register_scene_pyramid over hrn_mncc_reduce2 / hrn_mncc_search_scene_from / hrn_mncc_search_pyramid): reduce2 per
element against the fp64 restatement (tests/registration_pyramid_ref.py) inside guarded buffers at every alignment of a row; the search
from a centre against the existing device paths, bit for bit; the pyramid against the composition of its parts, bit for bit, and its
trace against fp64; recovery of shifts of up to 13 px that the plain search misses; bit-reproducibility, the independence of a view
from its batch, and the custom ops.

reduce2's shapes: (1, 2, 32, 32) is the smallest plane; (1, 2, 33, 47) has odd sides; (2, 3, 70, 96) a batch, 35 rows of output over three
tile rows of 16; (1, 2, 130, 150) an output of 65 x 75 that crosses the 16 x 64 tile in both directions by one row and eleven columns;
(1, 1, 129, 260) three tile columns and an odd height.  Each plane is given to the kernel 0, 1, 2 and 3 floats off a 16-byte boundary, so
that every row takes the 16-byte path, the head path and - with a mask at another offset - both at once.

The bounds: REDUCE2_BOUND is 4 x the largest |device - fp64| measured over all of these, rounded up to one digit (the issue's rule,
capped at 1e-6); scores carry sections 7f / 7g's 4e-7 against fp64; a recovered shift is bounded by 1.5 x the restatement's own worst
error on the same scenes (tests/test_registration_pyramid_host.py), capped at the project's 0.02 px."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import registration_pyramid_ref as Y
import registration_ref as R

pytestmark = pytest.mark.gpu

SCORE_BOUND = 4e-7           # DESIGN.md sections 7f / 7g: a device score against fp64
REDUCE2_BOUND = Y.REDUCE2_BOUND
SHIFT_BOUND_PX = 0.02        # the project's bound on a recovered shift
# tests/test_registration_pyramid_host.py: the restatement's worst error over seeds 1..3, four views each
RESTATEMENT_WORST_PX = {(64, 80): 0.00540, (96, 144): 0.00406}
PLAIN_REACH_PX = 4.0 * sum(0.25 ** k for k in range(6))      # the same file: how far six levels of radius 4 get at P = 7: 5.332 px

REDUCE_SHAPES = [(1, 2, 32, 32), (1, 2, 33, 47), (2, 3, 70, 96), (1, 2, 130, 150), (1, 1, 129, 260)]
GUARD = 1024                 # floats in front of and behind every device buffer of the reduce2 test
SENT = 0x7F7F7F7F            # the bit pattern of an untouched output word


def _cuda(*arrays):
    return tuple(None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays)


def ids(shapes):
    return ["x".join(map(str, s)) for s in shapes]


# ----------------------------------------------------------------------------- reduce2 per element
@functools.lru_cache(maxsize=None)
def reduce_case(shape):
    """-> (x (N,H,W) f32 in [0, 1), mask (N,H,W) f32 0 / 1 with holes and masked borders) for the planes of `shape`"""
    B, V, H, W = shape
    rng = np.random.default_rng(H * 1000 + W)
    x = rng.random((B * V, H, W), dtype=np.float32)
    mask = (rng.random((B * V, H, W)) > 0.35).astype(np.float32)
    mask[:, :3, : W // 2] = 0.0
    mask[:, H // 2:, -2:] = 0.0
    return x, mask


@functools.lru_cache(maxsize=None)
def reduce_want(shape, masks):
    x, mask = reduce_case(shape)
    parts = [Y.reduce2(x[n], mask[n] if masks else None) for n in range(x.shape[0])]
    return np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts])


def guarded(values, offset, fill):
    """values (numpy f32) in a device buffer `offset` floats off its 256-byte aligned start plus GUARD, `fill` around: -> (buffer, payload)"""
    n = values.size
    buf = torch.full((2 * GUARD + n + 4,), fill, dtype=torch.float32, device="cuda")
    payload = buf[GUARD + offset:GUARD + offset + n]
    payload.copy_(torch.from_numpy(values.reshape(-1)))
    return buf, payload


def sentinel_out(n, offset):
    buf = torch.full((2 * GUARD + n + 4,), SENT, dtype=torch.int32, device="cuda")
    return buf, buf[GUARD + offset:GUARD + offset + n]


@pytest.mark.parametrize("masks", [True, False])
@pytest.mark.parametrize("shape", REDUCE_SHAPES, ids=ids(REDUCE_SHAPES))
def test_reduce2_matches_fp64_per_element(shape, masks):
    from hrnet_hip import binding
    lib = binding.load_library()
    x, mask = reduce_case(shape)
    N, H, W = x.shape
    Ho, Wo = H // 2, W // 2
    want, want_clear = reduce_want(shape, masks)
    assert want_clear.any() and (not masks or not want_clear.all())
    worst = 0.0
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    for off in range(4):
        xb, xp = guarded(x, off, float("nan"))
        mb, mp = guarded(mask, (off + 2 * (off & 1) + 1) % 4 if off else 0, float("nan")) if masks else (None, None)
        runs = []
        for _ in range(2):
            ob, op = sentinel_out(N * Ho * Wo, (off * 3) % 4)
            omb, omp = sentinel_out(N * Ho * Wo, off)
            rc = lib.hrn_mncc_reduce2(ptr(xp), ptr(mp) if masks else ctypes.c_void_p(0), N, H, W, ptr(op), ptr(omp), ctypes.c_void_p(0))
            assert rc == 0, lib.hrn_last_error()
            torch.cuda.synchronize()
            for buf, pay in ((ob, op), (omb, omp)):
                lo = pay.data_ptr() - buf.data_ptr() >> 2
                assert bool((buf[:lo] == SENT).all()) and bool((buf[lo + pay.numel():] == SENT).all()), "a word outside the output was written"
            runs.append((op.clone(), omp.clone()))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), "two runs differ"
        got = runs[0][0].view(torch.float32).cpu().numpy().reshape(N, Ho, Wo)
        got_clear = runs[0][1].view(torch.float32).cpu().numpy().reshape(N, Ho, Wo)
        assert np.array_equal(got_clear, want_clear.astype(np.float32)), f"offset {off}: the coarse mask differs from the restatement"
        assert np.all(got[~want_clear] == 0.0) and np.isfinite(got).all()
        worst = max(worst, float(np.abs(got.astype(np.float64) - want).max()))
        assert torch.equal(xp.cpu(), torch.from_numpy(x.reshape(-1))), "the input was written"
    print(f"reduce2 {shape} masks={masks}: max |device - fp64| = {worst:.3e} over four alignments; {int(want_clear.sum())} of "
          f"{want_clear.size} coarse pixels clear")
    assert worst <= REDUCE2_BOUND


def test_reduce2_python_forms_agree():
    from hrnet_hip import registration as G
    x, mask = reduce_case((2, 3, 70, 96))
    dx, dm = _cuda(x.reshape(2, 3, 70, 96), mask.reshape(2, 3, 70, 96))
    out, om = G.reduce2(dx, dm)
    assert out.shape == om.shape == (2, 3, 35, 48)
    want, clear = reduce_want((2, 3, 70, 96), True)
    assert np.array_equal(om.cpu().numpy().reshape(6, 35, 48), clear.astype(np.float32))
    out3, om3 = G.reduce2(dx[:, 1], dm[:, 1])                  # (B,H,W), a strided view
    assert torch.equal(out3, out[:, 1]) and torch.equal(om3, om[:, 1])
    none, nm = G.reduce2(dx)
    assert bool((nm == 1).all()) and np.abs(none.cpu().numpy().reshape(6, 35, 48) - reduce_want((2, 3, 70, 96), False)[0]).max() <= REDUCE2_BOUND


# ----------------------------------------------------------------------------- scenes with large shifts
@functools.lru_cache(maxsize=None)
def far_scene(H, W, limit, seeds=(1, 2, 3), V=4):
    """One seeded scene per sample, the host test's own: -> (ref (B,H,W), ref_mask, views (B,V,H,W), view_masks, true (B,V,2))"""
    true = [R.random_shifts(V, limit, seed=s) for s in seeds]
    parts = [Y.scene(H, W, t, s) for t, s in zip(true, seeds)]
    return tuple(np.stack([p[i] for p in parts]) for i in range(4)) + (np.stack(true),)


# ----------------------------------------------------------------------------- the search from a centre
def test_init_none_is_the_existing_op_bit_for_bit():
    from hrnet_hip import registration as G
    ref, ref_mask, views, view_masks, _ = far_scene(96, 144, 13.0)
    d = _cuda(ref, ref_mask, views, view_masks)
    want = torch.ops.hrnet_hip.mncc_search_scene(d[0], d[1], d[2], d[3], 7, 4, 2.0)
    got = G.mncc_search_scene(d[2], d[3], d[0], d[1], points_per_dim=7, levels=4, radius=2.0, return_trace=True, init=None)
    frm = torch.ops.hrnet_hip.mncc_search_scene_from(d[0], d[1], d[2], d[3], None, 7, 4, 2.0)
    zero = G.mncc_search_scene(d[2], d[3], d[0], d[1], points_per_dim=7, levels=4, radius=2.0, return_trace=True,
                               init=torch.zeros(3, 4, 2, device="cuda"))
    for other in (got, frm, zero):
        assert torch.equal(want[0], other[0]) and torch.equal(want[1], other[1])


@pytest.mark.parametrize("masks", [True, False])
def test_every_level_from_a_centre_is_the_grid_at_the_previous_centre(masks):
    """P = 6 and radius 2: the widths 4, 1, 1/4, 1/16 are fp32 values that mncc_grid_scene can be given."""
    from hrnet_hip import registration as G
    ref, ref_mask, views, view_masks, true = far_scene(96, 144, 13.0)
    ref, ref_mask, views, view_masks = _cuda(ref, ref_mask if masks else None, views, view_masks if masks else None)
    init = torch.from_numpy((np.round(true) + np.array([0.4, -0.7])).astype(np.float32)).cuda()
    P, levels = 6, 4
    shifts, trace = G.mncc_search_scene(views, view_masks, ref, ref_mask, points_per_dim=P, levels=levels, radius=2.0, return_trace=True, init=init)
    assert float((shifts - torch.from_numpy(true).cuda()).abs().max()) < 0.1, "the search from a nearby centre finds the view"
    centres = init
    for k, width in enumerate(R.level_widths(P, levels, 2.0)):
        assert float(np.float32(width)) == width
        scores = G.mncc_grid_scene(views, view_masks, ref, ref_mask, centres=centres, points_per_dim=P, width=width)
        flat = scores.reshape(3, 4, P * P)
        assert bool(torch.isfinite(flat).all())
        best = flat.max(dim=2).values
        first = np.argmax(flat.cpu().numpy(), axis=2)        # the first maximum in row-major order
        assert torch.equal(best, trace[:, :, k, 2]), f"level {k}: the trace's score is not the grid's maximum"
        c = centres.cpu().numpy()
        for b in range(3):
            for v in range(4):
                dys, dxs = R.grid_coords(c[b, v, 0], width, P), R.grid_coords(c[b, v, 1], width, P)
                i, j = divmod(int(first[b, v]), P)
                assert (dys[i], dxs[j]) == tuple(trace[b, v, k, :2].tolist()), (b, v, k)
        centres = trace[:, :, k, :2].contiguous()
    assert torch.equal(shifts, centres)


@pytest.mark.parametrize("masks", [True, False])
def test_one_block_local_search_from_the_same_centre_agrees_bit_for_bit(masks):
    from hrnet_hip import registration as G
    ref, ref_mask, views, view_masks, true = far_scene(96, 144, 13.0)
    ref, ref_mask, views, view_masks = _cuda(ref, ref_mask if masks else None, views, view_masks if masks else None)
    init = torch.from_numpy((np.round(true) + np.array([-0.3, 0.6])).astype(np.float32)).cuda()
    for P, levels, radius in ((7, 5, 1.0), (4, 3, 2.0)):
        shifts, trace = G.mncc_search_scene(views, view_masks, ref, ref_mask, points_per_dim=P, levels=levels, radius=radius, return_trace=True,
                                            init=init)
        field, ltrace, ok = G.mncc_search_local(views, view_masks, ref, ref_mask, block=4096, init=init, points_per_dim=P, levels=levels,
                                                radius=radius, min_valid=0.0, return_trace=True)
        assert torch.equal(field[:, :, 0, 0], shifts) and torch.equal(ltrace[:, :, 0, 0], trace) and bool((ok == 1).all())


# ----------------------------------------------------------------------------- the pyramid and its parts
PYRAMIDS = [((64, 80), 1, 7.0), ((96, 144), 2, 13.0)]


@functools.lru_cache(maxsize=None)
def searched(shape, K, limit, masks):
    """The device's pyramid search of a scene with the defaults: -> (shifts (B,V,2), trace (B,V,K+1,3)) as device tensors"""
    from hrnet_hip import registration as G
    ref, ref_mask, views, view_masks, _ = far_scene(shape[0], shape[1], limit)
    ref, ref_mask, views, view_masks = _cuda(ref, ref_mask if masks else None, views, view_masks if masks else None)
    return G.mncc_search_pyramid(views, view_masks, ref, ref_mask, octaves=K, return_trace=True)


def composed(shape, K, limit, masks, **kw):
    """The same by the parts: reduce2, mncc_search_scene(init=...), * 2.  -> (shifts, trace (B,V,K+1,3), the octaves [(ref, ref_mask, views,
    view_masks)])"""
    from hrnet_hip import registration as G
    P, levels, radius = kw.get("points_per_dim", 7), kw.get("levels", 6), kw.get("radius", 4.0)
    coarse_levels, refine_radius = kw.get("coarse_levels", 3), kw.get("refine_radius", 1.0)
    ref, ref_mask, views, view_masks, _ = far_scene(shape[0], shape[1], limit)
    octs = [_cuda(ref, ref_mask if masks else None, views, view_masks if masks else None)]
    for _ in range(K):
        r, rm, v, vm = octs[-1]
        octs.append(G.reduce2(r, rm) + G.reduce2(v, vm))
    shifts, rows = None, []
    for k in range(K, -1, -1):
        r, rm, v, vm = octs[k]
        shifts, trace = G.mncc_search_scene(v, vm, r, rm, points_per_dim=P, levels=levels if k == 0 else coarse_levels,
                                            radius=radius if k == K else refine_radius, return_trace=True, init=None if k == K else shifts * 2)
        rows.append(trace[:, :, -1])
    return shifts, torch.stack(rows, dim=2), octs


@pytest.mark.parametrize("masks", [True, False])
def test_pyramid_without_octaves_is_the_scene_search_bit_for_bit(masks):
    from hrnet_hip import registration as G
    ref, ref_mask, views, view_masks, _ = far_scene(64, 80, 7.0)
    ref, ref_mask, views, view_masks = _cuda(ref, ref_mask if masks else None, views, view_masks if masks else None)
    for P, levels, radius in ((7, 6, 4.0), (5, 3, 1.0)):
        want, wtrace = G.mncc_search_scene(views, view_masks, ref, ref_mask, points_per_dim=P, levels=levels, radius=radius, return_trace=True)
        got, trace = G.mncc_search_pyramid(views, view_masks, ref, ref_mask, octaves=0, points_per_dim=P, levels=levels, radius=radius,
                                           coarse_levels=2, refine_radius=0.5, return_trace=True)
        assert trace.shape == (3, 4, 1, 3)
        assert torch.equal(got, want) and torch.equal(trace[:, :, 0], wtrace[:, :, -1])


@pytest.mark.parametrize("masks", [True, False])
@pytest.mark.parametrize("shape,K,limit", PYRAMIDS, ids=ids([p[0] for p in PYRAMIDS]))
def test_pyramid_is_the_composition_of_its_parts_bit_for_bit(shape, K, limit, masks):
    shifts, trace = searched(shape, K, limit, masks)
    want, wtrace, _ = composed(shape, K, limit, masks)
    assert trace.shape == (3, 4, K + 1, 3)
    assert torch.equal(shifts, want) and torch.equal(trace, wtrace)
    assert torch.equal(trace[:, :, K, :2], shifts)


def test_pyramid_with_other_arguments_is_the_composition_too():
    from hrnet_hip import registration as G
    kw = dict(points_per_dim=5, levels=4, radius=2.5, coarse_levels=2, refine_radius=1.5)
    ref, ref_mask, views, view_masks, _ = far_scene(130, 203, 14.0, seeds=(2,), V=3)
    d = _cuda(ref, ref_mask, views, view_masks)
    shifts, trace = G.mncc_search_pyramid(d[2], d[3], d[0], d[1], octaves=3, return_trace=True, **kw)
    octs = [d]
    for _ in range(3):
        r, rm, v, vm = octs[-1]
        octs.append(G.reduce2(r, rm) + G.reduce2(v, vm))
    assert octs[3][2].shape == (1, 3, 16, 25)
    s, rows = None, []
    for k in (3, 2, 1, 0):
        r, rm, v, vm = octs[k]
        s, t = G.mncc_search_scene(v, vm, r, rm, points_per_dim=5, levels=4 if k == 0 else 2, radius=2.5 if k == 3 else 1.5, return_trace=True,
                                   init=None if k == 3 else s * 2)
        rows.append(t[:, :, -1])
    assert torch.equal(shifts, s) and torch.equal(trace, torch.stack(rows, dim=2))


@pytest.mark.parametrize("masks", [True, False])
@pytest.mark.parametrize("shape,K,limit", PYRAMIDS, ids=ids([p[0] for p in PYRAMIDS]))
def test_trace_scores_match_fp64_at_the_chosen_points(shape, K, limit, masks):
    """One fp64 score per view and octave, on the planes the device reduced (so that the figure is the score's, not reduce2's)."""
    shifts, trace = searched(shape, K, limit, masks)
    _, _, octs = composed(shape, K, limit, masks)
    trace = trace.cpu().numpy()
    worst = 0.0
    for j in range(K + 1):
        r, rm, v, vm = (None if t is None else t.cpu().numpy() for t in octs[K - j])
        for b in range(3):
            for i in range(4):
                dy, dx, got = trace[b, i, j]
                want = R.score(r[b], None if rm is None else rm[b], v[b, i], None if vm is None else vm[b, i], (dy, dx))
                assert np.isfinite(got) and np.isfinite(want)
                worst = max(worst, abs(float(got) - want))
    print(f"pyramid trace {shape} K={K} masks={masks}: max |trace score - fp64| = {worst:.3e}")
    assert worst <= SCORE_BOUND


def test_results_are_reproducible_and_a_view_does_not_depend_on_its_batch():
    from hrnet_hip import registration as G
    shape, K, limit = (96, 144), 2, 13.0
    ref, ref_mask, views, view_masks, _ = far_scene(shape[0], shape[1], limit)
    ref, ref_mask, views, view_masks = _cuda(ref, ref_mask, views, view_masks)
    first = searched(shape, K, limit, True)
    again = G.mncc_search_pyramid(views, view_masks, ref, ref_mask, octaves=K, return_trace=True)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    for b in range(3):
        for vs in ([0, 1, 2, 3], [2], [3, 1]):
            s, t = G.mncc_search_pyramid(views[b:b + 1, vs], view_masks[b:b + 1, vs], ref[b:b + 1], ref_mask[b:b + 1], octaves=K, return_trace=True)
            assert torch.equal(s[0], first[0][b, vs]) and torch.equal(t[0], first[1][b, vs]), (b, vs)


# ----------------------------------------------------------------------------- recovery
@pytest.mark.parametrize("shape,K,limit", PYRAMIDS, ids=ids([p[0] for p in PYRAMIDS]))
def test_pyramid_recovers_shifts_the_plain_search_misses(shape, K, limit):
    from hrnet_hip import registration as G
    ref, ref_mask, views, view_masks, true = far_scene(shape[0], shape[1], limit)
    shifts, _ = searched(shape, K, limit, True)
    err = np.abs(shifts.cpu().numpy() - true).max(axis=2)
    bound = min(1.5 * RESTATEMENT_WORST_PX[shape], SHIFT_BOUND_PX)
    d = _cuda(ref, ref_mask, views, view_masks)
    plain = G.mncc_search_scene(d[2], d[3], d[0], d[1], points_per_dim=7, levels=6, radius=4.0).cpu().numpy()
    size, plain_err = np.abs(true).max(axis=2), np.abs(plain - true).max(axis=2)
    beyond, lost = size > PLAIN_REACH_PX, size > PLAIN_REACH_PX + 1.0
    print(f"pyramid recovery {shape} K={K} +-{limit:g} px: worst error {err.max():.5f} px over {err.size} views (bound {bound:.5f}); the plain "
          f"search misses {int(beyond.sum())} of them by {plain_err[beyond].min():.3f} px at least, {int(lost.sum())} by more than a pixel")
    assert err.max() <= bound
    # the control: the plain search cannot leave its reach of 5.332 px, so it misses every view beyond it by the excess at least, and by
    # more than a pixel where a component of the true shift passes reach + 1
    assert beyond.sum() >= 3 and np.all(np.abs(plain) <= PLAIN_REACH_PX)
    assert np.all(plain_err[beyond] >= (size - PLAIN_REACH_PX)[beyond] - 1e-6) and np.all(plain_err[lost] > 1.0)


def test_register_scene_pyramid_resamples_by_the_shifts_it_returns():
    from hrnet_hip import registration as G
    ref, ref_mask, views, view_masks, true = far_scene(96, 144, 13.0)
    ref, ref_mask, views, view_masks = _cuda(ref, ref_mask, views, view_masks)
    registered, valid, shifts = G.register_scene_pyramid(views, view_masks, ref=ref, ref_mask=ref_mask, octaves=2)
    assert torch.equal(shifts, searched((96, 144), 2, 13.0, True)[0])
    want, want_valid = G.shift_scene(views, view_masks, shifts)
    assert torch.equal(registered, want) and torch.equal(valid, want_valid)
    # the registered views lie on the reference where both are valid: far closer than the unregistered ones
    on = (valid * ref_mask[:, None]) > 0
    scale = lambda a: (a - a[on].mean()) / a[on].std()
    refs = ref[:, None].expand_as(registered)
    assert float((scale(registered) - scale(refs))[on].abs().mean()) < 0.1 * float((scale(views) - scale(refs))[on].abs().mean())


def test_register_scene_local_starts_from_the_pyramid():
    from hrnet_hip import registration as G
    true = np.array([[10.0, -10.0], [-9.6, 10.3]])
    ref, ref_mask, views, view_masks = Y.scene(130, 203, true, seed=7)
    ref, ref_mask, views, view_masks = _cuda(ref[None], ref_mask[None], views[None], view_masks[None])
    registered, valid, field, shifts = G.register_scene_local(views, view_masks, block=64, octaves=2, ref=ref, ref_mask=ref_mask)
    assert field.shape == (1, 2, 2, 3, 2) and registered.shape == valid.shape == (1, 2, 130, 203)
    assert torch.equal(shifts, G.mncc_search_pyramid(views, view_masks, ref, ref_mask, octaves=2))
    assert np.abs(shifts.cpu().numpy()[0] - true).max() <= SHIFT_BOUND_PX
    # four local levels of radius 0.5 stay within the sum of their half widths of the global shift
    assert np.abs(field.cpu().numpy()[0] - true[:, None, None, :]).max() <= 0.5 * sum(0.25 ** k for k in range(4)) + SHIFT_BOUND_PX
    plain = G.register_scene_local(views, view_masks, block=64, ref=ref, ref_mask=ref_mask, radius=4.0)[3]
    assert np.abs(plain.cpu().numpy()[0] - true).max() > 1.0                                            # octaves=0 is the path of before


# ----------------------------------------------------------------------------- the custom ops
def test_ops_are_the_binding_calls_and_pass_opcheck():
    from hrnet_hip import binding
    ops = torch.ops.hrnet_hip
    ref, ref_mask, views, view_masks, true = far_scene(64, 80, 7.0, seeds=(1,), V=2)
    ref, ref_mask, views, view_masks = _cuda(ref, ref_mask, views, view_masks)
    init = torch.from_numpy(np.round(true).astype(np.float32)).cuda()
    a, b = ops.reduce2(views[0], view_masks[0]), binding.mncc_reduce2(views[0], view_masks[0])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    a, b = ops.mncc_search_scene_from(ref, ref_mask, views, view_masks, init, 5, 2, 1.0), binding.mncc_search_scene_from(ref, ref_mask, views, view_masks, init, 5, 2, 1.0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    a, b = ops.mncc_search_pyramid(ref, ref_mask, views, view_masks, 1, 5, 2, 4.0, 2, 1.0), binding.mncc_search_pyramid(ref, ref_mask, views, view_masks, 1, 5, 2, 4.0, 2, 1.0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    checks = ("test_schema", "test_faketensor")            # no autograd formula is registered: the result is not differentiable
    torch.library.opcheck(ops.reduce2.default, (views[0], view_masks[0]), test_utils=checks)
    torch.library.opcheck(ops.reduce2.default, (views[0], None), test_utils=checks)
    torch.library.opcheck(ops.mncc_search_scene_from.default, (ref, ref_mask, views, view_masks, init, 5, 2, 1.0), test_utils=checks)
    torch.library.opcheck(ops.mncc_search_scene_from.default, (ref, None, views, None, None, 4, 2, 2.0), test_utils=checks)
    torch.library.opcheck(ops.mncc_search_pyramid.default, (ref, ref_mask, views, view_masks, 1, 5, 2, 4.0, 2, 1.0), test_utils=checks)
    torch.library.opcheck(ops.mncc_search_pyramid.default, (ref, None, views, None, 0, 4, 2, 2.0, 1, 0.5), test_utils=checks)
