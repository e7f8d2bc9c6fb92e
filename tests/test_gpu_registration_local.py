"""GPU: the shift field of a scene (hrnet_hip.registration's mncc_search_local / shift_field / register_scene_local over
hrn_mncc_search_local / hrn_mncc_apply_field): one block is the global search bit for bit; every level of every
block against the existing device path (mncc_grid_scene with the reference mask restricted to the block) and against the fp64
restatement (tests/registration_local_ref.py) at the chosen points; blocks without enough common pixels; shift_field against
shift_scene for a constant field and against the fp64 per-pixel sampler for fields whose whole parts change inside a tile; recovery of
a known linear field; bit-reproducibility, the independence of a view from its batch, and the custom ops.

The shapes: (1, 2, 16, 16) / 64 is one tile in one block; (1, 2, 130, 203) / 64 has 2 x 3 blocks, a two-row and an eleven-column ragged
tile merged into the last blocks; (1, 2, 257, 144) / 128 has 2 x 1 blocks of two and three tile rows, the last a one-pixel row; (2, 3,
200, 264) / 64 has 3 x 4 blocks with interior nodes, and a batch.

The bounds are sections 7f / 7g's, carried over: 4e-7 of a score against fp64, 8e-7 between two device paths (both within 4e-7 of
fp64; here only the subtracted mean differs), 8e-7 of a resampled pixel against fp64."""
import functools

import numpy as np
import pytest
import torch

import registration_local_ref as L
import registration_ref as R

pytestmark = pytest.mark.gpu

from registration_cases import APPLY_BOUND, DEVICE_BOUND, SCORE_BOUND      # sections 7f / 7g: 4e-7 of a score against fp64, 8e-7 between two
                                                                           # device paths, 8e-7 of a resampled pixel against fp64
NODE_BOUND_PX = 1.5 * 0.0243  # tests/test_registration_local_host.py: 1.5 times the restatement's worst node error over seeds 1..3

CASES = [((1, 2, 16, 16), 64), ((1, 2, 130, 203), 64), ((1, 2, 257, 144), 128), ((2, 3, 200, 264), 64)]
IDS = ["x".join(map(str, s)) + f"_b{b}" for s, b in CASES]
MASKS = [True, False]


@functools.lru_cache(maxsize=None)
def case(B, V, H, W):
    """-> (ref (B,H,W), ref_mask, views (B,V,H,W), view_masks) as numpy float32, one seeded scene per sample, shifts within +-0.9."""
    parts = [R.scene(H, W, R.random_shifts(V, 0.9, seed=9000 + 13 * b + H * W), seed=200 * b + H * W) for b in range(B)]
    return tuple(np.stack([p[i] for p in parts]) for i in range(4))


def _cuda(*arrays):
    return tuple(None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays)


def data(shape, masks):
    ref, ref_mask, views, view_masks = case(*shape)
    return (ref, ref_mask, views, view_masks) if masks else (ref, None, views, None)


@functools.lru_cache(maxsize=None)
def searched(shape, block, masks, P=6):
    """The device's own path for a case: the global shifts (P = 7, five levels of radius 1), then the local search from them with four
    levels of radius 0.5 at P = 6, whose widths 1, 1/4, 1/16, 1/64 are fp32 values that mncc_grid_scene can be given.
    -> (init (B,V,2), field (B,V,by,bx,2), trace (B,V,by,bx,4,3), ok (B,V,by,bx)) as numpy."""
    from hrnet_hip import registration as G
    ref, ref_mask, views, view_masks = _cuda(*data(shape, masks))
    init = G.mncc_search_scene(views, view_masks, ref, ref_mask, points_per_dim=7, levels=5, radius=1.0)
    field, trace, ok = G.mncc_search_local(views, view_masks, ref, ref_mask, block=block, init=init, points_per_dim=P, levels=4, radius=0.5,
                                           min_valid=0.25, return_trace=True)
    by, bx = G.local_blocks(shape[2], shape[3], block)
    assert field.shape == shape[:2] + (by, bx, 2) and trace.shape == shape[:2] + (by, bx, 4, 3) and ok.shape == shape[:2] + (by, bx)
    assert (by, bx) == (L.blocks(shape[2], block), L.blocks(shape[3], block))
    return tuple(t.cpu().numpy() for t in (init, field, trace, ok))


# ----------------------------------------------------------------------------- one block is the global search
@pytest.mark.parametrize("masks", MASKS)
def test_one_block_is_the_scene_search_bit_for_bit(masks):
    from hrnet_hip import registration as G
    ref, ref_mask, views, view_masks = _cuda(*data((1, 2, 130, 203), masks))
    for P, levels, radius in ((7, 5, 1.0), (4, 3, 2.0)):
        shifts, trace = G.mncc_search_scene(views, view_masks, ref, ref_mask, points_per_dim=P, levels=levels, radius=radius, return_trace=True)
        field, ltrace, ok = G.mncc_search_local(views, view_masks, ref, ref_mask, block=4096, init=None, points_per_dim=P, levels=levels,
                                                radius=radius, min_valid=0.0, return_trace=True)
        assert field.shape == (1, 2, 1, 1, 2) and ltrace.shape == (1, 2, 1, 1, levels, 3)
        assert torch.equal(field[:, :, 0, 0], shifts) and torch.equal(ltrace[:, :, 0, 0], trace) and bool((ok == 1).all())


# ----------------------------------------------------------------------------- every level of every block
@pytest.mark.parametrize("masks", MASKS)
@pytest.mark.parametrize("shape,block", CASES, ids=IDS)
def test_every_level_of_every_block_is_the_grid_of_the_restricted_reference(shape, block, masks):
    """mncc_grid_scene with the reference mask restricted to the block and the previous trace point as centre scores the same grid; it
    centres the reference on the block's mean where the local search centres on the frame's, and the score does not depend on either."""
    from hrnet_hip import registration as G
    B, V, H, W = shape
    P = 6
    ref, ref_mask, views, view_masks = data(shape, masks)
    init, field, trace, ok = searched(shape, block, masks)
    d_views, d_masks, d_ref = _cuda(views, view_masks, ref)
    widths = R.level_widths(P, 4, 0.5)
    worst_at, worst_gap, infs = 0.0, 0.0, 0
    for i, rows in enumerate(L.bounds(H, block)):
        for j, cols in enumerate(L.bounds(W, block)):
            rm = np.stack([L.restricted(None if ref_mask is None else ref_mask[b], (H, W), rows, cols) for b in range(B)])
            centres = init.copy()
            for k, width in enumerate(widths):
                assert float(np.float32(width)) == width
                scores = G.mncc_grid_scene(d_views, d_masks, d_ref, torch.from_numpy(rm).cuda(), centres=torch.from_numpy(centres).cuda(),
                                           points_per_dim=P, width=width).cpu().numpy()
                for b in range(B):
                    for v in range(V):
                        dy, dx, got = trace[b, v, i, j, k]
                        if not np.isfinite(scores[b, v]).any():
                            assert (dy, dx) == tuple(centres[b, v]) and np.isneginf(got)
                            infs += 1
                            continue
                        dys, dxs = R.grid_coords(centres[b, v, 0], width, P), R.grid_coords(centres[b, v, 1], width, P)
                        ii, jj = np.flatnonzero(dys == dy), np.flatnonzero(dxs == dx)
                        assert len(ii) and len(jj), f"view {b},{v} block {i},{j} level {k}: ({dy}, {dx}) is no point of {dys} x {dxs}"
                        at = float(scores[b, v, ii[0], jj[0]])
                        assert np.isfinite(got) and np.isfinite(at)
                        worst_at = max(worst_at, abs(float(got) - at))
                        worst_gap = max(worst_gap, float(scores[b, v].max()) - float(got))
                centres = np.ascontiguousarray(trace[:, :, i, j, k, :2])
            assert np.array_equal(np.where(ok[:, :, i, j, None] == 1, trace[:, :, i, j, -1, :2], init), field[:, :, i, j])
    print(f"local levels {shape} block {block} masks={masks}: max |trace score - grid_scene at the point| = {worst_at:.3e}, max (grid_scene "
          f"maximum - trace score) = {worst_gap:.3e}, {infs} levels without a finite score")
    assert worst_at <= DEVICE_BOUND and worst_gap <= DEVICE_BOUND


@pytest.mark.parametrize("masks", MASKS)
@pytest.mark.parametrize("shape,block", CASES, ids=IDS)
def test_trace_scores_match_fp64_at_the_chosen_points(shape, block, masks):
    """One fp64 score per view, block and level, and the fp64 count of common pixels behind `ok`."""
    B, V, H, W = shape
    ref, ref_mask, views, view_masks = data(shape, masks)
    init, field, trace, ok = searched(shape, block, masks)
    worst = 0.0
    for b in range(B):
        for v in range(V):
            vm = None if view_masks is None else view_masks[b, v]
            for i, rows in enumerate(L.bounds(H, block)):
                for j, cols in enumerate(L.bounds(W, block)):
                    for k in range(trace.shape[4]):
                        dy, dx, got = trace[b, v, i, j, k]
                        want = L.block_score(ref[b], None if ref_mask is None else ref_mask[b], views[b, v], vm, (dy, dx), rows, cols)
                        assert np.isneginf(got) == np.isneginf(want)
                        if np.isfinite(want):
                            worst = max(worst, abs(float(got) - want))
                    n = L.common_valid(None if ref_mask is None else ref_mask[b], vm, (H, W), trace[b, v, i, j, -1, :2], rows, cols)
                    area = (rows[1] - rows[0]) * (cols[1] - cols[0])
                    assert abs(n - 0.25 * area) > 0.0025 * area, "a block within 1 % of the threshold"
                    assert bool(ok[b, v, i, j]) == (np.isfinite(trace[b, v, i, j, -1, 2]) and n >= 0.25 * area)
    print(f"local trace {shape} block {block} masks={masks}: max |trace score - fp64| = {worst:.3e}; ok {int(ok.sum())} of {ok.size} blocks")
    assert worst <= SCORE_BOUND


# ----------------------------------------------------------------------------- ok and the fallback
def test_blocks_without_enough_common_pixels_keep_init():
    from hrnet_hip import registration as G
    ref, ref_mask, views, view_masks = L.fallback_cases()
    init = np.broadcast_to(np.float32(L.FALLBACK_INIT), (1, 2, 2)).copy()
    field, trace, ok = G.mncc_search_local(*_cuda(views[None], view_masks[None], ref[None], ref_mask[None]), block=L.FALLBACK_BLOCK,
                                           init=torch.from_numpy(init).cuda(), points_per_dim=5, levels=3, radius=0.5, min_valid=0.25,
                                           return_trace=True)
    field, trace, ok = field.cpu().numpy(), trace.cpu().numpy(), ok.cpu().numpy()
    for v in range(2):
        want_field, want_trace, want_ok, n = L.search_local(ref, ref_mask, views[v], view_masks[v], L.FALLBACK_BLOCK, init[0, v], 5, 3, 0.5, 0.25)
        for j, area in ((0, 70 * 64), (1, 70 * 76)):
            assert abs(n[0, j] - 0.25 * area) > 0.0025 * area
        assert np.array_equal(ok[0, v] == 1, want_ok) and want_ok.tolist() == [[False, True]] and set(np.unique(ok)) <= {0.0, 1.0}
        assert np.array_equal(field[0, v, 0, 0], init[0, v])
        assert np.isneginf(trace[0, v, 0, 0, -1, 2]) == (v == 0) and np.isneginf(want_trace[0, 0, -1, 2]) == (v == 0)
        assert np.array_equal(field[0, v, 0, 1], trace[0, v, 0, 1, -1, :2]) and np.abs(field[0, v, 0, 1] - want_field[0, 1]).max() <= 0.02
    # and with min_valid = 0 the block with a finite score is taken
    field0, _, ok0 = G.mncc_search_local(*_cuda(views[None], view_masks[None], ref[None], ref_mask[None]), block=L.FALLBACK_BLOCK,
                                         init=torch.from_numpy(init).cuda(), points_per_dim=5, levels=3, radius=0.5, min_valid=0.0,
                                         return_trace=True)
    assert ok0.cpu().numpy().tolist() == [[[[0.0, 1.0]], [[1.0, 1.0]]]]
    assert np.array_equal(field0.cpu().numpy()[0, 1, 0, 0], trace[0, 1, 0, 0, -1, :2])


# ----------------------------------------------------------------------------- the resampler by a field
APPLY_SHIFTS = [(0.37, -1.62), (-3.5, 2.25)]


@pytest.mark.parametrize("masks", MASKS)
@pytest.mark.parametrize("shape,block", CASES, ids=IDS)
def test_shift_field_with_a_constant_field_is_shift_scene(shape, block, masks):
    from hrnet_hip import registration as G
    B, V, H, W = shape
    _, _, views, view_masks = _cuda(*data(shape, masks))
    by, bx = G.local_blocks(H, W, block)
    for k in range(2):
        shifts = torch.tensor([[APPLY_SHIFTS[(b + v + k) % 2] for v in range(V)] for b in range(B)], device="cuda")
        shifts[0, 0] += torch.tensor([0.123456, -0.654321], device="cuda") * k
        const = shifts[:, :, None, None, :].expand(B, V, by, bx, 2).contiguous()
        got, want = G.shift_field(views, view_masks, const, block), G.shift_scene(views, view_masks, shifts)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        assert bool(want[1].any())


def synthetic_field(B, V, by, bx):
    """Nodes from -3.5 to +2.25: dy rises along the nodes in row-major order, dx falls, and every view starts somewhere else."""
    n = by * bx
    ramp = np.linspace(-3.5, 2.25, n) if n > 1 else np.array([-3.5])
    f = np.zeros((B, V, by, bx, 2), np.float32)
    for b in range(B):
        for v in range(V):
            r = np.roll(ramp, b + 2 * v)
            f[b, v, ..., 0], f[b, v, ..., 1] = r.reshape(by, bx), r[::-1].reshape(by, bx)
    return f


@pytest.mark.parametrize("masks", MASKS)
@pytest.mark.parametrize("shape,block", CASES, ids=IDS)
def test_shift_field_matches_the_fp64_sampler_per_pixel(shape, block, masks):
    """The searched field, and a synthetic one whose whole parts change inside a tile.  `valid` is compared at every pixel: a bilinear
    mask sample on 0.5 is decided by the definition (> is strict) on both sides; one within 1e-9 of 0.5 and off it would be a matter of
    rounding, and so would a coordinate within 1e-12 of a whole number: the fields have neither, asserted on the fp64 side."""
    from hrnet_hip import registration as G
    B, V, H, W = shape
    _, _, views, view_masks = data(shape, masks)
    by, bx = L.blocks(H, block), L.blocks(W, block)
    worst, near, whole_parts = 0.0, 0, set()
    for name, field in (("searched", searched(shape, block, masks)[1]), ("synthetic", synthetic_field(B, V, by, bx))):
        out, valid = G.shift_field(*_cuda(views, view_masks, field), block)
        out, valid = out.cpu().numpy(), valid.cpu().numpy()
        for b in range(B):
            for v in range(V):
                exact = L.field_at_pixels(field[b, v], H, W, block, rounded=False)
                assert np.abs(exact - np.round(exact)).min() > 1e-12
                px = L.field_at_pixels(field[b, v], H, W, block)
                want, want_valid, bil = L.sample_field(views[b, v], None if view_masks is None else view_masks[b, v], px)
                off = np.abs(bil - 0.5)
                near += int(((off > 0.0) & (off <= 1e-9)).sum())
                assert np.array_equal(valid[b, v], want_valid.astype(np.float32))
                assert np.all(out[b, v][~want_valid] == 0.0)
                worst = max(worst, float(np.abs(out[b, v] - want)[want_valid].max()) if want_valid.any() else 0.0)
                if name == "synthetic":
                    whole_parts |= set(np.floor(px[..., 0].astype(np.float64)).astype(int).ravel().tolist())
    print(f"shift_field {shape} block {block} masks={masks}: max |device - fp64| = {worst:.3e}; {near} pixels with the fp64 bilinear mask "
          f"within 1e-9 of 0.5 and off it; whole parts of the synthetic dy: {sorted(whole_parts)}")
    assert near == 0
    assert by * bx == 1 or len(whole_parts) >= 5                 # the whole parts do change inside the frame's tiles
    assert worst <= APPLY_BOUND


# ----------------------------------------------------------------------------- a known field
def test_search_recovers_a_linear_field_at_the_nodes():
    """The host test's scenes of seeds 1 and 2 as a batch of two, the global search and the local one as there."""
    from hrnet_hip import registration as G
    H, W, block = 130, 203, 64
    t = L.linear_field(H, W)
    ref, ref_mask, views, view_masks = (np.stack(a) for a in zip(*(L.warped_scene(H, W, [t], seed) for seed in (1, 2))))
    d = _cuda(views, view_masks)
    kw = dict(ref=torch.from_numpy(ref).cuda(), ref_mask=torch.from_numpy(ref_mask).cuda())
    registered, valid, field, shifts = G.register_scene_local(*d, block=block, local_levels=4, local_radius=0.5, min_valid=0.25,
                                                              points_per_dim=7, levels=5, radius=1.0, **kw)
    assert torch.equal(shifts, G.mncc_search_scene(*d, points_per_dim=7, levels=5, radius=1.0, **kw))
    f2, _, ok = G.mncc_search_local(*d, block=block, init=shifts, points_per_dim=7, levels=4, radius=0.5, min_valid=0.25, return_trace=True, **kw)
    want = G.shift_field(*d, field, block)
    assert torch.equal(field, f2) and bool((ok == 1).all()) and torch.equal(registered, want[0]) and torch.equal(valid, want[1])
    ny, nx = np.meshgrid(L.nodes(H, block), L.nodes(W, block), indexing="ij")
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    truth = L.recovered(t, y, x)
    field, shifts = field.cpu().numpy().astype(np.float64), shifts.cpu().numpy().astype(np.float64)
    for b in range(2):
        node_err = np.sqrt(((field[b, 0] - L.recovered(t, ny, nx)) ** 2).sum(-1))
        local = np.sqrt(((L.field_at_pixels(field[b, 0], H, W, block).astype(np.float64) - truth) ** 2).sum(-1))
        glob = np.sqrt(((shifts[b, 0] - truth) ** 2).sum(-1))
        print(f"seed {b + 1}: node error {node_err.min():.4f} .. {node_err.max():.4f} px; per pixel: local mean {local.mean():.4f}, global mean "
              f"{glob.mean():.4f} px")
        assert node_err.max() <= NODE_BOUND_PX
        assert local.mean() < glob.mean() / 3.0


# ----------------------------------------------------------------------------- reproducibility and independence
def test_search_and_apply_are_bit_reproducible_and_a_view_does_not_depend_on_its_batch():
    from hrnet_hip import registration as G
    shape, block = (2, 3, 200, 264), 64
    ref, ref_mask, views, view_masks = _cuda(*data(shape, True))
    init = G.mncc_search_scene(views, view_masks, ref, ref_mask, levels=4)
    kw = dict(block=block, points_per_dim=7, levels=3, radius=0.5, return_trace=True)
    runs = [G.mncc_search_local(views, view_masks, ref, ref_mask, init=init, **kw) for _ in range(2)]
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    field, trace, ok = runs[0]
    applied = [G.shift_field(views, view_masks, field, block) for _ in range(2)]
    assert torch.equal(applied[0][0], applied[1][0]) and torch.equal(applied[0][1], applied[1][1])
    for b, v in ((1, 2), (0, 1)):
        one = (views[b:b + 1, v:v + 1], view_masks[b:b + 1, v:v + 1], ref[b:b + 1], ref_mask[b:b + 1])
        f1, t1, ok1 = G.mncc_search_local(*one, init=init[b:b + 1, v:v + 1], **kw)
        assert torch.equal(f1[0, 0], field[b, v]) and torch.equal(t1[0, 0], trace[b, v]) and torch.equal(ok1[0, 0], ok[b, v])
        a1 = G.shift_field(one[0], one[1], f1, block)
        assert torch.equal(a1[0][0, 0], applied[0][0][b, v]) and torch.equal(a1[1][0, 0], applied[0][1][b, v])


# ----------------------------------------------------------------------------- the custom ops
def test_ops_are_the_binding_calls_and_pass_opcheck():
    from hrnet_hip import binding
    ops = torch.ops.hrnet_hip
    ref, ref_mask, views, view_masks = _cuda(*data((1, 2, 130, 203), True))
    init = torch.tensor([[[0.25, -0.5], [0.0, 0.0]]], device="cuda")
    got = ops.mncc_search_local(ref, ref_mask, views, view_masks, init, 5, 2, 0.5, 64, 0.25)
    want = binding.mncc_search_local(ref, ref_mask, views, view_masks, init, 5, 2, 0.5, 64, 0.25)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    field = got[0]
    got, want = ops.shift_field(views, view_masks, field, 64), binding.mncc_apply_field(views, view_masks, field, 64)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    checks = ("test_schema", "test_faketensor")
    torch.library.opcheck(ops.mncc_search_local.default, (ref, ref_mask, views, view_masks, init, 5, 2, 0.5, 64, 0.25), test_utils=checks)
    torch.library.opcheck(ops.mncc_search_local.default, (ref, None, views, None, None, 4, 2, 1.0, 128, 0.0), test_utils=checks)
    torch.library.opcheck(ops.shift_field.default, (views, view_masks, field, 64), test_utils=checks)
    torch.library.opcheck(ops.shift_field.default, (views, None, field, 64), test_utils=checks)
