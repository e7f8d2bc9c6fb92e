"""GPU (-m gpu): the device half of the x2 / x4 input pipeline.  DeviceImagesetCache at scale 2 and 4 against the host path
(bit for bit, native-ratio files), x3 unchanged through the old and the new entry point, the NaN guard of the collate kernel at
every scale, the target resampler (hrn_resample_targets) against its fp64 numpy reference (scale_ref.py), caches built with
resample_targets=True, and eight steps of the x3 -> x2 fine-tuning recipe of INTEGRATION.md on resampled targets."""
import copy
import os

import numpy as np
import pytest
import torch

import DataLoader as DL
from hrnet_hip import binding, io_binding, resample
from imageset_png import write_imageset, write_png
from scale_ref import (blob_mask, field_image, near_half, ref_resample_hr, ref_resample_sm, restated_read, write_scaled_imageset)

pytestmark = pytest.mark.gpu

N_THREADS = 8
VIEWS = (4, 12, 7, 9, 5, 11)


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    """{ratio: six imagesets with HR / SM stored at that ratio}"""
    root = tmp_path_factory.mktemp("scaled")
    out = {}
    for ratio in (2, 3, 4):
        r = str(root / f"x{ratio}")
        os.makedirs(r)
        out[ratio] = [write_scaled_imageset(r, f"imgset{i:04d}", n, ratio, seed=70 + i) for i, n in enumerate(VIEWS)]
    return out


def _same(host, dev, rng_host=None, rng_dev=None):
    """Tensors and names equal; with both RNG states given, they must be equal too."""
    lrs, alphas, hrs, maps, names = host
    assert names == dev[4]
    for name, h, d in (("lrs", lrs, dev[0]), ("alphas", alphas, dev[1]), ("maps", maps, dev[3])):
        assert d.is_cuda and d.dtype == torch.float32 and torch.equal(d, h.cuda()), name
    if isinstance(hrs, list):
        assert hrs == [] and dev[2] == []
    else:
        assert dev[2].is_cuda and torch.equal(dev[2], hrs.cuda())
    if rng_host is not None:
        assert rng_host[0] == rng_dev[0] and np.array_equal(rng_host[1], rng_dev[1]) and rng_host[2:] == rng_dev[2:]


def _both(ds, cache, indices, min_L, seed=99):
    np.random.seed(seed)
    host = ds.load_batch(indices, min_L, n_threads=N_THREADS)
    rng_host = np.random.get_state()
    np.random.seed(seed)
    dev = cache.load_batch(indices, min_L)
    torch.cuda.synchronize()
    return host, dev, rng_host, np.random.get_state()


# ------------------------------------------------------------------ 6. cache == host path at scale 2 and 4
@pytest.mark.parametrize("scale", [2, 4])
@pytest.mark.parametrize("create_patches,patch_size", [(True, 64), (False, 64), (True, 30)])
@pytest.mark.parametrize("top_k,beta,seed", [(-1, 0.0, None), (-1, 0.0, 5), (5, 0.0, None), (5, 50.0, 7), (40, 50.0, None), (3, 50.0, 11)])
def test_batches_equal_the_host_path(sets, scale, create_patches, patch_size, top_k, beta, seed):
    dirs = sets[scale]
    ds = DL.ImagesetDataset(dirs, {"create_patches": create_patches, "patch_size": patch_size, "scale": scale}, seed=seed, top_k=top_k, beta=beta)
    cache = ds.to_device("cuda", n_threads=N_THREADS)
    assert cache.scale == scale and cache.index.sm_elems == len(dirs) * scale * scale * 128 * 128
    assert len(cache) == len(dirs) and cache.nbytes == 2 * cache.index.lr_elems + 2 * cache.index.hr_elems + cache.index.sm_elems
    for indices, min_L in (([0, 1, 2, 3], 6), ([5, 0, "imgset0003"], 16), ([1], 12), ([2, 4, 1, 0, 5, 3], 32)):
        host, dev, rh, rd = _both(ds, cache, indices, min_L)
        _same(host, dev, rh, rd)
        S = patch_size if create_patches else 128
        assert dev[0].shape == (len(indices), min_L, S, S) and dev[2].shape == dev[3].shape == (len(indices), scale * S, scale * S)
    assert dev[1][3, 4:].abs().sum().item() == 0 and dev[0][3, 4:].abs().max().item() == 0


@pytest.mark.parametrize("scale", [2, 4])
def test_split_without_hr_and_consecutive_batches(sets, scale, tmp_path):
    t = [write_scaled_imageset(str(tmp_path), f"imgset{9000 + i}", n, scale, with_hr=False, seed=5 + i) for i, n in enumerate((4, 6))]
    ds = DL.ImagesetDataset(sets[scale][:2] + t, {"create_patches": False, "patch_size": 64}, top_k=-1, scale=scale)
    cache = ds.to_device(n_threads=N_THREADS)
    for indices in ([2, 3], [0, 2], [1, 0]):
        host, dev, rh, rd = _both(ds, cache, indices, 8)
        _same(host, dev, rh, rd)
    assert isinstance(_both(ds, cache, [2, 3], 8)[1][2], list)
    only_test = DL.ImagesetDataset(t, {"create_patches": True, "patch_size": 64, "scale": scale}, top_k=3, seed=1).to_device(n_threads=N_THREADS)
    assert only_test.hr is None and only_test.load_batch([0, 1], 4)[2] == []
    # consecutive batches from one seed
    ds = DL.ImagesetDataset(sets[scale], {"create_patches": True, "patch_size": 64, "scale": scale}, top_k=5, beta=50.0)
    cache = ds.to_device(n_threads=N_THREADS)
    batches = [[0, 1], [2, 3, 4], [5, 0], [1, 2], [3], [4, 5, 0, 1]]
    np.random.seed(3)
    want = [ds.load_batch(b, 8, n_threads=N_THREADS) for b in batches]
    rng_host = np.random.get_state()
    np.random.seed(3)
    got = list(cache.batches(batches, 8))
    torch.cuda.synchronize()
    for w, g in zip(want, got):
        _same(w, g)
    rng_dev = np.random.get_state()
    assert len(got) == len(batches) and np.array_equal(rng_host[1], rng_dev[1]) and rng_host[2:] == rng_dev[2:]


# ------------------------------------------------------------------ 7. x3 unchanged
@pytest.mark.parametrize("create_patches,patch_size", [(True, 64), (True, 30), (False, 64)])
def test_x3_is_unchanged_through_both_entry_points(sets, create_patches, patch_size):
    ds = DL.ImagesetDataset(sets[3], {"create_patches": create_patches, "patch_size": patch_size}, top_k=5, beta=50.0, seed=7)
    cache = ds.to_device(n_threads=N_THREADS)
    assert cache.scale == 3
    lib = binding.load_library()
    for indices, min_L in (([0, 1, 2, 3], 6), ([2, 4, 1, 0, 5, 3], 32)):
        host, dev, rh, rd = _both(ds, cache, indices, min_L)                    # DeviceImagesetCache.load_batch: the _s entry point
        _same(host, dev, rh, rd)
        np.random.seed(99)
        plan, names, S, have_hr = cache.index.plan(indices, min_L)
        plan_d = torch.from_numpy(plan).cuda()
        B = len(indices)
        mk = lambda *shape: torch.full(shape, 7.0, dtype=torch.float32, device="cuda")
        old = [mk(B, min_L, S, S), mk(B, min_L), mk(B, 3 * S, 3 * S), mk(B, 3 * S, 3 * S)]
        new = [torch.full_like(t, 9.0) for t in old]
        p = binding._ptr
        rc = lib.hrn_collate_device(p(cache.lr), cache.lr.numel(), p(cache.hr), cache.hr.numel(), p(cache.sm), cache.sm.numel(), p(plan_d), B,
                                    min_L, S, p(old[0]), p(old[1]), p(old[2]), p(old[3]), binding._stream())
        assert rc == 0, lib.hrn_last_error()
        binding.collate_device(cache.lr, cache.hr, cache.sm, plan_d, S, new[0], new[1], new[2], new[3], scale=3)
        torch.cuda.synchronize()
        for o, n, d in zip(old, new, dev[:4]):
            assert torch.equal(o, n) and torch.equal(o, d)
        binding.collate_device(cache.lr, cache.hr, cache.sm, plan_d, S, *[t.fill_(5.0) for t in new])        # the default scale is 3
        torch.cuda.synchronize()
        assert all(torch.equal(o, n) for o, n in zip(old, new))


# ------------------------------------------------------------------ 8. the NaN guard at every scale
@pytest.mark.parametrize("scale", [2, 4])
@pytest.mark.parametrize("S", [4, 6])            # the vector path (S % 4 == 0) and the scalar path
def test_bad_plan_rows_give_nan_planes(S, scale):
    """test_gpu_device_cache.py::test_bad_plan_rows_give_nan_planes at scale 2 and 4, plus an HR / SM offset that is aligned and
    inside its arena but whose scale^2 side^2 samples would end beyond it.  The arenas are views at the front of larger
    buffers, so even a broken guard would read only memory owned here."""
    side, min_L, k = 12, 2, scale
    g = np.random.Generator(np.random.PCG64(4))
    lr_h = g.integers(0, 65536, 4 * side * side, dtype=np.uint16)           # four stored views
    hr_h = g.integers(0, 65536, 2 * k * k * side * side, dtype=np.uint16)   # two stored HR images
    sm_h = g.integers(0, 3, 2 * k * k * side * side, dtype=np.uint8)

    def arena(host, dt, spare=1 << 16):
        big = torch.zeros(host.size + spare, dtype=torch.int16 if dt == torch.uint16 else torch.uint8, device="cuda")
        big[:host.size] = torch.from_numpy(host.view(np.int16) if dt == torch.uint16 else host).cuda()
        return big, big[:host.size].view(dt)

    keep_lr, lr = arena(lr_h, torch.uint16)
    keep_hr, hr = arena(hr_h, torch.uint16)
    keep_sm, sm = arena(sm_h, torch.uint8)
    r, c, v, V = 5, 3, side * side, k * k * side * side
    huge = 1 << 62
    rows = [[0, 0, side, r, c, v, -1],                          # good (slot 1 padding)
            [V, V, side, r, c, 2, 0],                           # second HR / SM image: good; slot 0 misaligned
            [0, 0, side, r, c, lr_h.size - 4, 3 * v],           # slot 0 runs past the LR arena
            [V + 4, 0, side, r, c, 2 * v, v],                   # HR: aligned, starts inside, ends 4 samples beyond its arena
            [0, V + 4, side, r, c, 2 * v, v],                   # SM: the same
            [0, 0, side, side - S + 1, c, v, 0],                # corner leaves the image: every plane
            [0, 0, side, r, -1, v, 0],                          # negative corner
            [huge, huge, 1 << 40, r, c, huge, v],               # absurd side and offsets
            [0, 0, (1 << 20) + 1, r, c, 0, v]]                  # side just over the limit
    B = len(rows)
    plan = torch.tensor(rows, dtype=torch.int64, device="cuda")
    mk = lambda *shape: torch.full(shape, 7.0, dtype=torch.float32, device="cuda")
    lrs, alphas, hrs, maps = mk(B, min_L, S, S), mk(B, min_L), mk(B, k * S, k * S), mk(B, k * S, k * S)
    binding.collate_device(lr, hr, sm, plan, S, lrs, alphas, hrs, maps, scale=scale)
    torch.cuda.synchronize()
    lrs, alphas, hrs, maps = (t.cpu().numpy() for t in (lrs, alphas, hrs, maps))

    f = lambda u: (u.astype(np.float64) / 65535.0).astype(np.float32)
    want_lr = lambda off: f(lr_h[off:off + v].reshape(side, side)[r:r + S, c:c + S])
    win = lambda a, i: a[i * V:(i + 1) * V].reshape(k * side, k * side)[k * r:k * r + k * S, k * c:k * c + k * S]
    want_hr = lambda i: f(win(hr_h, i))
    want_sm = lambda i: (win(sm_h, i) != 0).astype(np.float32)
    nan = lambda a: bool(np.isnan(a).all())
    assert np.array_equal(lrs[0, 0], want_lr(v)) and not lrs[0, 1].any() and alphas[0].tolist() == [1, 0]
    assert np.array_equal(hrs[0], want_hr(0)) and np.array_equal(maps[0], want_sm(0))
    assert nan(lrs[1, 0]) and np.array_equal(lrs[1, 1], want_lr(0)) and alphas[1].tolist() == [1, 1]
    assert np.array_equal(hrs[1], want_hr(1)) and np.array_equal(maps[1], want_sm(1))
    assert nan(lrs[2, 0]) and np.array_equal(lrs[2, 1], want_lr(3 * v))
    assert nan(hrs[3]) and np.array_equal(maps[3], want_sm(0)) and np.array_equal(lrs[3, 0], want_lr(2 * v))
    assert nan(maps[4]) and np.array_equal(hrs[4], want_hr(0)) and np.array_equal(lrs[4, 1], want_lr(v))
    for b in (5, 6, 7, 8):
        assert nan(lrs[b]) and nan(hrs[b]) and nan(maps[b]), b
    assert alphas[1:].tolist() == [[1, 1]] * (B - 1)
    with pytest.raises(ValueError, match="2, 3 or 4"):
        binding.collate_device(lr, hr, sm, plan, S, torch.empty(0), alphas, hrs, maps, scale=5)
    del keep_lr, keep_hr, keep_sm


# ------------------------------------------------------------------ 9. the resampling kernel against the fp64 reference
def _round4(n):
    return (n + 3) // 4 * 4


def _device_resample(images, side, R, scale, pad=12):
    """hrn_resample_targets over `images` (uint16 or uint8, each (R side)^2) in one launch -> list of (scale side)^2 arrays.
    Source and destination images sit at spaced, 4-aligned offsets of arenas prefilled with a marker."""
    n_in, n_out = R * side, scale * side
    dt = images[0].dtype
    src_slot, dst_slot = _round4(n_in * n_in) + pad, _round4(n_out * n_out) + pad
    src = np.full(src_slot * len(images) + 8, 3, dt)
    jobs = []
    for i, u in enumerate(images):
        src[8 + i * src_slot:8 + i * src_slot + n_in * n_in] = u.ravel()
        jobs.append((8 + i * src_slot, 4 + (len(images) - 1 - i) * dst_slot))           # results in reverse order
    as_t = lambda a: torch.from_numpy(a.view(np.int16)).cuda().view(torch.uint16) if a.dtype == np.uint16 else torch.from_numpy(a).cuda()
    marker = 0xABCD if dt == np.uint16 else 0xAB
    dst = as_t(np.full(dst_slot * len(images) + 4, marker, dt))
    binding.resample_targets(as_t(src), dst, np.asarray(jobs), n_in, n_out, resample.weight_table(side, R, scale))
    torch.cuda.synchronize()
    out = (dst.view(torch.int16) if dt == np.uint16 else dst).cpu().numpy().view(dt)
    written = np.zeros(out.size, bool)
    for _, o in jobs:
        written[o:o + n_out * n_out] = True
    assert (out[~written] == marker).all()                                              # nothing outside the result images
    return [out[o:o + n_out * n_out].reshape(n_out, n_out) for _, o in jobs]


def _hr_agrees(dev, ref, v):
    """The bound of the issue: within one code everywhere, and equal wherever the reference's unrounded value is farther than
    1e-6 code from a half-integer (any fp64 summation order of <= 144 products of magnitude <= 1.55^2 * 65535 stays within
    144 * 2^-53 * 1.6e5 = 2.5e-9 code of exact, so 1e-6 leaves a factor 400)."""
    d = np.abs(dev.astype(np.int64) - ref.astype(np.int64))
    return bool(d.max() <= 1 and (d[~near_half(v)] == 0).all())


@pytest.mark.parametrize("R,scale", [(3, 2), (3, 4), (2, 4), (4, 2)])
def test_resampling_against_the_fp64_reference(R, scale):
    side = 128
    n_in = R * side
    images = [field_image(n_in, seed=100 * R + 10 * scale + i) for i in range(4)]
    refs = [ref_resample_hr(u, side, R, scale) for u in images]
    below = sum(int((v < 0).sum()) for _, v in refs)
    above = sum(int((v > 65535).sum()) for _, v in refs)
    band = sum(int(near_half(v).sum()) for _, v in refs)
    total = sum(v.size for _, v in refs)
    print(f"resample ({R},{scale}): clipped at 0: {below}, at 65535: {above}, within 1e-6 of a half: {band} of {total}")
    assert below > 0 and above > 0 and band < 1e-4 * total          # conditions on the inputs, on the reference alone
    got = _device_resample(images, side, R, scale)
    worst = max(int(np.abs(g.astype(np.int64) - r.astype(np.int64)).max()) for g, (r, _) in zip(got, refs))
    differ = sum(int((g != r).sum()) for g, (r, _) in zip(got, refs))
    print(f"resample ({R},{scale}): max |device - reference| = {worst} code, {differ} samples differ")
    for g, (r, v) in zip(got, refs):
        assert g.dtype == np.uint16 and _hr_agrees(g, r, v)
        assert not _hr_agrees(g, np.roll(r, 1, axis=1), np.roll(v, 1, axis=1))           # negative control: one output sample off
        assert not _hr_agrees(g, np.roll(r, 1, axis=0), np.roll(v, 1, axis=0))
    # status maps: blob-shaped unclear regions, exact equality with the reference's rule
    masks = [blob_mask(n_in, seed=7 * R + scale + i) for i in range(4)]
    want = [ref_resample_sm(m, side, R, scale) for m in masks]
    assert all(w.mean() >= 0.5 and not w.all() for w in want)
    got = _device_resample([m.astype(np.uint8) * (1 + 37 * i) for i, m in enumerate(masks)], side, R, scale)      # any non-zero value is clear
    for g, w in zip(got, want):
        assert g.dtype == np.uint8 and set(np.unique(g)) <= {0, 1} and np.array_equal(g != 0, w)
        assert not np.array_equal(g != 0, np.roll(w, 1, axis=1)) and not np.array_equal(g != 0, np.roll(w, 1, axis=0))


@pytest.mark.parametrize("R,scale", [(3, 2), (4, 3), (2, 3), (4, 2)])
def test_resampling_tile_edges(R, scale):
    """A side whose output is no multiple of the kernel's 16 x 16 tile: same bound, edge tiles included."""
    side = 21
    u = field_image(R * side, seed=R + scale, noise=300.0)
    ref, v = ref_resample_hr(u, side, R, scale)
    m = blob_mask(R * side, seed=3)
    got = _device_resample([u], side, R, scale)[0]
    assert _hr_agrees(got, ref, v)
    assert np.array_equal(_device_resample([m.astype(np.uint8)], side, R, scale)[0] != 0, ref_resample_sm(m, side, R, scale))


def test_resample_binding_refuses_bad_arguments():
    t16 = lambda n: torch.zeros(n, dtype=torch.int16, device="cuda").view(torch.uint16)
    table = resample.weight_table(8, 3, 2)
    src, dst = t16(24 * 24 + 4), t16(16 * 16)
    ok = dict(src=src, dst=dst, jobs=[[4, 0]], n_in=24, n_out=16, table=table)
    binding.resample_targets(**ok)
    first, count, w = table
    bad_first = first.copy(); bad_first[-1] = 23
    bad_count = count.copy(); bad_count[3] = 13
    for kw, exc in [(dict(jobs=[[8, 0]]), ValueError), (dict(jobs=[[4, 4]]), ValueError), (dict(jobs=[[-4, 0]]), ValueError),
                    (dict(jobs=[4, 0]), ValueError), (dict(n_out=15), ValueError), (dict(n_in=20, n_out=16), ValueError),
                    (dict(dst=torch.zeros(256, dtype=torch.uint8, device="cuda")), ValueError), (dict(src=src.cpu()), RuntimeError),
                    (dict(table=(bad_first, count, w)), ValueError), (dict(table=(first, bad_count, w)), ValueError),
                    (dict(table=(first, count, w[:, :6])), ValueError), (dict(table=(first, count, np.full_like(w, np.nan))), ValueError)]:
        with pytest.raises(exc):
            binding.resample_targets(**dict(ok, **kw))
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 10. caches built with resample_targets=True
def _codes(t):
    """float32 batch of (u / 65535) -> the uint16 codes u (exact: float32 carries 24 bits)."""
    return np.rint(t.cpu().numpy().astype(np.float64) * 65535.0).astype(np.int64)


@pytest.fixture(scope="module")
def x3_fields(tmp_path_factory):
    """Four x3 imagesets whose HR is a field image and whose SM is a blob mask, with what was written."""
    root = str(tmp_path_factory.mktemp("x3fields"))
    out = []
    for i, n in enumerate((4, 9, 6, 5)):
        hr, sm = field_image(384, seed=40 + i), blob_mask(384, seed=50 + i)
        out.append((write_scaled_imageset(root, f"imgset{i:04d}", n, 3, seed=30 + i, hr=hr, sm=sm.astype(np.uint8) * 200), hr, sm))
    return out


@pytest.mark.parametrize("scale", [2, 4])
@pytest.mark.parametrize("create_patches,patch_size,top_k,seed", [(True, 64, -1, None), (True, 30, 5, 7), (False, 64, -1, None)])
def test_cache_with_resampled_targets(x3_fields, scale, create_patches, patch_size, top_k, seed):
    dirs = [d for d, _, _ in x3_fields]
    cfg = {"create_patches": create_patches, "patch_size": patch_size}
    ds3 = DL.ImagesetDataset(dirs, cfg, seed=seed, top_k=top_k, beta=50.0)
    ds = DL.ImagesetDataset(dirs, dict(cfg, scale=scale), seed=seed, top_k=top_k, beta=50.0)
    with pytest.raises(ValueError, match="resample_targets=True"):
        ds.to_device(n_threads=N_THREADS)
    cache3 = ds3.to_device(n_threads=N_THREADS)
    cache = ds.to_device(n_threads=N_THREADS, resample_targets=True)
    assert cache.index.ratios == [3] * 4 and cache.hr.numel() == 4 * (scale * 128) ** 2
    refs = [(ref_resample_hr(hr, 128, 3, scale), ref_resample_sm(sm, 128, 3, scale)) for _, hr, sm in x3_fields]
    P = patch_size if create_patches else 128
    for indices, min_L in (([0, 1, 2, 3], 6), ([3, 1], 4)):
        np.random.seed(77)
        corners = [restated_read(dirs[i], create_patches, patch_size, seed, top_k, 50.0, 3, io_binding.png_read)["corner"] for i in indices]
        state = np.random.get_state()
        np.random.seed(77)
        want3 = cache3.load_batch(indices, min_L)
        np.random.seed(77)
        lrs, alphas, hrs, maps, names = cache.load_batch(indices, min_L)
        torch.cuda.synchronize()
        after = np.random.get_state()
        assert np.array_equal(state[1], after[1]) and state[2:] == after[2:]
        assert torch.equal(lrs, want3[0]) and torch.equal(alphas, want3[1]) and names == want3[4]
        assert hrs.shape == maps.shape == (len(indices), scale * P, scale * P)
        got_hr, got_sm = _codes(hrs), maps.cpu().numpy()
        for b, (i, (x, y)) in enumerate(zip(indices, corners)):
            win = (slice(scale * x, scale * x + scale * P), slice(scale * y, scale * y + scale * P))
            (ref, v), sm = refs[i]
            assert _hr_agrees(got_hr[b], ref[win], v[win])
            assert np.array_equal(got_sm[b], sm[win].astype(np.float32))


def test_mixed_split_in_one_cache(x3_fields, sets):
    """Imagesets stored at the scale are kept as decoded, the others are resampled, in one cache and one batch."""
    scale = 2
    dirs = [sets[2][0], x3_fields[1][0], x3_fields[2][0], sets[2][3], sets[4][4]]
    cfg = {"create_patches": True, "patch_size": 64, "scale": scale}
    ds = DL.ImagesetDataset(dirs, cfg, seed=3, top_k=-1)
    cache = ds.to_device(n_threads=N_THREADS, resample_targets=True)
    assert cache.index.ratios == [2, 3, 3, 2, 4]
    native = DL.ImagesetDataset([dirs[0], dirs[3]], cfg, seed=3, top_k=-1)
    np.random.seed(5)
    want = native.load_batch([0, 1], 6, n_threads=N_THREADS)
    np.random.seed(5)
    lrs, alphas, hrs, maps, names = cache.load_batch([0, 3, 1, 2, 4], 6)
    torch.cuda.synchronize()
    assert names == [os.path.basename(dirs[i]) for i in (0, 3, 1, 2, 4)]
    for got, w in zip((lrs, alphas, hrs, maps), want[:4]):
        assert torch.equal(got[:2].cpu(), w)                                            # stored at x2: the host path's bits
    x, y = restated_read(dirs[1], True, 64, 3, -1, 0.0, 3, io_binding.png_read)["corner"]      # seeded dataset: the corner of every imageset
    win = (slice(2 * x, 2 * x + 128), slice(2 * y, 2 * y + 128))
    for b, i in ((2, 1), (3, 2)):
        (ref, v), sm = ref_resample_hr(x3_fields[i][1], 128, 3, 2), ref_resample_sm(x3_fields[i][2], 128, 3, 2)
        assert _hr_agrees(_codes(hrs[b]), ref[win], v[win]) and np.array_equal(maps[b].cpu().numpy(), sm[win].astype(np.float32))
    # the x4-stored one, against the reference from its decoded files
    hr4, sm4 = io_binding.png_read(os.path.join(dirs[4], "HR.png")), io_binding.png_read(os.path.join(dirs[4], "SM.png")) != 0
    (ref, v), sm = ref_resample_hr(hr4, 128, 4, 2), ref_resample_sm(sm4, 128, 4, 2)
    assert _hr_agrees(_codes(hrs[4]), ref[win], v[win]) and np.array_equal(maps[4].cpu().numpy(), sm[win].astype(np.float32))


# ------------------------------------------------------------------ 11. x3 -> x2 fine-tuning on resampled targets
def test_x2_finetune_from_x3_data(tmp_path):
    """The recipe of INTEGRATION.md end to end: x3 imagesets, a cache at scale 2 with resampled targets, the x3 encoder and
    fusion frozen under a new stride-2 decoder, a fixed ShiftNet (eval mode, fc2 zero: identity registration), FusedAdam on the
    decoder, the registered cPSNR loss.  Eight steps on one fixed batch: the loss goes down."""
    from DeepNetworks.HRNet import HRNet
    from DeepNetworks.ShiftNet import ShiftNet
    from hrnet_hip.losses import get_loss
    from hrnet_hip.optim import FusedAdam
    from oracle import weights

    g = np.random.Generator(np.random.PCG64(21))
    dirs = []
    for i in range(4):
        yy, xx = np.mgrid[0:384, 0:384] / 384.0
        ph = g.random(4)
        field = 0.35 + 0.2 * np.sin(2 * np.pi * (1.3 * xx + ph[0])) * np.cos(2 * np.pi * (0.9 * yy + ph[1])) + 0.1 * np.sin(2 * np.pi * (2.1 * (xx + yy) + ph[2]))
        hr = np.rint(field * 65535 * 0.25).astype(np.uint16)                      # PROBA-V-like brightness: well below full scale
        box = (field * 65535 * 0.25).reshape(128, 3, 128, 3).mean(axis=(1, 3))     # LR = the 3x box average plus small noise
        views = [np.clip(np.rint(box + 20.0 * g.standard_normal((128, 128))), 0, 65535).astype(np.uint16) for _ in range(5)]
        d = write_imageset(str(tmp_path), f"imgset{i:04d}", 5, lr_views=views, hr=hr, seed=60 + i)
        write_png(os.path.join(d, "SM.png"), blob_mask(384, seed=80 + i).astype(np.uint8) * 255)      # blobs, not per-pixel noise
        dirs.append(d)
    scale, P = 2, 64
    ds = DL.ImagesetDataset(dirs, {"create_patches": True, "patch_size": P, "scale": scale}, seed=9, top_k=-1)
    cache = ds.to_device("cuda", n_threads=N_THREADS, resample_targets=True)
    lrs, alphas, hrs, hr_maps, _ = cache.load_batch([0, 1, 2, 3], min_L=4)
    assert hrs.shape == hr_maps.shape == (4, 128, 128) and float(hr_maps.mean()) > 0.5

    torch.manual_seed(0)
    cfg = copy.deepcopy(weights.HRNET_CONFIG)
    cfg["decoder"]["deconv"]["kernel_size"] = cfg["decoder"]["deconv"]["stride"] = scale
    fusion = HRNet(cfg)
    sd = weights.to_torch_state(weights.hrnet_state(1234))                         # stands for the published x3 model
    fusion.load_state_dict({k: v for k, v in sd.items() if not k.startswith("decode.")}, strict=False)
    frozen = [*fusion.encode.parameters(), *fusion.fuse.parameters()]
    for p in frozen:
        p.requires_grad_(False)
    fusion = fusion.cuda().train()
    regis = ShiftNet()
    regis.load_state_dict(weights.to_torch_state(weights.shiftnet_state(4321)))
    regis.fc2.weight.data.zero_()
    for p in regis.parameters():
        p.requires_grad_(False)
    regis = regis.cuda().eval()
    trainable = [p for p in fusion.parameters() if p.requires_grad]
    assert len(trainable) == len(list(fusion.decode.parameters())) > 0
    optimizer = FusedAdam(trainable, lr=1e-3)
    offset = (scale * P - 128) // 2
    losses = []
    for step in range(8):
        optimizer.zero_grad()
        srs = fusion(lrs, alphas)
        assert tuple(srs.shape) == (4, 1, scale * P, scale * P)
        shifts = regis(torch.cat([hrs[:, offset:offset + 128, offset:offset + 128].reshape(-1, 1, 128, 128),
                                  srs[:, :, offset:offset + 128, offset:offset + 128]], 1))
        assert float(shifts.abs().max()) == 0.0
        shifted = regis.transform(shifts.view(-1, 2), srs.view(-1, 1, scale * P, scale * P), device="cuda").view(-1, 1, scale * P, scale * P)[:, 0]
        loss = -get_loss(shifted, hrs, hr_maps, metric="cPSNR", crop=3).mean()
        loss.backward()
        assert all(p.grad is not None and float(p.grad.abs().sum()) > 0 for p in fusion.decode.parameters() if p.numel() > 1)
        assert all(p.grad is None for p in frozen) and all(p.grad is None for p in regis.parameters())
        optimizer.step()
        losses.append(float(loss.detach()))
    print("x2 fine-tune losses:", " ".join(f"{v:.4f}" for v in losses))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
