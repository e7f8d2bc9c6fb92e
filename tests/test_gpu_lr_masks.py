"""GPU (-m gpu): the LR quality masks on the device path.  hrn_collate_device_m with every code in one launch against the host
path's masks and against hrn_collate_device_a's other four outputs; DeviceImagesetCache against ImagesetDataset.load_batch from the
same RNG state; the test split; an unaligned mask output; bad plan rows and bad codes with canaries behind every buffer; the argument
checks; BatchPrefetcher; and the masks reaching register_views on scenes with saturated blobs.  Every mask comparison is bit for bit."""
import os

import numpy as np
import pytest
import torch

import DataLoader as DL
import lr_masks_ref as ref
from hrnet_hip import augment, binding, io_binding, registration
from imageset_png import write_imageset

pytestmark = pytest.mark.gpu

N_THREADS = 8


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    """{ratio: six imagesets (LR side 128) with HR / SM stored at that ratio and quality maps of {0, 1, 128, 255}}"""
    root = tmp_path_factory.mktemp("lr_masks_gpu")
    return {ratio: ref.write_sets(str(root / f"x{ratio}"), ratio) for ratio in (2, 3, 4)}


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def _same(host, dev):
    """A host batch and a device batch, six items each"""
    lrs, alphas, hrs, maps, names, masks = host
    assert len(dev) == 6 and names == dev[4]
    for name, h, d in (("lrs", lrs, dev[0]), ("alphas", alphas, dev[1]), ("maps", maps, dev[3]), ("lr_masks", masks, dev[5])):
        assert d.is_cuda and d.dtype == torch.float32 and torch.equal(d, h.cuda()), name
    if isinstance(hrs, list):
        assert hrs == [] and dev[2] == []
    else:
        assert dev[2].is_cuda and torch.equal(dev[2], hrs.cuda())


def _both(ds, cache, indices, min_L, seed=99):
    np.random.seed(seed)
    host = ds.load_batch(indices, min_L, n_threads=N_THREADS)
    rng_host, codes_host = np.random.get_state(), ds.last_augment
    np.random.seed(seed)
    dev = cache.load_batch(indices, min_L)
    torch.cuda.synchronize()
    assert _same_state(rng_host, np.random.get_state()) and codes_host == cache.last_augment
    return host, dev


def _launch(cache, plan_d, S, min_L, scale, codes, have_hr=True, masks=True, fill=7.0):
    """-> (lrs, alphas, hrs, maps, lr_masks or None) of one launch into buffers filled with `fill`"""
    B = plan_d.shape[0]
    mk = lambda *shape: torch.full(shape, fill, dtype=torch.float32, device="cuda")
    lrs, alphas, maps = mk(B, min_L, S, S), mk(B, min_L), mk(B, scale * S, scale * S)
    hrs = mk(B, scale * S, scale * S) if have_hr else None
    lr_masks = mk(B, min_L, S, S) if masks else None
    codes_d = None if codes is None else torch.tensor(codes, dtype=torch.int32, device="cuda")
    binding.collate_device(cache.lr, cache.hr, cache.sm, plan_d, S, lrs, alphas, hrs, maps, scale=scale, codes=codes_d,
                           qm_arena=cache.qm if masks else None, lr_masks=lr_masks)
    torch.cuda.synchronize()
    return lrs, alphas, hrs, maps, lr_masks


# ------------------------------------------------------------------ 1. every code in one launch
@pytest.mark.parametrize("scale", [2, 3, 4])
@pytest.mark.parametrize("S", [64, 36, 30])
def test_every_code_in_one_launch(sets, scale, S):
    """Eight samples with codes 0..7 (and rotated by three): S = 64 is four whole LDS tiles per mask plane, 36 two tiles per axis with
    an edge tile of 4, 30 the per-element path; patch columns of every residue mod 4, so both funnel-shift branches of load4_u8 run;
    imageset 0 has 4 views, so two padding slots at min_L = 6.  The masks against the host library's, the other four outputs against
    the same launch without masks (hrn_collate_device_a)."""
    dirs = sets[scale]
    ds = DL.ImagesetDataset(dirs, {"create_patches": True, "patch_size": S, "scale": scale}, top_k=-1, lr_masks=True)
    cache = ds.to_device("cuda", n_threads=N_THREADS)
    assert cache.qm.dtype == torch.uint8 and cache.qm.numel() == cache.lr.numel() and int(cache.qm.max()) == 1
    indices, min_L = [0, 1, 2, 3, 4, 5, 0, 3], 6
    np.random.seed(41)
    plan, names, _, have_hr = cache.index.plan(indices, min_L)
    hi = 128 - S
    plan[:, 3] = [5, 17, hi, 0, 33, hi - 1, 1, 2]
    plan[:, 4] = [8, 21, 2, 3, hi, hi - 1, 13, 7]
    assert {int(c) % 4 for c in plan[:, 4]} == {0, 1, 2, 3} and have_hr
    plan_d = torch.from_numpy(plan).cuda()
    order = [np.flip(np.argsort(cache.index.clearances[i])) for i in indices]
    paths = lambda stem: [[os.path.join(dirs[i], f"{stem}{cache.index.ids[i][v]}.png") for v in o] for i, o in zip(indices, order)]
    for codes in (list(range(8)), [(c + 3) % 8 for c in range(8)], None):
        host = io_binding.collate(paths("LR"), [os.path.join(dirs[i], "HR.png") for i in indices], [os.path.join(dirs[i], "SM.png") for i in indices],
                                  min_L, 128, patch=S, corners=[(int(r), int(c)) for r, c in plan[:, 3:5]], n_threads=N_THREADS, scale=scale,
                                  codes=codes, qm_paths_per_set=paths("QM"))
        got = _launch(cache, plan_d, S, min_L, scale, codes)
        without = _launch(cache, plan_d, S, min_L, scale, codes, masks=False, fill=9.0)
        assert torch.equal(got[4], torch.from_numpy(host["lr_masks"]).cuda())
        assert not got[4][0, 4:].any() and got[1][0].tolist() == [1, 1, 1, 1, 0, 0] and 0.5 < float(got[4][:, :4].mean()) < 0.9
        for name, g, w, h in zip(("lrs", "alphas", "hrs", "maps"), got, without, (host["lrs"], host["alphas"], host["hrs"], host["maps"])):
            assert torch.equal(g, w) and torch.equal(g, torch.from_numpy(h).cuda()), name


def test_unaligned_mask_output_takes_the_per_element_path(sets):
    """S % 4 == 0, every other output 16-byte aligned, lr_masks a view one float into its buffer: the per-element path, all codes."""
    ds = DL.ImagesetDataset(sets[3], {"create_patches": True, "patch_size": 32}, top_k=-1, lr_masks=True)
    cache = ds.to_device("cuda", n_threads=N_THREADS)
    np.random.seed(2)
    plan, _, S, _ = cache.index.plan([0, 1, 2, 3, 4, 5, 1, 2], 5)
    plan_d = torch.from_numpy(plan).cuda()
    codes = list(range(8))
    want = _launch(cache, plan_d, S, 5, 3, codes)
    mk = lambda *shape: torch.full(shape, 3.0, dtype=torch.float32, device="cuda")
    lrs, alphas, hrs, maps = mk(8, 5, S, S), mk(8, 5), mk(8, 3 * S, 3 * S), mk(8, 3 * S, 3 * S)
    buf = mk(8 * 5 * S * S + 5)
    lr_masks = buf[1:1 + 8 * 5 * S * S].view(8, 5, S, S)
    assert lr_masks.data_ptr() % 16 == 4 and all(t.data_ptr() % 16 == 0 for t in (lrs, alphas, hrs, maps))
    binding.collate_device(cache.lr, cache.hr, cache.sm, plan_d, S, lrs, alphas, hrs, maps, codes=torch.arange(8, dtype=torch.int32, device="cuda"),
                           qm_arena=cache.qm, lr_masks=lr_masks)
    torch.cuda.synchronize()
    for g, w in zip((lrs, alphas, hrs, maps, lr_masks), want):
        assert torch.equal(g, w)
    assert buf[0].item() == 3.0 and (buf[1 + 8 * 5 * S * S:] == 3.0).all()


# ------------------------------------------------------------------ 2. the cache against the host path
@pytest.mark.parametrize("create_patches,patch_size", [(True, 64), (False, 64), (True, 30)])
@pytest.mark.parametrize("top_k,beta,seed,mode", [(-1, 0.0, None, "dihedral"), (5, 50.0, 7, "flip"), (40, 50.0, None, None), (3, 0.0, 11, "dihedral"),
                                                  (5, 0.0, None, None)])
def test_cache_equals_the_host_path(sets, create_patches, patch_size, top_k, beta, seed, mode):
    ds = DL.ImagesetDataset(sets[3], {"create_patches": create_patches, "patch_size": patch_size, "lr_masks": True}, seed=seed, top_k=top_k, beta=beta,
                            augment=mode)
    cache = ds.to_device("cuda", n_threads=N_THREADS)
    assert cache.nbytes == 2 * cache.lr.numel() + 2 * cache.hr.numel() + cache.sm.numel() + cache.lr.numel()
    for k, (indices, min_L) in enumerate((([0, 1, 2, 3], 6), ([5, 0, "imgset0003"], 16), ([2, 4, 1, 0, 5, 3], 3))):
        host, dev = _both(ds, cache, indices, min_L, seed=99 + k)
        _same(host, dev)
        S = patch_size if create_patches else 128
        assert dev[5].shape == (len(indices), min_L, S, S) and not dev[5][dev[1] == 0].any()
    got = list(cache.batches([[0, 1], [2]], 4))
    assert all(len(b) == 6 for b in got)
    off = DL.ImagesetDataset(sets[3], {"create_patches": create_patches, "patch_size": patch_size}, top_k=top_k, beta=beta).to_device(n_threads=N_THREADS)
    assert off.qm is None and len(off.load_batch([0, 1], 4)) == 5 and off.nbytes == cache.nbytes - cache.lr.numel()


@pytest.mark.parametrize("scale", [2, 4])
def test_cache_equals_the_host_path_at_other_scales_and_with_resampled_targets(sets, scale):
    cfg = {"create_patches": True, "patch_size": 36, "scale": scale, "augment": "dihedral", "lr_masks": True}
    ds = DL.ImagesetDataset(sets[scale], cfg, top_k=5, beta=50.0)
    cache = ds.to_device("cuda", n_threads=N_THREADS)
    host, dev = _both(ds, cache, [2, 4, 1, 0, 5, 3], 8, seed=7)
    _same(host, dev)
    # x3 files in a cache at this scale: the masks do not depend on the targets, the rest is what the cache gives without masks
    resampled = DL.ImagesetDataset(sets[3], cfg, top_k=5, beta=50.0).to_device("cuda", n_threads=N_THREADS, resample_targets=True)
    plain = DL.ImagesetDataset(sets[3], dict(cfg, lr_masks=False), top_k=5, beta=50.0).to_device("cuda", n_threads=N_THREADS, resample_targets=True)
    np.random.seed(7)
    got = resampled.load_batch([2, 4, 1, 0, 5, 3], 8)
    np.random.seed(7)
    want = plain.load_batch([2, 4, 1, 0, 5, 3], 8)
    torch.cuda.synchronize()
    assert resampled.last_augment == ds.last_augment and torch.equal(got[5], host[5].cuda())       # the same LR views and QM files at every ratio
    assert all(torch.equal(g, w) for g, w in zip(got[:4], want[:4])) and got[4] == want[4] and got[2].shape == (6, scale * 36, scale * 36)


def test_split_without_hr(sets, tmp_path):
    """Without the HR units the mask units start earlier in the grid."""
    t = [write_imageset(str(tmp_path), f"imgset{9000 + i}", n, with_hr=False, seed=5 + i) for i, n in enumerate((4, 6))]
    for i, d in enumerate(t):
        ref.rewrite_quality_maps(d, 40 + i)
    for patch in (64, 30):
        ds = DL.ImagesetDataset(sets[3][:2] + t, {"create_patches": True, "patch_size": patch}, top_k=-1, augment="dihedral", lr_masks=True)
        cache = ds.to_device(n_threads=N_THREADS)
        for k, indices in enumerate(([2, 3], [0, 2], [3, 2, 1, 0])):
            host, dev = _both(ds, cache, indices, 8, seed=30 + k)
            _same(host, dev)
            assert dev[2] == [] and host[2] == [] and dev[5].any()
        host, dev = _both(ds, cache, [1, 0], 8, seed=3)
        _same(host, dev)
        assert isinstance(dev[2], torch.Tensor)


# ------------------------------------------------------------------ 3. bad rows, bad codes, bad arguments
def _with_canary(shape, fill=7.0, spare=64):
    """-> (whole buffer, view of `shape` at its front); the `spare` floats behind the view are the canary"""
    n = int(np.prod(shape))
    whole = torch.full((n + spare,), fill, dtype=torch.float32, device="cuda")
    return whole, whole[:n].view(shape)


@pytest.mark.parametrize("scale", [2, 3, 4])
@pytest.mark.parametrize("S", [4, 8, 6])         # the vector path (one LDS tile of side 4 / 8 per mask plane) and the scalar path
def test_bad_plan_rows_and_bad_codes_give_nan_mask_planes(S, scale):
    """The rows of test_gpu_augment.py::test_bad_plan_rows_give_nan_planes_under_every_code under each of the eight codes, and the
    codes of test_a_bad_code_gives_nan_planes_for_that_sample_only on good rows.  The arenas are views at the front of larger buffers
    (even a broken guard would read only memory owned here) and every output has a canary behind it."""
    side, min_L, k = 12, 2, scale
    g = np.random.Generator(np.random.PCG64(4))
    lr_h = g.integers(0, 65536, 4 * side * side, dtype=np.uint16)
    qm_h = g.integers(0, 2, 4 * side * side, dtype=np.uint8)
    hr_h = g.integers(0, 65536, 2 * k * k * side * side, dtype=np.uint16)
    sm_h = g.integers(0, 3, 2 * k * k * side * side, dtype=np.uint8)

    def arena(host, dt, spare=1 << 16):
        big = torch.zeros(host.size + spare, dtype=torch.int16 if dt == torch.uint16 else torch.uint8, device="cuda")
        big[:host.size] = torch.from_numpy(host.view(np.int16) if dt == torch.uint16 else host).cuda()
        return big, big[:host.size].view(dt)

    keep_lr, lr = arena(lr_h, torch.uint16)
    keep_qm, qm = arena(qm_h, torch.uint8)
    keep_hr, hr = arena(hr_h, torch.uint16)
    keep_sm, sm = arena(sm_h, torch.uint8)
    r, c, v, V = 3, 1, side * side, k * k * side * side
    huge = 1 << 62
    rows = [[0, 0, side, r, c, v, -1],                          # good (slot 1 padding)
            [V, V, side, r, c, 2, 0],                           # second HR / SM image: good; slot 0 misaligned
            [0, 0, side, r, c, lr_h.size - 4, 3 * v],           # slot 0 runs past the LR (and so the QM) arena
            [V + 4, 0, side, r, c, 2 * v, v],                   # HR ends 4 samples beyond its arena
            [0, V + 4, side, r, c, 2 * v, v],                   # SM: the same
            [0, 0, side, side - S + 1, c, v, 0],                # corner leaves the image: every plane
            [0, 0, side, r, -1, v, 0],                          # negative corner
            [huge, huge, 1 << 40, r, c, huge, v]]               # absurd side and offsets
    B = len(rows)
    plan = torch.tensor(rows, dtype=torch.int64, device="cuda")
    good = torch.tensor([[0, 0, side, r, c, v, 2 * v]] * 6, dtype=torch.int64, device="cuda")
    want_qm = lambda off: qm_h[off:off + v].reshape(side, side)[r:r + S, c:c + S].astype(np.float32)
    nan = lambda a: bool(np.isnan(a).all())

    def launch(table, codes):
        n = table.shape[0]
        bufs = [_with_canary(shape) for shape in ((n, min_L, S, S), (n, min_L), (n, k * S, k * S), (n, k * S, k * S), (n, min_L, S, S))]
        plain = [torch.full_like(b[1], 5.0) for b in bufs[:4]]
        codes_d = torch.tensor(codes, dtype=torch.int32, device="cuda")
        binding.collate_device(lr, hr, sm, table, S, *[b[1] for b in bufs[:4]], scale=scale, codes=codes_d, qm_arena=qm, lr_masks=bufs[4][1])
        binding.collate_device(lr, hr, sm, table, S, *plain, scale=scale, codes=codes_d)
        torch.cuda.synchronize()
        for (whole, view), p in zip(bufs, plain + [None]):
            assert (whole[view.numel():] == 7.0).all()                                      # the canary behind every buffer
            assert p is None or torch.equal(torch.nan_to_num(view, nan=-1.0), torch.nan_to_num(p, nan=-1.0))   # the other four: as without masks
        return bufs[4][1].cpu().numpy(), bufs[1][1].cpu().numpy()

    for code in range(8):
        masks, alphas = launch(plan, [code] * B)
        eq = lambda got, want: np.array_equal(got, augment.apply(want, code))
        assert eq(masks[0, 0], want_qm(v)) and not masks[0, 1].any() and alphas[0].tolist() == [1, 0]
        assert nan(masks[1, 0]) and eq(masks[1, 1], want_qm(0))
        assert nan(masks[2, 0]) and eq(masks[2, 1], want_qm(3 * v))
        for b in (3, 4):                                                                 # a bad HR or SM row leaves the masks alone
            assert eq(masks[b, 0], want_qm(2 * v)) and eq(masks[b, 1], want_qm(v))
        for b in (5, 6, 7):
            assert nan(masks[b]), (code, b)
    codes = [5, 8, 2, -1, 7, 1 << 20]
    masks, alphas = launch(good, codes)
    for b, code in enumerate(codes):
        if 0 <= code <= 7:
            assert np.array_equal(masks[b, 0], augment.apply(want_qm(v), code)) and np.array_equal(masks[b, 1], augment.apply(want_qm(2 * v), code))
        else:
            assert nan(masks[b]), (b, code)
    assert alphas.tolist() == [[1, 1]] * 6
    del keep_lr, keep_qm, keep_hr, keep_sm


def test_argument_checks_refuse_before_any_launch(sets):
    ds = DL.ImagesetDataset(sets[3], {"create_patches": True, "patch_size": 32}, top_k=-1, lr_masks=True)
    cache = ds.to_device("cuda", n_threads=N_THREADS)
    np.random.seed(1)
    plan, _, S, _ = cache.index.plan([0, 1], 4)
    plan_d = torch.from_numpy(plan).cuda()
    lib, p = binding.load_library(), binding._ptr
    mk = lambda *shape: torch.full(shape, 7.0, dtype=torch.float32, device="cuda")
    outs = [mk(2, 4, S, S), mk(2, 4), mk(2, 3 * S, 3 * S), mk(2, 3 * S, 3 * S), mk(2, 4, S, S)]

    def call(qm, qm_elems, masks):
        rc = lib.hrn_collate_device_m(p(cache.lr), cache.lr.numel(), p(cache.hr), cache.hr.numel(), p(cache.sm), cache.sm.numel(), qm, qm_elems,
                                      p(plan_d), 2, 4, S, 3, p(outs[0]), p(outs[1]), p(outs[2]), p(outs[3]), masks, None, binding._stream())
        torch.cuda.synchronize()
        return rc

    for qm, n, masks in ((p(cache.qm), cache.qm.numel() - 4, p(outs[4])), (p(cache.qm), cache.qm.numel() + 4, p(outs[4])), (None, 0, p(outs[4])),
                         (None, cache.lr.numel(), p(outs[4])), (p(cache.qm), cache.qm.numel(), None), (p(cache.qm[1:]), cache.qm.numel(), p(outs[4]))):
        assert call(qm, n, masks) == -2
        assert all(bool((t == 7.0).all()) for t in outs)                             # nothing was launched
    assert call(p(cache.qm), cache.qm.numel(), p(outs[4])) == 0 and not any(bool((t == 7.0).all()) for t in outs)
    with pytest.raises(ValueError, match="go together"):
        binding.collate_device(cache.lr, cache.hr, cache.sm, plan_d, S, *outs[:4], lr_masks=outs[4])
    with pytest.raises(ValueError, match="lr_masks"):
        binding.collate_device(cache.lr, cache.hr, cache.sm, plan_d, S, *outs[:4], qm_arena=cache.qm, lr_masks=outs[4][:, :3])


# ------------------------------------------------------------------ 4. the prefetcher
def test_the_prefetcher_yields_the_masks(sets):
    ds = DL.ImagesetDataset(sets[3], {"create_patches": True, "patch_size": 36, "augment": "flip"}, top_k=5, beta=50.0, lr_masks=True)
    batches = [[0, 1], [2, 3, 4], [5, 0], [3]]
    np.random.seed(3)
    want = [ds.load_batch(b, 6, n_threads=N_THREADS) for b in batches]
    state = np.random.get_state()
    np.random.seed(3)
    got = list(DL.BatchPrefetcher(ds, batches, 6, device="cuda", n_threads=N_THREADS))
    torch.cuda.synchronize()
    assert _same_state(state, np.random.get_state()) and len(got) == len(want)
    for w, g in zip(want, got):
        _same(w, g)
    on_host = list(DL.BatchPrefetcher(ds, batches[:2], 6))
    assert all(len(b) == 6 and not b[5].is_cuda for b in on_host)
    plain = DL.ImagesetDataset(sets[3], {"create_patches": True, "patch_size": 36}, top_k=5)
    assert all(len(b) == 5 for b in DL.BatchPrefetcher(plain, batches[:2], 6, device="cuda"))


# ------------------------------------------------------------------ 5. end to end: the masks reach the registration
def test_the_masks_reach_registration(tmp_path):
    """Two imagesets of four 48 x 48 views, each a known sub-pixel shift of one scene with a saturated blob of its own under a QM that
    is zero on the blob and a one-pixel rim (lr_masks_ref.write_registration_sets; test_lr_masks_host.py asks the same of the fp64
    restatement).  cache.load_batch, full frames, top_k = -1, then register_views with the batch's masks, P = 7, 5 levels, radius 1:
    the shifts relative to the clearest view within the 0.02 px of DESIGN 7f.  No claim about the unmasked result."""
    dirs, wanted = ref.write_registration_sets(str(tmp_path / "reg"))
    ds = DL.ImagesetDataset(dirs, {"create_patches": False, "patch_size": 0}, top_k=-1, lr_masks=True)
    cache = ds.to_device("cuda", n_threads=N_THREADS)
    lrs, alphas, hrs, hr_maps, names, lr_masks = cache.load_batch([0, 1], ref.REG_VIEWS)
    assert lrs.shape == lr_masks.shape == (ref.REG_SETS, ref.REG_VIEWS, ref.REG_SIDE, ref.REG_SIDE) and bool(alphas.all())
    assert not lr_masks[lrs == 1.0].any()                                               # every saturated sample is masked
    registered, valid, shifts = registration.register_views(lrs, lr_masks, points_per_dim=7, levels=5, radius=1.0)
    torch.cuda.synchronize()
    err = (shifts.cpu().numpy().astype(np.float64) - np.array(wanted)).reshape(-1, 2)
    print("shift errors (px), per view:", np.round(np.abs(err).max(axis=1), 4).tolist())
    assert registered.shape == lrs.shape and np.abs(err).max() <= 0.02
