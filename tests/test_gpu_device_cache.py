"""GPU (-m gpu): DataLoader.DeviceImagesetCache - imagesets decoded once into HBM, each batch assembled by one
hrn_collate_device launch - is torch.equal to ImagesetDataset.load_batch moved to the device, tensor by tensor, with the same
names and the same numpy RNG state afterwards, over patches / whole images, view sampling with and without a seed, truncation
and padding to min_L, the test split (no HR.png), consecutive batches, every uint16 code, and the errors of the host path."""
import numpy as np
import pytest
import torch

import DataLoader as DL
from hrnet_hip import binding
from imageset_png import write_imageset

pytestmark = pytest.mark.gpu

N_THREADS = 8


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("sets"))
    return [write_imageset(root, f"imgset{i:04d}", n, seed=70 + i) for i, n in enumerate((4, 12, 7, 9, 5, 11))]


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


@pytest.mark.parametrize("create_patches,patch_size", [(True, 64), (False, 64), (True, 30)])
@pytest.mark.parametrize("top_k,beta,seed", [(-1, 0.0, None), (-1, 0.0, 5), (5, 0.0, None), (5, 50.0, 7), (40, 50.0, None), (3, 50.0, 11)])
def test_batches_equal_the_host_path(sets, create_patches, patch_size, top_k, beta, seed):
    ds = DL.ImagesetDataset(sets, {"create_patches": create_patches, "patch_size": patch_size}, seed=seed, top_k=top_k, beta=beta)
    cache = ds.to_device("cuda", n_threads=N_THREADS)
    assert len(cache) == len(sets) and cache.nbytes == 2 * cache.index.lr_elems + 2 * cache.index.hr_elems + cache.index.sm_elems
    for indices, min_L in (([0, 1, 2, 3], 6), ([5, 0, "imgset0003"], 16), ([1], 12), ([2, 4, 1, 0, 5, 3], 32)):
        host, dev, rh, rd = _both(ds, cache, indices, min_L)
        _same(host, dev, rh, rd)
        S = patch_size if create_patches else 128
        assert dev[0].shape == (len(indices), min_L, S, S) and dev[3].shape == (len(indices), 3 * S, 3 * S)
    # padding slots: alpha 0 and zero frames (imageset 0 has 4 views)
    assert dev[1][3, 4:].abs().sum().item() == 0 and dev[0][3, 4:].abs().max().item() == 0


def test_test_split_without_hr(sets, tmp_path):
    t = [write_imageset(str(tmp_path), f"imgset{9000 + i}", n, with_hr=False, seed=5 + i) for i, n in enumerate((4, 6))]
    ds = DL.ImagesetDataset(sets[:2] + t, {"create_patches": False, "patch_size": 64}, top_k=-1)
    cache = ds.to_device(n_threads=N_THREADS)
    for indices in ([2, 3], [0, 2], [1, 0]):
        host, dev, rh, rd = _both(ds, cache, indices, 8)
        _same(host, dev, rh, rd)
    assert isinstance(_both(ds, cache, [2, 3], 8)[1][2], list)
    only_test = DL.ImagesetDataset(t, {"create_patches": True, "patch_size": 64}, top_k=3, seed=1).to_device(n_threads=N_THREADS)
    assert only_test.hr is None and only_test.load_batch([0, 1], 4)[2] == []


def test_consecutive_batches(sets):
    ds = DL.ImagesetDataset(sets, {"create_patches": True, "patch_size": 64}, top_k=5, beta=50.0)
    cache = ds.to_device(n_threads=N_THREADS)
    batches = [[0, 1], [2, 3, 4], [5, 0], [1, 2], [3], [4, 5, 0, 1]] * 2
    np.random.seed(3)
    want = [ds.load_batch(b, 8, n_threads=N_THREADS) for b in batches]
    rng_host = np.random.get_state()
    np.random.seed(3)
    got = list(cache.batches(batches, 8))
    torch.cuda.synchronize()
    assert len(got) == len(batches)
    for w, g in zip(want, got):
        _same(w, g)                              # per batch: tensors and names; the RNG state is compared after the last batch
    rng_dev = np.random.get_state()
    assert np.array_equal(rng_host[1], rng_dev[1]) and rng_host[2:] == rng_dev[2:]


def test_every_uint16_code(tmp_path):
    """All 65,536 codes through the value rule: spread over four 128x128 LR views, and all of them in one 384x384 HR image."""
    codes = np.random.Generator(np.random.PCG64(8)).permutation(65536).astype(np.uint16)
    views = list(codes.reshape(4, 128, 128))
    hr = np.resize(codes[::-1], (384, 384)).astype(np.uint16)
    d = write_imageset(str(tmp_path), "imgset0001", 4, lr_views=views, hr=hr, seed=2)
    ds = DL.ImagesetDataset([d], {"create_patches": False, "patch_size": 64}, top_k=-1)
    cache = ds.to_device(n_threads=N_THREADS)
    host, dev, rh, rd = _both(ds, cache, [0], 4)
    _same(host, dev, rh, rd)
    got = dev[0][0].cpu().numpy()
    assert np.unique(got).size == 65536 and np.unique(dev[2].cpu().numpy()).size == 65536
    want = {int(c): np.float32(np.float64(c) / 65535.0) for c in range(65536)}
    order = np.flip(np.argsort(np.load(f"{d}/clearance.npy")))
    for slot, v in enumerate(order):
        assert np.array_equal(got[slot], np.vectorize(want.get, otypes=[np.float32])(views[v]))


def test_errors_match_the_host_path(sets, tmp_path):
    small = write_imageset(str(tmp_path), "imgset0500", 5, lr=64, seed=3)
    ds = DL.ImagesetDataset(sets + [small], {"create_patches": True, "patch_size": 32}, top_k=-1)
    cache = ds.to_device(n_threads=N_THREADS)
    with pytest.raises(ValueError, match="share the LR size"):
        ds.load_batch([0, 6], 4)
    with pytest.raises(ValueError, match="share the LR size"):
        cache.load_batch([0, 6], 4)
    with pytest.raises(KeyError):
        ds.load_batch(["imgset0404"], 4)
    with pytest.raises(KeyError):
        cache.load_batch(["imgset0404"], 4)
    host, dev, rh, rd = _both(ds, cache, [6, "imgset0500"], 7)      # a 64x64 imageset on its own is fine
    _same(host, dev, rh, rd)


@pytest.mark.parametrize("S", [4, 6])            # the vector path (S % 4 == 0) and the scalar path
def test_bad_plan_rows_give_nan_planes(S):
    """hrn_collate_device's guard: a plan row whose image is misaligned or runs past its arena, whose corner leaves the stored
    image, or whose side is absurd (an int64 overflow if multiplied out) gives NaN planes; the good slots of the same launch are
    exact.  The arenas are views at the front of larger buffers, so even a broken guard would read only memory owned here."""
    side, M, min_L = 12, binding.COLLATE_META, 2
    g = np.random.Generator(np.random.PCG64(4))
    lr_h = g.integers(0, 65536, 4 * side * side, dtype=np.uint16)           # four stored views
    hr_h = g.integers(0, 65536, 9 * side * side, dtype=np.uint16)
    sm_h = g.integers(0, 3, 9 * side * side, dtype=np.uint8)

    def arena(host, dt, spare=1 << 16):
        big = torch.zeros(host.size + spare, dtype=torch.int16 if dt == torch.uint16 else torch.uint8, device="cuda")
        big[:host.size] = torch.from_numpy(host.view(np.int16) if dt == torch.uint16 else host).cuda()
        return big, big[:host.size].view(dt)

    keep_lr, lr = arena(lr_h, torch.uint16)
    keep_hr, hr = arena(hr_h, torch.uint16)
    keep_sm, sm = arena(sm_h, torch.uint8)
    r, c, v = 5, 3, side * side
    huge = 1 << 62
    rows = [[0, 0, side, r, c, v, -1],                          # good (slot 1 padding)
            [0, 0, side, r, c, 2, 0],                           # slot 0 misaligned
            [0, 0, side, r, c, lr_h.size - 4, 3 * v],           # slot 0 runs past the LR arena
            [4, 0, side, r, c, 2 * v, v],                       # HR runs past its arena
            [0, 0, side, side - S + 1, c, v, 0],                # corner leaves the image: every plane
            [0, 0, side, r, -1, v, 0],                          # negative corner
            [huge, huge, 1 << 40, r, c, huge, v]]               # absurd side and offsets
    B = len(rows)
    plan = torch.tensor(rows, dtype=torch.int64, device="cuda")
    mk = lambda *shape: torch.full(shape, 7.0, dtype=torch.float32, device="cuda")
    lrs, alphas, hrs, maps = mk(B, min_L, S, S), mk(B, min_L), mk(B, 3 * S, 3 * S), mk(B, 3 * S, 3 * S)
    binding.collate_device(lr, hr, sm, plan, S, lrs, alphas, hrs, maps)
    torch.cuda.synchronize()
    lrs, alphas, hrs, maps = (t.cpu().numpy() for t in (lrs, alphas, hrs, maps))

    f = lambda u: (u.astype(np.float64) / 65535.0).astype(np.float32)
    want_lr = lambda off: f(lr_h[off:off + v].reshape(side, side)[r:r + S, c:c + S])
    want_hr = f(hr_h.reshape(3 * side, 3 * side)[3 * r:3 * r + 3 * S, 3 * c:3 * c + 3 * S])
    want_sm = (sm_h.reshape(3 * side, 3 * side)[3 * r:3 * r + 3 * S, 3 * c:3 * c + 3 * S] != 0).astype(np.float32)
    nan = lambda a: bool(np.isnan(a).all())
    assert np.array_equal(lrs[0, 0], want_lr(v)) and not lrs[0, 1].any() and alphas[0].tolist() == [1, 0]
    assert np.array_equal(hrs[0], want_hr) and np.array_equal(maps[0], want_sm)
    assert nan(lrs[1, 0]) and np.array_equal(lrs[1, 1], want_lr(0)) and alphas[1].tolist() == [1, 1]
    assert nan(lrs[2, 0]) and np.array_equal(lrs[2, 1], want_lr(3 * v))
    assert nan(hrs[3]) and np.array_equal(maps[3], want_sm) and np.array_equal(lrs[3, 0], want_lr(2 * v))
    for b in (4, 5, 6):
        assert nan(lrs[b]) and nan(hrs[b]) and nan(maps[b]), b
    assert alphas[1:].tolist() == [[1, 1]] * (B - 1)
    del keep_lr, keep_hr, keep_sm
