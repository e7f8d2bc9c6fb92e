"""GPU (-m gpu): flip / rotate augmentation on the device path.  hrn_collate_device_a with every code in one launch against
augment.apply of the un-augmented launch; DeviceImagesetCache against the host path from the same RNG state; a bad code and
bad plan rows under every code; the test split; resampled targets; five bf16 training steps from an augmented cache.  Every
comparison is bit for bit: the transform moves values and computes none."""
import os

import numpy as np
import pytest
import torch

import DataLoader as DL
from hrnet_hip import augment, binding
from imageset_png import write_imageset
from scale_ref import write_scaled_imageset

pytestmark = pytest.mark.gpu

N_THREADS = 8
VIEWS = (4, 12, 7, 9, 5, 11)


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    """{ratio: six imagesets with HR / SM stored at that ratio}"""
    root = tmp_path_factory.mktemp("augment_gpu")
    out = {}
    for ratio in (2, 3, 4):
        r = str(root / f"x{ratio}")
        os.makedirs(r)
        out[ratio] = [write_scaled_imageset(r, f"imgset{i:04d}", n, ratio, seed=70 + i) for i, n in enumerate(VIEWS)]
    return out


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def _same(host, dev):
    lrs, alphas, hrs, maps, names = host
    assert names == dev[4]
    for name, h, d in (("lrs", lrs, dev[0]), ("alphas", alphas, dev[1]), ("maps", maps, dev[3])):
        assert d.is_cuda and d.dtype == torch.float32 and torch.equal(d, h.cuda()), name
    if isinstance(hrs, list):
        assert hrs == [] and dev[2] == []
    else:
        assert dev[2].is_cuda and torch.equal(dev[2], hrs.cuda())


def _launch(cache, plan_d, S, min_L, scale, codes, have_hr=True, fill=7.0):
    B = plan_d.shape[0]
    mk = lambda *shape: torch.full(shape, fill, dtype=torch.float32, device="cuda")
    lrs, alphas, maps = mk(B, min_L, S, S), mk(B, min_L), mk(B, scale * S, scale * S)
    hrs = mk(B, scale * S, scale * S) if have_hr else None
    codes_d = None if codes is None else torch.tensor(codes, dtype=torch.int32, device="cuda")
    binding.collate_device(cache.lr, cache.hr, cache.sm, plan_d, S, lrs, alphas, hrs, maps, scale=scale, codes=codes_d)
    torch.cuda.synchronize()
    return lrs, alphas, hrs, maps


# ------------------------------------------------------------------ 1. every code in one launch
@pytest.mark.parametrize("scale", [2, 3, 4])
@pytest.mark.parametrize("create_patches,patch_size", [(True, 64), (True, 30), (False, 128)])
def test_every_code_in_one_launch(sets, scale, create_patches, patch_size):
    """Eight samples with codes 0..7 (then rotated by three, so that every imageset meets other codes): the vector path with
    its LDS tiles at S = 64 and S = 128 (HR / SM planes of up to 512 a side: 256 tiles over 16 blocks), the per-element path at
    S = 30; corners of every column alignment, odd ones included; imageset 0 has padding slots at min_L = 6."""
    ds = DL.ImagesetDataset(sets[scale], {"create_patches": create_patches, "patch_size": patch_size, "scale": scale}, top_k=-1)
    cache = ds.to_device("cuda", n_threads=N_THREADS)
    indices, min_L = [0, 1, 2, 3, 4, 5, 0, 3], 6
    np.random.seed(41)
    plan, names, S, have_hr = cache.index.plan(indices, min_L)
    assert S == patch_size and have_hr
    if create_patches:
        hi = 128 - S
        plan[:, 3] = [5, 17, hi, 0, 33, hi - 1, 1, 2]
        plan[:, 4] = [8, 21, 2, 3, hi, hi - 1, 13, 7]
        assert {int(c) % 4 for c in plan[:, 4]} == {0, 1, 2, 3} and (plan[:, 4] % 2 == 1).sum() >= 3
    plan_d = torch.from_numpy(plan).cuda()
    plain = _launch(cache, plan_d, S, min_L, scale, None)
    assert not any(torch.isnan(t).any() or (t == 7.0).all() for t in plain)
    assert plain[1][0].tolist() == [1, 1, 1, 1, 0, 0] and not plain[0][0, 4:].any()
    for codes in (list(range(8)), [(c + 3) % 8 for c in range(8)], [0] * 8, [7] * 8):
        got = _launch(cache, plan_d, S, min_L, scale, codes, fill=9.0)
        assert torch.equal(got[1], plain[1])
        for b, c in enumerate(codes):
            for name, g, p in zip(("lrs", "hrs", "maps"), (got[0], got[2], got[3]), (plain[0], plain[2], plain[3])):
                assert torch.equal(g[b], augment.apply(p[b], c)), (name, b, c)
    # the old entry points: hrn_collate_device_s is the new one without codes
    lib, p = binding.load_library(), binding._ptr
    old = [torch.full_like(t, 5.0) for t in plain]
    rc = lib.hrn_collate_device_s(p(cache.lr), cache.lr.numel(), p(cache.hr), cache.hr.numel(), p(cache.sm), cache.sm.numel(), p(plan_d), 8,
                                  min_L, S, scale, p(old[0]), p(old[1]), p(old[2]), p(old[3]), binding._stream())
    torch.cuda.synchronize()
    assert rc == 0 and all(torch.equal(o, n) for o, n in zip(old, plain))


def test_unaligned_outputs_take_the_per_element_path(sets):
    """S % 4 == 0 but output buffers that are not 16-byte aligned: the per-element path, all eight codes."""
    ds = DL.ImagesetDataset(sets[3], {"create_patches": True, "patch_size": 32}, top_k=-1)
    cache = ds.to_device("cuda", n_threads=N_THREADS)
    np.random.seed(2)
    plan, _, S, _ = cache.index.plan([0, 1, 2, 3, 4, 5, 1, 2], 5)
    plan_d = torch.from_numpy(plan).cuda()
    plain = _launch(cache, plan_d, S, 5, 3, None)
    off = lambda *shape: torch.full((int(np.prod(shape)) + 1,), 3.0, dtype=torch.float32, device="cuda")[1:].view(shape)
    lrs, alphas, hrs, maps = off(8, 5, S, S), off(8, 5), off(8, 3 * S, 3 * S), off(8, 3 * S, 3 * S)
    assert lrs.data_ptr() % 16 == 4
    binding.collate_device(cache.lr, cache.hr, cache.sm, plan_d, S, lrs, alphas, hrs, maps, codes=torch.arange(8, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    for c in range(8):
        for g, p in zip((lrs, hrs, maps), (plain[0], plain[2], plain[3])):
            assert torch.equal(g[c], augment.apply(p[c], c)), c
    assert torch.equal(alphas, plain[1])


# ------------------------------------------------------------------ 2. the cache against the host path
def _both(ds, cache, indices, min_L, seed=99):
    np.random.seed(seed)
    host = ds.load_batch(indices, min_L, n_threads=N_THREADS)
    rng_host, codes_host = np.random.get_state(), ds.last_augment
    np.random.seed(seed)
    dev = cache.load_batch(indices, min_L)
    torch.cuda.synchronize()
    assert _same_state(rng_host, np.random.get_state())
    assert codes_host == cache.last_augment and len(codes_host) == len(indices) and all(isinstance(c, int) for c in codes_host)
    return host, dev


@pytest.mark.parametrize("create_patches,patch_size", [(True, 64), (False, 64), (True, 30)])
@pytest.mark.parametrize("top_k,beta,seed", [(-1, 0.0, None), (-1, 0.0, 5), (5, 0.0, None), (5, 50.0, 7), (40, 50.0, None), (3, 50.0, 11)])
def test_cache_equals_the_host_path(sets, create_patches, patch_size, top_k, beta, seed):
    """The parameter grid of test_gpu_device_cache.py::test_batches_equal_the_host_path, augmentation on."""
    ds = DL.ImagesetDataset(sets[3], {"create_patches": create_patches, "patch_size": patch_size}, seed=seed, top_k=top_k, beta=beta,
                            augment="dihedral")
    cache = ds.to_device("cuda", n_threads=N_THREADS)
    seen = set()
    for k, (indices, min_L) in enumerate((([0, 1, 2, 3], 6), ([5, 0, "imgset0003"], 16), ([1], 12), ([2, 4, 1, 0, 5, 3], 32))):
        host, dev = _both(ds, cache, indices, min_L, seed=99 + k)
        _same(host, dev)
        seen |= set(cache.last_augment)
        S = patch_size if create_patches else 128
        assert dev[0].shape == (len(indices), min_L, S, S) and dev[3].shape == (len(indices), 3 * S, 3 * S)
    assert dev[1][3, 4:].abs().sum().item() == 0 and dev[0][3, 4:].abs().max().item() == 0          # padding slots stay zeros, alpha 0
    assert len(seen) >= (1 if seed is not None else 4)                # a seeded dataset re-seeds before every draw: one code


@pytest.mark.parametrize("scale", [2, 4])
@pytest.mark.parametrize("create_patches,patch_size,mode", [(True, 64, "dihedral"), (True, 30, "flip"), (False, 64, "dihedral")])
def test_cache_equals_the_host_path_at_other_scales(sets, scale, create_patches, patch_size, mode):
    ds = DL.ImagesetDataset(sets[scale], {"create_patches": create_patches, "patch_size": patch_size, "scale": scale, "augment": mode},
                            top_k=5, beta=50.0)
    cache = ds.to_device("cuda", n_threads=N_THREADS)
    for k, (indices, min_L) in enumerate((([0, 1, 2, 3], 6), ([2, 4, 1, 0, 5, 3], 8))):
        host, dev = _both(ds, cache, indices, min_L, seed=7 + k)
        _same(host, dev)
        assert all(c < augment.MODES[mode] for c in cache.last_augment)
    # consecutive batches from one seed, through cache.batches and through BatchPrefetcher onto the device
    batches = [[0, 1], [2, 3, 4], [5, 0], [1, 2], [3], [4, 5, 0, 1]]
    np.random.seed(3)
    want, want_codes = [], []
    for b in batches:
        want.append(ds.load_batch(b, 8, n_threads=N_THREADS))
        want_codes.append(ds.last_augment)
    state = np.random.get_state()
    np.random.seed(3)
    got = []
    for batch in cache.batches(batches, 8):
        got.append((batch, cache.last_augment))
    torch.cuda.synchronize()
    assert _same_state(state, np.random.get_state()) and [c for _, c in got] == want_codes
    np.random.seed(3)
    pf = DL.BatchPrefetcher(ds, batches, 8, device="cuda", n_threads=N_THREADS)
    fetched = [(batch, pf.last_augment) for batch in pf]
    torch.cuda.synchronize()
    assert _same_state(state, np.random.get_state()) and [c for _, c in fetched] == want_codes
    for w, (g, _), (f, _) in zip(want, got, fetched):
        _same(w, g)
        _same(w, f)


# ------------------------------------------------------------------ 3. errors and edges
@pytest.mark.parametrize("S", [64, 30])
def test_a_bad_code_gives_nan_planes_for_that_sample_only(sets, S):
    ds = DL.ImagesetDataset(sets[3], {"create_patches": True, "patch_size": S}, top_k=-1)
    cache = ds.to_device("cuda", n_threads=N_THREADS)
    np.random.seed(6)
    plan, _, _, _ = cache.index.plan([0, 1, 2, 3, 4, 5], 6)
    plan_d = torch.from_numpy(plan).cuda()
    plain = _launch(cache, plan_d, S, 6, 3, None)
    codes = [5, 8, 2, -1, 7, 1 << 20]
    got = _launch(cache, plan_d, S, 6, 3, codes)
    assert torch.equal(got[1], plain[1])                              # alphas as usual
    for b, c in enumerate(codes):
        for g, p in zip((got[0], got[2], got[3]), (plain[0], plain[2], plain[3])):
            if 0 <= c <= 7:
                assert torch.equal(g[b], augment.apply(p[b], c)), (b, c)
            else:
                assert bool(torch.isnan(g[b]).all()), (b, c)
    with pytest.raises(ValueError, match="codes"):
        binding.collate_device(cache.lr, cache.hr, cache.sm, plan_d, S, *got, codes=torch.zeros(6, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError, match="codes"):
        binding.collate_device(cache.lr, cache.hr, cache.sm, plan_d, S, *got, codes=torch.zeros(5, dtype=torch.int32, device="cuda"))


@pytest.mark.parametrize("scale", [2, 3, 4])
@pytest.mark.parametrize("S", [4, 8, 6])         # the vector path (one LDS tile of side 4 / 8 for LR) and the scalar path
def test_bad_plan_rows_give_nan_planes_under_every_code(S, scale):
    """The rows of test_gpu_device_cache.py::test_bad_plan_rows_give_nan_planes, every one under each of the eight codes.  The
    arenas are views at the front of larger buffers, so even a broken guard would read only memory owned here."""
    side, min_L, k = 12, 2, scale
    g = np.random.Generator(np.random.PCG64(4))
    lr_h = g.integers(0, 65536, 4 * side * side, dtype=np.uint16)
    hr_h = g.integers(0, 65536, 2 * k * k * side * side, dtype=np.uint16)
    sm_h = g.integers(0, 3, 2 * k * k * side * side, dtype=np.uint8)

    def arena(host, dt, spare=1 << 16):
        big = torch.zeros(host.size + spare, dtype=torch.int16 if dt == torch.uint16 else torch.uint8, device="cuda")
        big[:host.size] = torch.from_numpy(host.view(np.int16) if dt == torch.uint16 else host).cuda()
        return big, big[:host.size].view(dt)

    keep_lr, lr = arena(lr_h, torch.uint16)
    keep_hr, hr = arena(hr_h, torch.uint16)
    keep_sm, sm = arena(sm_h, torch.uint8)
    r, c, v, V = 3, 1, side * side, k * k * side * side
    huge = 1 << 62
    rows = [[0, 0, side, r, c, v, -1],                          # good (slot 1 padding)
            [V, V, side, r, c, 2, 0],                           # second HR / SM image: good; slot 0 misaligned
            [0, 0, side, r, c, lr_h.size - 4, 3 * v],           # slot 0 runs past the LR arena
            [V + 4, 0, side, r, c, 2 * v, v],                   # HR ends 4 samples beyond its arena
            [0, V + 4, side, r, c, 2 * v, v],                   # SM: the same
            [0, 0, side, side - S + 1, c, v, 0],                # corner leaves the image: every plane
            [0, 0, side, r, -1, v, 0],                          # negative corner
            [huge, huge, 1 << 40, r, c, huge, v]]               # absurd side and offsets
    B = len(rows)
    plan = torch.tensor(rows, dtype=torch.int64, device="cuda")
    f = lambda u: (u.astype(np.float64) / 65535.0).astype(np.float32)
    want_lr = lambda off: f(lr_h[off:off + v].reshape(side, side)[r:r + S, c:c + S])
    win = lambda a, i: a[i * V:(i + 1) * V].reshape(k * side, k * side)[k * r:k * r + k * S, k * c:k * c + k * S]
    want_hr = lambda i: f(win(hr_h, i))
    want_sm = lambda i: (win(sm_h, i) != 0).astype(np.float32)
    nan = lambda a: bool(np.isnan(a).all())
    for code in range(8):
        mk = lambda *shape: torch.full(shape, 7.0, dtype=torch.float32, device="cuda")
        lrs, alphas, hrs, maps = mk(B, min_L, S, S), mk(B, min_L), mk(B, k * S, k * S), mk(B, k * S, k * S)
        binding.collate_device(lr, hr, sm, plan, S, lrs, alphas, hrs, maps, scale=scale, codes=torch.full((B,), code, dtype=torch.int32, device="cuda"))
        torch.cuda.synchronize()
        lrs, alphas, hrs, maps = (t.cpu().numpy() for t in (lrs, alphas, hrs, maps))
        eq = lambda got, want: np.array_equal(got, augment.apply(want, code))
        assert eq(lrs[0, 0], want_lr(v)) and not lrs[0, 1].any() and alphas[0].tolist() == [1, 0]
        assert eq(hrs[0], want_hr(0)) and eq(maps[0], want_sm(0))
        assert nan(lrs[1, 0]) and eq(lrs[1, 1], want_lr(0)) and eq(hrs[1], want_hr(1)) and eq(maps[1], want_sm(1))
        assert nan(lrs[2, 0]) and eq(lrs[2, 1], want_lr(3 * v))
        assert nan(hrs[3]) and eq(maps[3], want_sm(0)) and eq(lrs[3, 0], want_lr(2 * v))
        assert nan(maps[4]) and eq(hrs[4], want_hr(0)) and eq(lrs[4, 1], want_lr(v))
        for b in (5, 6, 7):
            assert nan(lrs[b]) and nan(hrs[b]) and nan(maps[b]), (code, b)
        assert alphas[1:].tolist() == [[1, 1]] * (B - 1)
    del keep_lr, keep_hr, keep_sm


def test_split_without_hr(sets, tmp_path):
    t = [write_imageset(str(tmp_path), f"imgset{9000 + i}", n, with_hr=False, seed=5 + i) for i, n in enumerate((4, 6))]
    ds = DL.ImagesetDataset(sets[3][:2] + t, {"create_patches": True, "patch_size": 64}, top_k=-1, augment="dihedral")
    cache = ds.to_device(n_threads=N_THREADS)
    for k, indices in enumerate(([2, 3], [0, 2], [1, 0], [3, 2, 1, 0])):
        host, dev = _both(ds, cache, indices, 8, seed=30 + k)
        _same(host, dev)
    assert isinstance(_both(ds, cache, [2, 3], 8)[1][2], list)
    # a sample without HR in a launch that has an HR plane keeps its zero plane, under a transposing code too
    np.random.seed(1)
    plan, _, S, _ = cache.index.plan([0, 1], 4)
    plan[1, 0] = -1
    got = _launch(cache, torch.from_numpy(plan).cuda(), S, 4, 3, [6, 5])
    assert not got[2][1].any() and got[2][0].any() and got[3][1].any()


def test_resampled_targets_with_augmentation(sets):
    """x3 files in a cache at scale 2 (resample_targets=True), augmentation on: the un-augmented cache's batch under the codes."""
    cfg = {"create_patches": True, "patch_size": 64, "scale": 2}
    plain = DL.ImagesetDataset(sets[3], cfg, top_k=5, beta=50.0).to_device(n_threads=N_THREADS, resample_targets=True)
    cache = DL.ImagesetDataset(sets[3], cfg, top_k=5, beta=50.0, augment="dihedral").to_device(n_threads=N_THREADS, resample_targets=True)
    np.random.seed(17)
    got = cache.load_batch([0, 1, 2, 3, 4, 5], 6)
    codes = cache.last_augment
    # the same views and corners without the extra draws: take the plan the augmented cache made and launch it without codes
    np.random.seed(17)
    plan, _, S, have_hr = cache.index.plan([0, 1, 2, 3, 4, 5], 6)
    want = _launch(plain, torch.from_numpy(plan).cuda(), S, 6, 2, None)
    assert len(set(codes)) >= 3 and got[2].shape == (6, 128, 128)
    for b, c in enumerate(codes):
        for g, w in zip((got[0], got[2], got[3]), (want[0], want[2], want[3])):
            assert torch.equal(g[b], augment.apply(w[b], c)), (b, c)
    assert torch.equal(got[1], want[1])


# ------------------------------------------------------------------ 4. end to end: five bf16 steps from an augmented cache
def test_five_bf16_steps_from_an_augmented_cache(tmp_path):
    """Plumbing only (no claim about accuracy): batches drawn from an augmented cache feed HRNet + ShiftNet in bf16, the
    registered loss and FusedAdam, in the pattern of test_gpu_scale_pipeline.py::test_x2_finetune_from_x3_data."""
    from DeepNetworks.HRNet import HRNet
    from DeepNetworks.ShiftNet import ShiftNet
    from hrnet_hip.losses import get_loss
    from hrnet_hip.optim import FusedAdam
    from oracle import weights

    g = np.random.Generator(np.random.PCG64(21))
    dirs = []
    for i in range(4):
        yy, xx = np.mgrid[0:384, 0:384] / 384.0
        ph = g.random(3)
        field = 0.35 + 0.2 * np.sin(2 * np.pi * (1.3 * xx + ph[0])) * np.cos(2 * np.pi * (0.9 * yy + ph[1])) + 0.1 * np.sin(2 * np.pi * (2.1 * (xx + yy) + ph[2]))
        hr = np.rint(field * 65535 * 0.25).astype(np.uint16)
        box = (field * 65535 * 0.25).reshape(128, 3, 128, 3).mean(axis=(1, 3))
        views = [np.clip(np.rint(box + 20.0 * g.standard_normal((128, 128))), 0, 65535).astype(np.uint16) for _ in range(5)]
        dirs.append(write_imageset(str(tmp_path), f"imgset{i:04d}", 5, lr_views=views, hr=hr, seed=60 + i))
    P = 64
    ds = DL.ImagesetDataset(dirs, {"create_patches": True, "patch_size": P, "augment": "dihedral"}, top_k=4, beta=50.0)
    cache = ds.to_device("cuda", n_threads=N_THREADS)

    torch.manual_seed(0)
    fusion = HRNet(weights.HRNET_CONFIG)
    fusion.load_state_dict(weights.to_torch_state(weights.hrnet_state(1234)))
    fusion.train_precision = "bf16"
    fusion = fusion.cuda().train()
    regis = ShiftNet(train_precision="bf16")
    regis.load_state_dict(weights.to_torch_state(weights.shiftnet_state(4321)))
    regis = regis.cuda().train()
    optimizer = FusedAdam([*fusion.parameters(), *regis.parameters()], lr=1e-4)
    offset = (3 * P - 128) // 2
    np.random.seed(5)
    losses, seen = [], set()
    for lrs, alphas, hrs, hr_maps, names in cache.batches([[0, 1, 2, 3]] * 5, 4):
        seen |= set(cache.last_augment)
        assert lrs.shape == (4, 4, P, P) and hrs.shape == hr_maps.shape == (4, 3 * P, 3 * P)
        optimizer.zero_grad()
        srs = fusion(lrs, alphas)
        assert tuple(srs.shape) == (4, 1, 3 * P, 3 * P)
        shifts = regis(torch.cat([hrs[:, offset:offset + 128, offset:offset + 128].reshape(-1, 1, 128, 128),
                                  srs[:, :, offset:offset + 128, offset:offset + 128]], 1))
        shifted = regis.transform(shifts.view(-1, 2), srs.view(-1, 1, 3 * P, 3 * P), device="cuda").view(-1, 1, 3 * P, 3 * P)[:, 0]
        loss = -get_loss(shifted, hrs, hr_maps, metric="cPSNR", crop=3).mean()
        loss.backward()
        optimizer.step()
        losses.append(float(loss.detach()))
    print("augmented bf16 steps, losses:", " ".join(f"{v:.4f}" for v in losses), "codes seen:", sorted(seen))
    assert len(losses) == 5 and all(np.isfinite(losses)) and len(seen) >= 4
