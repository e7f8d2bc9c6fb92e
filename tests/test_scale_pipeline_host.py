"""CPU: the input pipeline at target scales 2 and 4 (and 3 through the new entry points): ImagesetDataset / read_imageset
/ load_batch against a numpy restatement, bit for bit, from imagesets whose HR / SM files are stored at that ratio; the numpy
RNG contract across scales; the errors; and the fp64 reference of the target resampler (scale_ref.py) checked against its own
definition and against the weight table the product uploads (hrnet_hip/resample.py).  The device half is in
test_gpu_scale_pipeline.py."""
import ctypes
import os

import numpy as np
import pytest
import torch

import DataLoader as DL
from hrnet_hip import binding, build, io_binding, resample
from imageset_png import write_imageset
from scale_ref import PAIRS, field_image, ref_matrix, ref_resample_hr, restated_batch, restated_read, write_scaled_imageset

VIEWS = (4, 12, 7, 9)


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    """{ratio: four imagesets with HR and one without, HR / SM stored at that ratio; LR views and clearances do not depend on
    the ratio (the writer draws them first), so the three splits are comparable draw by draw}"""
    root = tmp_path_factory.mktemp("scaled")
    out = {}
    for ratio in (2, 3, 4):
        r = str(root / f"x{ratio}")
        os.makedirs(r)
        out[ratio] = [write_scaled_imageset(r, f"imgset{i:04d}", n, ratio, seed=10 + i) for i, n in enumerate(VIEWS)]
        out[ratio].append(write_scaled_imageset(r, "imgset0900", 5, ratio, with_hr=False, seed=19))
    return out


def _state_equal(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


@pytest.mark.parametrize("scale", [2, 4])
@pytest.mark.parametrize("create_patches,patch_size", [(True, 64), (True, 30), (False, 64)])
@pytest.mark.parametrize("top_k,beta,seed", [(-1, 0.0, None), (-1, 0.0, 5), (5, 50.0, 7), (5, 0.0, None), (40, 50.0, None)])
def test_host_batches_equal_the_numpy_restatement(sets, scale, create_patches, patch_size, top_k, beta, seed):
    dirs = sets[scale]
    cfg = {"create_patches": create_patches, "patch_size": patch_size, "scale": scale}
    ds = DL.ImagesetDataset(dirs, cfg, seed=seed, top_k=top_k, beta=beta)
    assert ds.scale == scale
    S = patch_size if create_patches else 128
    for indices, min_L in (([0, 1, 2, 3], 6), ([3, "imgset0001"], 16), ([4, 0], 8)):       # the last one has an imageset without HR
        picked = [dirs[i] if isinstance(i, int) else ds.name_to_dir[i] for i in indices]
        np.random.seed(31)
        want = restated_batch(picked, min_L, create_patches, patch_size, seed, top_k, beta, scale, io_binding.png_read)
        want_state = np.random.get_state()
        np.random.seed(31)
        got = ds.load_batch(indices, min_L, n_threads=3)
        assert _state_equal(np.random.get_state(), want_state)
        assert got[4] == want[4] and got[0].shape == (len(indices), min_L, S, S) and got[3].shape == (len(indices), scale * S, scale * S)
        for name, g, w in zip(("lrs", "alphas", "hrs", "maps"), got[:4], want[:4]):
            if isinstance(w, list):
                assert g == [] and w == [], name
            else:
                assert g.dtype == torch.float32 and np.array_equal(g.numpy(), w), name
    # __getitem__ and read_imageset, one labelled imageset and the one without HR
    for d in (dirs[1], dirs[4]):
        np.random.seed(32)
        want = restated_read(d, create_patches, patch_size, seed, top_k, beta, scale, io_binding.png_read)
        np.random.seed(32)
        item = ds[os.path.basename(d)]
        assert np.array_equal(item["lr"].numpy(), want["lr"]) and np.array_equal(item["clearances"], want["cl"])
        if want["hr"] is None:
            assert item["hr"] is None and item["hr_map"].dtype == bool and np.array_equal(item["hr_map"], want["sm"])
        else:
            assert np.array_equal(item["hr"].numpy(), want["hr"]) and np.array_equal(item["hr_map"].numpy(), want["sm"].astype(np.float32))
            assert tuple(item["hr"].shape) == (scale * S, scale * S)
        np.random.seed(32)
        ims = DL.read_imageset(d, create_patches=create_patches, patch_size=patch_size, seed=seed, top_k=top_k, beta=beta, scale=scale)
        assert np.array_equal(ims["lr"], want["lr_u16"]) and ims["hr_map"].dtype == bool and np.array_equal(ims["hr_map"], want["sm"])
        assert (ims["hr"] is None) if want["hr_u16"] is None else np.array_equal(ims["hr"], want["hr_u16"])


def test_scale_argument_and_config_key(sets):
    cfg = {"create_patches": True, "patch_size": 64}
    assert DL.ImagesetDataset(sets[3], cfg).scale == 3
    assert DL.ImagesetDataset(sets[2], dict(cfg, scale=2)).scale == 2
    assert DL.ImagesetDataset(sets[4], dict(cfg, scale=2), scale=4).scale == 4           # the argument wins over the config
    ds = DL.ImagesetDataset(sets[4], cfg, scale=4, seed=3)
    got = list(DL.BatchPrefetcher(ds, [[0, 1], [2]], min_L=5, device="cpu", depth=1))
    assert [tuple(b[2].shape) for b in got] == [(2, 256, 256), (1, 256, 256)] and tuple(got[0][3].shape) == (2, 256, 256)
    want = ds.load_batch([0, 1], 5)
    assert all(torch.equal(a, b) for a, b in zip(got[0][:4], want[:4]))


def _collate_args(dirs, views, min_L, lr_size, patch, corner, scale):
    """ctypes arguments of hrn_io_collate(_s) for `dirs`, their first `views` LR files each, and fresh output buffers."""
    B, S = len(dirs), patch if patch else lr_size
    flat = [os.fsencode(os.path.join(d, f"LR{v:03d}.png")) for d in dirs for v in range(views)]
    arr = lambda items: (ctypes.c_char_p * len(items))(*items)
    ints = lambda vals: (ctypes.c_int * len(vals))(*vals)
    bufs = [np.full(shape, 7.0, np.float32) for shape in ((B, min_L, S, S), (B, min_L), (B, scale * S, scale * S), (B, scale * S, scale * S))]
    ptrs = [b.ctypes.data_as(ctypes.c_void_p) for b in bufs]
    head = [B, arr(flat), ints([views] * B), arr([os.fsencode(os.path.join(d, "HR.png")) for d in dirs]),
            arr([os.fsencode(os.path.join(d, "SM.png")) for d in dirs]), min_L, lr_size, patch]
    tail = [ints([corner[0]] * B), ints([corner[1]] * B)] + ptrs + [2]
    return head, tail, bufs


@pytest.mark.parametrize("patch,corner", [(64, (17, 40)), (30, (98, 0)), (0, (0, 0))])
def test_io_collate_s_at_scale_3_is_io_collate(sets, patch, corner):
    lib = io_binding.load_library()
    dirs = sets[3][:3]
    head, tail, old = _collate_args(dirs, 4, 6, 128, patch, corner, 3)
    assert lib.hrn_io_collate(*head, *tail) == 0
    head, tail, new = _collate_args(dirs, 4, 6, 128, patch, corner, 3)
    assert lib.hrn_io_collate_s(*head, 3, *tail) == 0
    for a, b in zip(old, new):
        assert not (a == 7.0).all() and a.tobytes() == b.tobytes()
    # and the Python wrapper's default is that call
    S = patch if patch else 128
    out = io_binding.collate([[os.path.join(d, f"LR{v:03d}.png") for v in range(4)] for d in dirs], [os.path.join(d, "HR.png") for d in dirs],
                             [os.path.join(d, "SM.png") for d in dirs], min_L=6, lr_size=128, patch=patch, corners=[corner] * 3, n_threads=2)
    assert out["hrs"].shape == (3, 3 * S, 3 * S) and all(out[k].tobytes() == b.tobytes() for k, b in zip(("lrs", "alphas", "hrs", "maps"), old))


@pytest.mark.parametrize("create_patches", [True, False])
@pytest.mark.parametrize("top_k,beta", [(-1, 0.0), (3, 50.0), (40, 0.0)])
@pytest.mark.parametrize("seed", [None, 13])
def test_rng_contract_is_the_same_at_every_scale(sets, create_patches, top_k, beta, seed):
    """Same seed -> same views, same LR corner, same global RNG state afterwards at scale 2, 3 and 4, on the host path and in
    ImagesetIndex.plan."""
    order, min_L = [1, 0, 3, 1, 4, 2, 0], 6
    corners, states = {}, {}
    for scale in (2, 3, 4):
        dirs = sets[scale]
        ds = DL.ImagesetDataset(dirs, {"create_patches": create_patches, "patch_size": 32, "scale": scale}, seed=seed, top_k=top_k, beta=beta)
        np.random.seed(2024)
        host = [ds._plan(dirs[i]) for i in order]
        states[scale] = np.random.get_state()
        corners[scale] = [(h["corner"], [os.path.basename(p) for p in h["lr_paths"]]) for h in host]
        np.random.seed(2024)
        ds.load_batch([1, 0, 3, 1], min_L)
        after_batch = np.random.get_state()
        np.random.seed(2024)
        [ds._plan(dirs[i]) for i in [1, 0, 3, 1]]
        assert _state_equal(after_batch, np.random.get_state())
        # the planner of the device cache makes the same draws
        index = DL.ImagesetIndex(ds)
        assert index.scale == scale and index.ratios == [scale] * 5
        assert index.hr_elems == 4 * scale * scale * 128 * 128 and index.sm_elems == 5 * scale * scale * 128 * 128
        np.random.seed(2024)
        plan, names, S, have_hr = index.plan(order, min_L)
        assert _state_equal(np.random.get_state(), states[scale])
        assert names == [h["name"] for h in host] and S == (32 if create_patches else 128) and not have_hr
        M = binding.COLLATE_META
        for b, (i, h) in enumerate(zip(order, host)):
            ids = list(index.ids[i])
            want_off = [int(index.lr_off[i][ids.index(os.path.basename(p)[2:-4])]) for p in h["lr_paths"]][:min_L]
            assert plan[b, M:M + len(want_off)].tolist() == want_off and (plan[b, M + len(want_off):] == -1).all()
            assert plan[b, :M].tolist() == [-1, index.sm_off[i], 128, *(h["corner"] if create_patches else (0, 0))]
    assert corners[2] == corners[3] == corners[4]
    assert _state_equal(states[2], states[3]) and _state_equal(states[4], states[3])


def test_ratio_mismatch_and_bad_scales_raise(sets, tmp_path):
    cfg = {"create_patches": True, "patch_size": 64}
    for bad in (0, 1, 5, 2.0, "3", True):
        with pytest.raises(ValueError, match="2, 3 or 4"):
            DL.ImagesetDataset(sets[3], cfg, scale=bad)
        with pytest.raises(ValueError, match="2, 3 or 4"):
            DL.read_imageset(sets[3][0], scale=bad)
    for bad in (0, 1, 5):
        with pytest.raises(ValueError, match="2, 3 or 4"):
            DL.ImagesetDataset(sets[3], dict(cfg, scale=bad))
        with pytest.raises(ValueError, match="2, 3 or 4"):
            io_binding.collate([[os.path.join(sets[3][0], "LR000.png")]], None, [os.path.join(sets[3][0], "SM.png")], min_L=1, lr_size=128, scale=bad)
    # x3 files at scale 2 / 4, and x2 files at the default scale: ValueError that names the imageset, both sides and the way out
    for dirs, scale, found in ((sets[3], 2, 384), (sets[3], 4, 384), (sets[2], 3, 256)):
        ds = DL.ImagesetDataset(dirs, cfg, scale=scale, seed=1)
        for call in (lambda: ds.load_batch([0, 1], 4), lambda: ds[1], lambda: ds[4], lambda: DL.ImagesetIndex(ds),
                     lambda: DL.read_imageset(dirs[1], create_patches=True, scale=scale), lambda: DL.read_imageset(dirs[1], scale=scale)):
            with pytest.raises(ValueError) as e:
                call()
            msg = str(e.value)
            assert "imgset" in msg and str(found) in msg and str(scale * 128) in msg and "resample_targets=True" in msg, msg
        with pytest.raises(ValueError, match="imgset0001"):
            ds.load_batch([1], 4)
    # a mixed split names the imageset that does not fit, and with resample_targets the index records each stored ratio
    mixed = [sets[2][0], sets[3][1], sets[2][2], sets[4][3]]
    ds = DL.ImagesetDataset(mixed, cfg, scale=2)
    with pytest.raises(ValueError, match="imgset0001"):
        ds.load_batch([0, 1, 2], 4)
    with pytest.raises(ValueError, match="imgset0001"):
        DL.ImagesetIndex(ds)
    index = DL.ImagesetIndex(ds, resample_targets=True)
    assert index.ratios == [2, 3, 2, 4] and index.hr_elems == 4 * 4 * 128 * 128 and index.sm_elems == 4 * 4 * 128 * 128
    # a failure that is not a ratio mismatch stays what it was
    broken = write_scaled_imageset(str(tmp_path), "imgset0777", 3, 2, seed=1)
    os.remove(os.path.join(broken, "LR001.png"))
    with pytest.raises(io_binding.HrnetIoError, match="LR001"):
        DL.ImagesetDataset([broken], cfg, scale=2).load_batch([0], 4)
    # HR / SM that are no multiple of 2, 3, 4 of the LR side cannot be resampled either
    odd = write_imageset(str(tmp_path), "imgset0778", 3, lr=64, seed=2)
    from imageset_png import write_png
    write_png(os.path.join(odd, "SM.png"), np.ones((100, 100), np.uint8))
    with pytest.raises(ValueError, match="imgset0778"):
        DL.ImagesetIndex(DL.ImagesetDataset([odd], cfg, scale=2), resample_targets=True)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(binding.LIB_PATH):
        build.build_library(verbose=False)
    return binding.load_library()


def test_s_entry_points_refuse_a_bad_scale_without_touching_a_buffer(sets, lib):
    io = io_binding.load_library()
    for bad in (0, 1, 5, -3):
        head, tail, bufs = _collate_args(sets[3][:2], 4, 6, 128, 64, (3, 4), 3)
        assert io.hrn_io_collate_s(*head, bad, *tail) == -2 and b"scale" in io.hrn_io_last_error()
        assert all((b == 7.0).all() for b in bufs)
    null = ctypes.c_void_p(0)
    p = ctypes.c_void_p(4096)                       # never dereferenced: every call below is refused on the host
    for bad in (0, 1, 5, -3):
        assert lib.hrn_adam_step(null, null, null, null, 4, 0.1, 0.9, 0.99, 1e-8, 0.0, 1, null) == -2      # leaves another message
        assert lib.hrn_collate_device_s(p, 64, p, 64, p, 64, p, 2, 3, 8, bad, p, p, p, p, null) == -2
        msg = lib.hrn_last_error()
        assert msg.startswith(b"hrn_collate_device") and b"scale" in msg, msg
    for kw, word in [(dict(B=0), b"B"), (dict(S=0), b"S"), (dict(lr_n=6), b"multiples of 4"), (dict(plan=null), b"null")]:
        a = dict(dict(lr_n=64, B=2, S=8, plan=p), **kw)
        for scale in (2, 3, 4):
            assert lib.hrn_collate_device_s(p, a["lr_n"], p, 64, p, 64, a["plan"], a["B"], 3, a["S"], scale, p, p, p, p, null) == -2
            assert word in lib.hrn_last_error()


def test_resample_entry_point_refuses_bad_arguments_before_any_launch(lib):
    null = ctypes.c_void_p(0)
    p = ctypes.c_void_p(4096)
    good = dict(src=p, src_n=1 << 20, dst=p, dst_n=1 << 20, eb=2, jobs=p, n_jobs=3, n_in=384, n_out=256, first=p, count=p, w=p)

    def call(**kw):
        a = dict(good, **kw)
        return lib.hrn_resample_targets(a["src"], a["src_n"], a["dst"], a["dst_n"], a["eb"], a["jobs"], a["n_jobs"], a["n_in"], a["n_out"],
                                        a["first"], a["count"], a["w"], null)

    for kw, word in [(dict(src=null), b"null"), (dict(dst=null), b"null"), (dict(jobs=null), b"null"), (dict(first=null), b"null"),
                     (dict(count=null), b"null"), (dict(w=null), b"null"), (dict(eb=4), b"elem_bytes"), (dict(eb=0), b"elem_bytes"),
                     (dict(n_jobs=0), b"n_jobs"), (dict(n_jobs=70000), b"n_jobs"), (dict(n_in=0), b"n_in"), (dict(n_out=-4), b"n_in"),
                     (dict(n_in=384, n_out=100), b"R : S"), (dict(n_in=500, n_out=100), b"R : S"), (dict(src_n=100), b"less than one image"),
                     (dict(dst_n=0), b"less than one image"), (dict(src=ctypes.c_void_p(4097)), b"misaligned"),
                     (dict(w=ctypes.c_void_p(4100)), b"misaligned")]:
        assert lib.hrn_adam_step(null, null, null, null, 4, 0.1, 0.9, 0.99, 1e-8, 0.0, 1, null) == -2
        assert call(**kw) == -2, kw
        msg = lib.hrn_last_error()
        assert msg.startswith(b"hrn_resample_targets") and word in msg, (kw, msg)
    assert binding.RESAMPLE_TAPS == resample.MAX_TAPS == 12
    # the Python wrapper checks its tensors first (no device here: a host tensor is refused)
    with pytest.raises(RuntimeError, match="device tensor"):
        binding.resample_targets(torch.zeros(16, dtype=torch.uint8), torch.zeros(16, dtype=torch.uint8), [[0, 0]], 4, 4, None)


# ------------------------------------------------------------------ the resampler's reference checks itself
SIDE = 128


@pytest.mark.parametrize("R,scale", PAIRS)
def test_reference_weights_and_the_uploaded_table(R, scale):
    A = ref_matrix(SIDE, R, scale)
    n_in, n_out = R * SIDE, scale * SIDE
    assert A.shape == (n_out, n_in)
    assert np.abs(A.sum(axis=1) - 1.0).max() <= 1e-15
    taps = (A != 0).sum(axis=1)
    assert taps.max() <= 12 and taps.min() >= 3 and np.abs(A).sum(axis=1).max() <= 1.55
    want_taps = {(2, 3): 6, (2, 4): 6, (3, 2): 9, (3, 4): 6, (4, 2): 12, (4, 3): 8}[R, scale]
    assert taps.max() == want_taps
    # the table the product uploads: the same weights, bit for bit, and nothing outside it
    first, count, weights = resample.weight_table(SIDE, R, scale)
    assert first.dtype == np.int32 and count.dtype == np.int32 and weights.dtype == np.float64 and weights.shape == (n_out, 12)
    dense = np.zeros_like(A)
    for j in range(n_out):
        assert np.all(weights[j, count[j]:] == 0)
        dense[j, first[j]:first[j] + count[j]] = weights[j, :count[j]]
    assert dense.tobytes() == A.tobytes()
    assert (count == taps).all()


@pytest.mark.parametrize("R,scale", PAIRS)
def test_reference_constant_separable_and_clip(R, scale):
    n_in, n_out = R * SIDE, scale * SIDE
    for c in (0, 1, 777, 40000, 65535):
        got, _ = ref_resample_hr(np.full((n_in, n_in), c, np.uint16), SIDE, R, scale)
        assert got.shape == (n_out, n_out) and (got == c).all(), c
    u = field_image(n_in, seed=10 * R + scale)
    got, v = ref_resample_hr(u, SIDE, R, scale)
    # separable form from the product's table (rows, then columns) against the dense A U A^T
    first, count, weights = resample.weight_table(SIDE, R, scale)
    uf = u.astype(np.float64)
    rows = np.zeros((n_out, n_in))
    for t in range(12):
        on = t < count
        rows[on] += weights[on, t, None] * uf[first[on] + t]
    sep = np.zeros((n_out, n_out))
    for t in range(12):
        on = t < count
        sep[:, on] += weights[on, t] * rows[:, first[on] + t]
    assert np.abs(sep - v).max() <= 1e-6                              # codes; 144 products of <= 1.6e5 each: see the GPU test
    assert ((v < 0).sum() > 0) and ((v > 65535).sum() > 0)            # the clip acts at both ends
    assert got.min() == 0 and got.max() == 65535


@pytest.mark.parametrize("k", [2, 3, 4])
def test_reference_is_the_identity_when_the_ratios_agree(k):
    u = field_image(k * 64, seed=k)
    got, _ = ref_resample_hr(u, 64, k, k)
    assert np.array_equal(got, u)
    first, count, weights = resample.weight_table(64, k, k)
    assert count.max() <= 6 and np.abs(weights.sum(axis=1) - 1).max() <= 1e-15
    with pytest.raises(ValueError, match="2, 3 or 4"):
        resample.weight_table(64, 5, 2)
    with pytest.raises(ValueError, match="2, 3 or 4"):
        resample.weight_table(64, 3, 1)
