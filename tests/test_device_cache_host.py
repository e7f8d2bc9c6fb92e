"""CPU: the host half of the HBM-resident input pipeline (DataLoader.DeviceImagesetCache; include/hrnet_io.h,
include/hrnet_hip.h): the bulk PNG decoder, the batch planner's numpy RNG contract, and hrn_collate_device's argument checks,
which fail before any launch.  The device half is pinned in test_gpu_device_cache.py."""
import ctypes
import os

import numpy as np
import pytest
import torch

import DataLoader as DL
from hrnet_hip import binding, build, io_binding
from imageset_png import write_imageset, write_png


def test_read_many_is_bit_exact_and_names_a_bad_file(tmp_path):
    rng = np.random.Generator(np.random.PCG64(5))
    imgs = [rng.integers(0, 65536, (37, 53), dtype=np.uint16), rng.integers(0, 256, (40, 33), dtype=np.uint8),
            rng.integers(0, 65536, (1, 1), dtype=np.uint16), rng.integers(0, 256, (7, 129), dtype=np.uint8),
            (np.add.outer(np.arange(64), np.arange(80)) * 257 % 65536).astype(np.uint16)]
    paths = []
    for i, a in enumerate(imgs):
        paths.append(str(tmp_path / f"img{i}.png"))
        write_png(paths[-1], a, level=i % 10)
    sizes = [a.size for a in imgs]
    offsets = np.concatenate([[3], 3 + np.cumsum([s + 2 for s in sizes[:-1]])])      # gaps between images must stay untouched
    arena = np.full(int(offsets[-1]) + sizes[-1] + 5, 0xBEEF, np.uint16)
    io_binding.read_many(paths, arena, offsets, [a.shape[1] for a in imgs], [a.shape[0] for a in imgs], n_threads=3)
    touched = np.zeros(arena.size, bool)
    for p, a, o in zip(paths, imgs, offsets):
        got = arena[o:o + a.size].reshape(a.shape)
        assert np.array_equal(got, io_binding.png_read(p)) and np.array_equal(got, a.astype(np.uint16))
        touched[o:o + a.size] = True
    assert (arena[~touched] == 0xBEEF).all()
    # a missing file: negative status, and the message names it
    lib = io_binding.load_library()
    bad = [paths[0], str(tmp_path / "nope.png"), paths[1]]
    arr = (ctypes.c_char_p * 3)(*[os.fsencode(p) for p in bad])
    off = (ctypes.c_int64 * 3)(0, 37 * 53, 2 * 37 * 53)
    w = (ctypes.c_int * 3)(53, 53, 33)
    h = (ctypes.c_int * 3)(37, 37, 40)
    buf = np.zeros(4 * 37 * 53, np.uint16)
    rc = lib.hrn_io_read_many_u16(3, arr, buf.ctypes.data_as(ctypes.c_void_p), off, w, h, 2)
    assert rc < 0 and b"nope.png" in lib.hrn_io_last_error()
    with pytest.raises(io_binding.HrnetIoError, match="nope.png"):
        io_binding.read_many(bad, buf, [0, 37 * 53, 2 * 37 * 53], [53, 53, 33], [37, 37, 40], n_threads=2)
    # a size that does not match the file is an error too
    with pytest.raises(io_binding.HrnetIoError, match="expected"):
        io_binding.read_many(paths[:1], buf, [0], [52], [37], n_threads=1)
    assert lib.hrn_io_read_many_u16(0, arr, buf.ctypes.data_as(ctypes.c_void_p), off, w, h, 1) == -2


@pytest.fixture(scope="module")
def imagesets(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("sets"))
    return [write_imageset(root, f"imgset{i:04d}", n, lr=96, with_hr=i != 2, seed=40 + i) for i, n in enumerate((4, 12, 7, 9, 5))]


@pytest.mark.parametrize("create_patches", [True, False])
@pytest.mark.parametrize("top_k", [-1, 3, 40])
@pytest.mark.parametrize("beta", [0.0, 50.0])
@pytest.mark.parametrize("seed", [None, 13])
def test_plan_makes_the_host_paths_rng_calls(imagesets, create_patches, top_k, beta, seed):
    """Over a sequence of imagesets the planner leaves numpy's global RNG exactly where ImagesetDataset._plan leaves it, and
    picks the same views and the same patch corner."""
    ds = DL.ImagesetDataset(imagesets, {"create_patches": create_patches, "patch_size": 32}, seed=seed, top_k=top_k, beta=beta)
    index = DL.ImagesetIndex(ds)
    order = [1, 0, 3, 1, 4, 2, 0]
    np.random.seed(2024)
    host = [ds._plan(imagesets[i]) for i in order]
    want_state = np.random.get_state()
    np.random.seed(2024)
    min_L = 6
    plan, names, S, have_hr = index.plan(order, min_L)
    got_state = np.random.get_state()
    assert got_state[0] == want_state[0] and np.array_equal(got_state[1], want_state[1]) and got_state[2:] == want_state[2:]
    assert names == [h["name"] for h in host] and S == (32 if create_patches else 96) and not have_hr
    M = binding.COLLATE_META
    for b, (i, h) in enumerate(zip(order, host)):
        ids = list(index.ids[i])
        want_off = [int(index.lr_off[i][ids.index(os.path.basename(p)[2:-4])]) for p in h["lr_paths"]][:min_L]
        assert plan[b, M:M + len(want_off)].tolist() == want_off and (plan[b, M + len(want_off):] == -1).all()
        row, col = h["corner"] if create_patches else (0, 0)
        assert plan[b, :M].tolist() == [-1, index.sm_off[i], 96, row, col]          # imageset 2 has no HR: no HR plane at all
    # a batch whose imagesets all have HR.png keeps their HR offsets
    np.random.seed(1)
    plan, _, _, have_hr = index.plan([0, 1], min_L)
    assert have_hr and plan[:, 0].tolist() == [index.hr_off[0], index.hr_off[1]]


def test_index_layout_and_errors(imagesets, tmp_path):
    ds = DL.ImagesetDataset(imagesets, {"create_patches": True, "patch_size": 32}, top_k=-1)
    index = DL.ImagesetIndex(ds)
    assert len(index) == 5 and index.lr_elems == 96 * 96 * (4 + 12 + 7 + 9 + 5)
    assert index.hr_elems == 4 * 9 * 96 * 96 and index.sm_elems == 5 * 9 * 96 * 96
    assert all(o % 4 == 0 for offs in index.lr_off for o in offs)
    assert index.resolve("imgset0003") == 3 and index.resolve(-1) == 4
    with pytest.raises(KeyError):
        index.plan([0, "imgset9999"], 4)
    odd = write_imageset(str(tmp_path), "imgset0100", 3, lr=64, seed=1)
    ds2 = DL.ImagesetDataset(imagesets + [odd], {"create_patches": True, "patch_size": 32}, top_k=-1)
    with pytest.raises(ValueError, match="share the LR size"):
        DL.ImagesetIndex(ds2).plan([0, 5], 4)
    with pytest.raises(ValueError, match="share the LR size"):
        ds2.load_batch([0, 5], 4)
    with pytest.raises(ValueError, match="ROCm device"):
        ds.to_device("cpu")
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no GPU"):
            ds.to_device("cuda")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(binding.LIB_PATH):
        build.build_library(verbose=False)
    return binding.load_library()


def test_collate_device_bad_arguments_fail_before_any_launch(lib):
    null = ctypes.c_void_p(0)
    p = ctypes.c_void_p(4096)                       # never dereferenced: every call below is refused on the host
    good = dict(lr=p, lr_n=64, hr=p, hr_n=64, sm=p, sm_n=64, plan=p, B=2, min_L=3, S=8, lrs=p, alphas=p, hrs=p, maps=p)

    def call(**kw):
        a = dict(good, **kw)
        return lib.hrn_collate_device(a["lr"], a["lr_n"], a["hr"], a["hr_n"], a["sm"], a["sm_n"], a["plan"], a["B"], a["min_L"], a["S"],
                                      a["lrs"], a["alphas"], a["hrs"], a["maps"], null)

    for kw, word in [(dict(lr=null), b"null"), (dict(sm=null), b"null"), (dict(plan=null), b"null"), (dict(lrs=null), b"null"),
                     (dict(alphas=null), b"null"), (dict(maps=null), b"null"), (dict(hr=null), b"HR arena"),
                     (dict(B=0), b"B"), (dict(B=-1), b"B"), (dict(min_L=0), b"min_L"), (dict(min_L=-2), b"min_L"),
                     (dict(S=0), b"S"), (dict(S=-8), b"S"), (dict(lr_n=6), b"multiples of 4"), (dict(sm_n=0), b"multiples of 4"),
                     (dict(lr=ctypes.c_void_p(4098)), b"aligned")]:
        assert lib.hrn_adam_step(null, null, null, null, 4, 0.1, 0.9, 0.99, 1e-8, 0.0, 1, null) == -2      # leaves another message
        assert call(**kw) == -2, kw
        msg = lib.hrn_last_error()
        assert msg.startswith(b"hrn_collate_device") and word in msg, (kw, msg)
