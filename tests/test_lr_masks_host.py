"""CPU: the LR quality masks on the host path.  load_batch with `lr_masks` on against the numpy restatement of lr_masks_ref.py over
patches / top_k / beta / augmentation / scale / padding and truncation, with the switch leaving every other output and the RNG as
they were; items and shapes; a missing and a mis-sized QM file; hrn_io_collate_m's argument check; save_clearance_scores; the QM
arena of ImagesetIndex; and the fp64 restatement of the registration search on the scenes the GPU test registers."""
import ctypes
import os

import numpy as np
import pytest
import torch

import DataLoader as DL
import lr_masks_ref as ref
import registration_ref
from hrnet_hip import io_binding
from imageset_png import write_png

N_THREADS = 4
LR_SIDE = 72                                      # the smallest comfortable side above the 64-pixel patch


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    """{scale: six imagesets of LR side 72 with HR / SM stored at that ratio and quality maps of {0, 1, 128, 255}}"""
    root = tmp_path_factory.mktemp("lr_masks_host")
    return {k: ref.write_sets(str(root / f"x{k}"), k, lr=LR_SIDE) for k in (2, 3, 4)}


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def _check_batch(dirs, cfg, indices, min_L, rng_seed, **kw):
    """One batch with the switch on: masks against the restatement, everything else and the RNG against the switch off."""
    on, off = DL.ImagesetDataset(dirs, cfg, lr_masks=True, **kw), DL.ImagesetDataset(dirs, cfg, lr_masks=False, **kw)
    assert on.lr_masks is True and off.lr_masks is False
    np.random.seed(rng_seed)
    got = on.load_batch(indices, min_L, n_threads=N_THREADS)
    state = np.random.get_state()
    np.random.seed(rng_seed)
    plain = off.load_batch(indices, min_L, n_threads=N_THREADS)
    assert _same_state(state, np.random.get_state())
    assert len(got) == 6 and len(plain) == 5 and got[4] == plain[4] and on.last_augment == off.last_augment
    for g, p in zip(got[:4], plain[:4]):
        assert torch.equal(g, p) if isinstance(p, torch.Tensor) else g == p == []
    np.random.seed(rng_seed)
    want = ref.restated_masks(on, indices, min_L, on.last_augment)
    assert _same_state(state, np.random.get_state())
    masks = got[5]
    assert masks.dtype == torch.float32 and masks.shape == got[0].shape and np.array_equal(masks.numpy(), want)
    assert not masks[got[1] == 0].any()                                          # padding slots (alpha 0) are zeros
    return masks, got[1]


@pytest.mark.parametrize("augment", [None, "flip", "dihedral"])
@pytest.mark.parametrize("top_k", [-1, 5, 40])
@pytest.mark.parametrize("beta", [0.0, 50.0])
@pytest.mark.parametrize("create_patches,patch_size", [(True, 30), (True, 64), (False, 64)])
def test_load_batch_masks_equal_the_restatement(sets, create_patches, patch_size, top_k, beta, augment):
    """Every scale; min_L = 6 pads imageset 0 (4 views), min_L = 3 truncates every imageset."""
    seen = set()
    for k, scale in enumerate((2, 3, 4)):
        cfg = {"create_patches": create_patches, "patch_size": patch_size, "scale": scale}
        for j, (indices, min_L) in enumerate((([0, 1, 2, 3], 6), ([5, 0, "imgset0003", 4], 3))):
            masks, alphas = _check_batch(sets[scale], cfg, indices, min_L, 11 + 7 * k + j, top_k=top_k, beta=beta, augment=augment)
            S = patch_size if create_patches else LR_SIDE
            assert masks.shape == (4, min_L, S, S)
            assert (alphas[0].tolist() == [1, 1, 1, 1, 0, 0]) if min_L == 6 else bool(alphas.all())
            seen |= set(np.unique(masks.numpy()).tolist())
    assert seen == {0.0, 1.0}


def test_a_seeded_dataset_and_the_config_key(sets):
    cfg = {"create_patches": True, "patch_size": 30, "lr_masks": True, "augment": "dihedral"}
    _check_batch(sets[3], cfg, [0, 1, 2], 5, 3, seed=5, top_k=5, beta=50.0)
    assert DL.ImagesetDataset(sets[3], cfg).lr_masks is True and DL.ImagesetDataset(sets[3], cfg, lr_masks=False).lr_masks is False
    assert DL.ImagesetDataset(sets[3], {"create_patches": True, "patch_size": 30}).lr_masks is False


def test_stored_values_other_than_255_count_as_clear(sets):
    d = sets[3][0]
    stored = np.stack([io_binding.png_read(os.path.join(d, f"QM{v:03d}.png")) for v in range(4)])
    assert set(np.unique(stored).tolist()) == {0, 1, 128, 255}
    ds = DL.ImagesetDataset([d], {"create_patches": False, "patch_size": 0}, top_k=-1, lr_masks=True)
    masks = ds.load_batch([0], 4)[5].numpy()[0]
    order = np.flip(np.argsort(np.load(os.path.join(d, "clearance.npy"))))
    assert np.array_equal(masks, (stored[order] != 0).astype(np.float32)) and masks[stored[order] == 1].all()


def test_items_and_shapes(sets):
    d = sets[3][1]
    for create_patches, S in ((True, 30), (False, LR_SIDE)):
        np.random.seed(4)
        a = DL.read_imageset(d, create_patches, 30, top_k=5, beta=50.0, augment="dihedral", lr_masks=True)
        assert list(a)[-2:] == ["clearances", "lr_maps"] and a["lr_maps"].dtype == bool and a["lr_maps"].shape == a["lr"].shape == (5, S, S)
        np.random.seed(4)
        b = DL.read_imageset(d, create_patches, 30, top_k=5, beta=50.0, augment="dihedral")
        assert "lr_maps" not in b and np.array_equal(a["lr"], b["lr"]) and np.array_equal(a["hr_map"], b["hr_map"])
        cfg = {"create_patches": create_patches, "patch_size": 30, "augment": "dihedral"}
        np.random.seed(4)
        item = DL.ImagesetDataset(sets[3], cfg, top_k=5, beta=50.0, lr_masks=True)[1]
        assert item["lr_maps"].dtype == torch.float32 and tuple(item["lr_maps"].shape) == (5, S, S)
        assert np.array_equal(item["lr_maps"].numpy(), a["lr_maps"].astype(np.float32))          # the two readers agree
        off = DL.ImagesetDataset(sets[3], cfg, top_k=5, beta=50.0)
        assert "lr_maps" not in off[1] and len(off.load_batch([0, 1], 4)) == 5
    from utils import collateFunction
    ds = DL.ImagesetDataset(sets[3], {"create_patches": True, "patch_size": 30}, top_k=5, lr_masks=True)
    assert len(collateFunction(min_L=4)([ds[0], ds[1]])) == 5                    # the collate function ignores the key


def _copy_set(src, dst):
    os.makedirs(dst)
    for name in os.listdir(src):
        with open(os.path.join(src, name), "rb") as f, open(os.path.join(dst, name), "wb") as g:
            g.write(f.read())
    return dst


def test_a_missing_or_mis_sized_qm_file_is_an_error_that_names_it(sets, tmp_path):
    cfg = {"create_patches": True, "patch_size": 30}
    d = _copy_set(sets[3][0], str(tmp_path / "imgset0000"))
    qm = os.path.join(d, "QM002.png")
    write_png(qm, np.full((LR_SIDE, LR_SIDE - 1), 255, np.uint8))
    for attempt in (lambda: DL.ImagesetDataset([d], cfg, lr_masks=True).load_batch([0], 4), lambda: DL.ImagesetDataset([d], cfg, lr_masks=True)[0],
                    lambda: DL.read_imageset(d, lr_masks=True), lambda: DL.ImagesetIndex(DL.ImagesetDataset([d], cfg, lr_masks=True)) and
                    io_binding.read_many([qm], np.zeros(LR_SIDE * LR_SIDE, np.uint16), [0], [LR_SIDE], [LR_SIDE])):
        with pytest.raises(Exception, match="QM002.png"):
            attempt()
    # a view is listed by its QM file, so one can only be missing if it goes between the listing and the decode: the native collate names it
    lr = [os.path.join(d, f"LR{v:03d}.png") for v in (0, 3)]
    with pytest.raises(io_binding.HrnetIoError, match="QM777.png"):
        io_binding.collate([lr], None, [os.path.join(d, "SM.png")], 2, LR_SIDE,
                           qm_paths_per_set=[[os.path.join(d, "QM000.png"), os.path.join(d, "QM777.png")]])
    with pytest.raises(io_binding.HrnetIoError, match="QM777.png"):
        io_binding.png_read(os.path.join(d, "QM777.png"))                        # what read_imageset decodes a mask with
    # with the switch off nothing looks at the QM files' contents
    assert len(DL.ImagesetDataset([d], cfg).load_batch([0], 4)) == 5


def test_collate_m_with_one_of_the_two_pointers_null_touches_nothing(sets):
    lib = io_binding.load_library()
    d = sets[3][0]
    B, min_L, S, k = 1, 2, LR_SIDE, 3
    views = [os.path.join(d, f"LR{v:03d}.png") for v in range(2)]
    qms = [os.path.join(d, f"QM{v:03d}.png") for v in range(2)]
    bufs = {n: np.full(shape, 7.0, np.float32) for n, shape in (("lrs", (B, min_L, S, S)), ("alphas", (B, min_L)), ("hrs", (B, k * S, k * S)),
                                                                 ("maps", (B, k * S, k * S)), ("lr_masks", (B, min_L, S, S)))}
    p = lambda n: bufs[n].ctypes.data_as(ctypes.c_void_p)
    nv = (ctypes.c_int * 1)(2)
    call = lambda qm, masks: lib.hrn_io_collate_m(B, io_binding._strs(views), nv, io_binding._strs([os.path.join(d, "HR.png")]),
                                                  io_binding._strs([os.path.join(d, "SM.png")]), min_L, S, 0, k, None, None, p("lrs"), p("alphas"),
                                                  p("hrs"), p("maps"), 2, None, qm, masks)
    for qm, masks in ((io_binding._strs(qms), None), (None, p("lr_masks"))):
        assert call(qm, masks) == -2 and b"lr_masks" in lib.hrn_io_last_error()
        assert all((b == 7.0).all() for b in bufs.values())
    assert call(io_binding._strs(qms), p("lr_masks")) == 0
    want = np.stack([io_binding.png_read(q) != 0 for q in qms]).astype(np.float32)
    assert np.array_equal(bufs["lr_masks"][0], want)
    both_null = {n: b.copy() for n, b in bufs.items()}
    assert call(None, None) == 0 and all(np.array_equal(bufs[n], both_null[n]) for n in bufs)      # hrn_io_collate_a: the same four outputs


def test_save_clearance_scores(sets, tmp_path):
    dirs = [_copy_set(sets[3][i], str(tmp_path / f"imgset{i:04d}")) for i in (0, 1)]
    for d in dirs:
        os.remove(os.path.join(d, "clearance.npy"))
    cfg = {"create_patches": True, "patch_size": 30}
    with pytest.raises(Exception, match="save_clearance"):
        DL.ImagesetDataset(dirs, cfg)[0]
    saved = DL.save_clearance_scores(dirs)
    for d, s in zip(dirs, saved):
        names = sorted(n for n in os.listdir(d) if n.startswith("QM"))
        want = np.array([io_binding.png_read(os.path.join(d, q)).astype(np.uint16) for q in names]).sum(axis=(1, 2))
        got = np.load(os.path.join(d, "clearance.npy"))
        assert got.dtype == want.dtype == np.uint64 and np.array_equal(got, want) and np.array_equal(s, want)
    ds = DL.ImagesetDataset(dirs, cfg, lr_masks=True)
    assert tuple(ds[0]["lr"].shape) == (4, 30, 30) and len(ds.load_batch([0, 1], 4)) == 6


def test_the_index_reports_a_qm_arena_of_the_lr_arenas_size(sets):
    cfg = {"create_patches": True, "patch_size": 30}
    on = DL.ImagesetIndex(DL.ImagesetDataset(sets[3], cfg, lr_masks=True))
    off = DL.ImagesetIndex(DL.ImagesetDataset(sets[3], cfg))
    assert on.qm_elems == on.lr_elems == sum(ref.VIEWS) * LR_SIDE * LR_SIDE and off.qm_elems == 0 and off.lr_elems == on.lr_elems


def test_the_restated_search_recovers_the_shifts_of_the_registration_scenes(tmp_path):
    """What test_gpu_lr_masks.py asks of the device, asked of the fp64 restatement alone first: the masks and views as the host path
    delivers them, P = 7, 5 levels, radius 1, the known shifts relative to the clearest view within the 0.02 px of DESIGN 7f."""
    dirs, wanted = ref.write_registration_sets(str(tmp_path / "reg"))
    ds = DL.ImagesetDataset(dirs, {"create_patches": False, "patch_size": 0}, top_k=-1, lr_masks=True)
    lrs, alphas, _, _, _, masks = ds.load_batch([0, 1], ref.REG_VIEWS, n_threads=N_THREADS)
    lrs, masks = lrs.numpy(), masks.numpy()
    assert lrs.shape == masks.shape == (ref.REG_SETS, ref.REG_VIEWS, ref.REG_SIDE, ref.REG_SIDE) and bool(alphas.all())
    assert np.abs(np.array(wanted)).max() < 0.95                                  # inside the reach of radius 1
    for b in range(ref.REG_SETS):
        for v in range(ref.REG_VIEWS):
            blob = lrs[b, v] == 1.0
            assert 0.08 < blob.mean() < 0.12 and not masks[b, v][blob].any() and 0.10 < (masks[b, v] == 0).mean() < 0.16
            if v:
                shift, _ = registration_ref.search(lrs[b, 0], masks[b, 0], lrs[b, v], masks[b, v], P=7, levels=5, radius=1.0)
                err = np.abs(shift - wanted[b][v]).max()
                print(f"imageset {b} view {v}: wanted {wanted[b][v]}, fp64 search {shift}, error {err:.4f} px")
                assert err <= 0.02
