"""Helpers of the LR-quality-mask tests (test_lr_masks_host.py, test_gpu_lr_masks.py): imagesets whose QM*.png hold stored values
from {0, 1, 128, 255} (so that "non-zero is clear" is exercised), the numpy restatement of the `lr_masks` of a batch, and the
imagesets of shifted views with saturated blobs that the end-to-end registration tests load.  No test logic here."""
import os

import numpy as np

import DataLoader as DL
from hrnet_hip import augment, io_binding
from imageset_png import write_png
from scale_ref import write_scaled_imageset

QM_VALUES = np.array([0, 1, 128, 255], np.uint8)
VIEWS = (4, 12, 7, 9, 5, 11)


def rewrite_quality_maps(d, seed):
    """Replace every QM*.png of imageset `d` by 8-bit maps of QM_VALUES in blocks of random size (about a quarter of the samples 0)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    for name in sorted(os.listdir(d)):
        if not DL._QM_FILE.match(name):
            continue
        h, w = io_binding.png_info(os.path.join(d, name))[1::-1]
        block = int(rng.integers(1, 6))
        coarse = rng.integers(0, 4, (-(-h // block), -(-w // block)))
        q = QM_VALUES[np.kron(coarse, np.ones((block, block), np.int64))[:h, :w]]
        q[rng.random((h, w)) < 0.05] = 0                               # and single samples, so that no block edge is special
        write_png(os.path.join(d, name), q)


def write_sets(root, ratio, lr=128, views=VIEWS, seed=70):
    """len(views) imagesets with HR / SM stored at `ratio`, LR side `lr`, quality maps of QM_VALUES."""
    os.makedirs(root)
    dirs = [write_scaled_imageset(root, f"imgset{i:04d}", n, ratio, lr=lr, seed=seed + i) for i, n in enumerate(views)]
    for i, d in enumerate(dirs):
        rewrite_quality_maps(d, 900 + i)
    return dirs


def restated_masks(ds, indices, min_L, codes):
    """The `lr_masks` of ds.load_batch(indices, min_L) restated: png_read(QM) != 0 in the order of _pick_views, cut by get_patch at the
    drawn corner, put through augment.apply with the batch's codes (`codes`: ds.last_augment of the call restated, None when
    augmentation is off); padded slots zero.  Makes the RNG calls of load_batch, so it starts from the same RNG state as that call."""
    planes = []
    for b, i in enumerate(indices):
        d = ds.imset_dir[i] if isinstance(i, int) else ds.name_to_dir[i]
        ids, scores = DL._list_views(d)
        pick = DL._pick_views(scores, len(ids), ds.top_k, ds.beta, ds.seed)
        full = [io_binding.png_read(os.path.join(d, f"QM{v}.png")) != 0 for v in ids[pick][:min_L]]
        if ds.create_patches:
            row, col = DL._corner(full[0].shape[0], ds.patch_size, ds.seed)
            full = [DL.get_patch(m, row, col, ds.patch_size) for m in full]
        if ds.augment is not None:
            assert DL._draw_code(ds.augment, ds.seed) == codes[b]             # keeps the RNG in step with load_batch
            full = [augment.apply(m, codes[b]) for m in full]
        S = full[0].shape[0]
        planes.append(np.stack(full + [np.zeros((S, S), bool)] * (min_L - len(full))))
    return np.stack(planes).astype(np.float32)


# ----------------------------------------------------------------------------- shifted views with blobs, for registration
REG_SIDE, REG_VIEWS, REG_SETS = 48, 4, 2
# The seed of registration_shifts: the search reaches +-1 px per axis at radius 1, and two offsets in +-0.9 px can lie 1.8 px apart, so
# the seed is one whose shifts relative to the clearest view stay inside +-0.95 px; and among those (14, 20, 21, 57, 71 below 80) one at
# which the fp64 restatement of the search is well inside the 0.02 px of DESIGN 7f (0.007; at 14, 20 and 71 it is itself at 0.021 ..
# 0.027 for one view, drawn to a fraction of 0.5 where the shifted mask changes by whole pixels).
REG_SHIFT_SEED = 57


def analytic_scene(y, x, k):
    """A scene at real coordinates (imageset k has its own): 48 plane waves of random phase whose frequency vectors are drawn from
    N(0, 0.12^2) cycles / pixel per axis - the spectrum of registration_ref.scene, written as a sum so that it can be evaluated at any
    sub-pixel offset - around 0.7 with a standard deviation of 0.075, cut at 0.99 (below saturation).  Why not something smoother:
    the six-tap sampler of the search has a position bias of up to 0.02 px on a slowly varying scene (its taps' first moment is
    not the fraction they stand for: -0.0198 px at a fraction of 0.25), which alone would use up the bound; and why bright: the
    sampler's taps reach 3 px, past the one-pixel rim of the masks, so what a saturated blob adds to its neighbours grows with
    its distance from the scene's level."""
    rng = np.random.Generator(np.random.PCG64(4000 + k))
    z = np.zeros(np.broadcast(y, x).shape)
    n_waves = 48
    for _ in range(n_waves):
        fy, fx = rng.normal(0.0, 0.12, size=2)
        z = z + np.cos(2 * np.pi * (fy * y + fx * x) + rng.uniform(0, 2 * np.pi))
    return np.clip(0.7 + 0.075 * z / np.sqrt(n_waves / 2.0), 0.0, 0.99)


def registration_shifts(k):
    """(REG_VIEWS, 2) true offsets (ty, tx) of imageset k's views, uniform in +-0.9 px: view(y, x) = scene(y + ty, x + tx)."""
    return np.random.default_rng(REG_SHIFT_SEED + 100 * k).uniform(-0.9, 0.9, size=(REG_VIEWS, 2))


def write_registration_sets(root):
    """REG_SETS imagesets of REG_VIEWS 48 x 48 views, as PNGs: view v of imageset k is the analytic scene at the offset
    registration_shifts(k)[v], 16 bit, with a saturated disc (65535) of its own of about 10 % of the frame (radius 8.1 .. 9 px, a
    different one per view, so the clearance order is strict) and a QM that is 0 exactly on the disc grown by one pixel and 255
    elsewhere; SM / HR (x3) are filler.  clearance.npy comes from DataLoader.save_clearance_scores.
    -> (dirs, wanted): wanted[k] (REG_VIEWS, 2) = the shifts that register the views of imageset k, in the loader's order (clearest
    first), onto the clearest: S(view, s) = first view for s = t_first - t_view (Output(y, x) = Input(y + dy, x + dx))."""
    os.makedirs(root, exist_ok=True)
    n = REG_SIDE
    yy, xx = np.mgrid[0:n, 0:n].astype(np.float64)
    dirs, wanted = [], []
    for k in range(REG_SETS):
        rng = np.random.Generator(np.random.PCG64(77 + k))
        t = registration_shifts(k)
        views = []
        qms = []
        for v in range(REG_VIEWS):
            a = np.rint(analytic_scene(yy + t[v, 0], xx + t[v, 1], k) * 65535.0).astype(np.uint16)
            cy, cx = rng.uniform(12, n - 12, size=2)
            r = 8.1 + 0.3 * ((v + k) % REG_VIEWS)
            blob = (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
            a[blob] = 65535
            grown = blob.copy()
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    grown |= np.roll(np.roll(blob, dy, 0), dx, 1)            # the grown disc stays 2 px inside the frame: nothing wraps
            views.append(a)
            qms.append(np.where(grown, 0, 255).astype(np.uint8))
        d = write_scaled_imageset(root, f"imgset{k:04d}", REG_VIEWS, 3, lr=n, seed=k, lr_views=views)
        for v in range(REG_VIEWS):
            write_png(os.path.join(d, f"QM{v:03d}.png"), qms[v])
        os.remove(os.path.join(d, "clearance.npy"))
        scores, = DL.save_clearance_scores([d])
        order = np.flip(np.argsort(scores))
        assert len(set(scores.tolist())) == REG_VIEWS
        dirs.append(d)
        wanted.append(t[order[0]][None, :] - t[order])
    return dirs, wanted
