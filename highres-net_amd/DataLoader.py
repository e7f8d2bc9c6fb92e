"""DataLoader on the native input pipeline: same import path and names as the reference's `src/DataLoader.py`
(get_patch :16-31, ImageSet :34-49, sample_clearest :52-72, read_imageset :75-148, ImagesetDataset :153-204), so that
`from DataLoader import ImagesetDataset, ImageSet` in src/train.py:20 / src/predict.py:11 resolves here.

Directory listing, clearance loading, the clearance-softmax view sampling and the random patch corner stay in Python and
draw from numpy's global RNG in the reference's order (so a seeded run picks the same views and patch); the byte work -
PNG decode, crop, uint16 -> float32, padding - runs in libhrnet_io.so (`hrnet_hip.io_binding`).  Beyond the reference's
surface, `ImagesetDataset.load_batch()` collates a whole batch straight into (optionally pinned) buffers on a thread pool,
and `ImagesetDataset.to_device()` decodes the whole split once into HBM (DeviceImagesetCache), after which every batch is one
kernel launch (`hrn_collate_device_s`) with the same RNG draws and bit-identical values.

Target scale: HR / SM batches are `scale * S` a side for LR patches of side S, `scale` in {2, 3, 4} (the dataset's `scale`
argument, else config["scale"], else 3).  The patch corner is always drawn in LR pixels, so a seeded run picks the same views and
corner at every scale.  The host path reads files stored at that ratio and never resamples; the device cache can resample
HR / SM stored at another ratio once, when it is built (`to_device(resample_targets=True)`, hrnet_hip/resample.py).

Augmentation (`augment`, else config["augment"]; off by default): "flip" or "dihedral" draws one code per imageset - one of the
4 flips or of all 8 flips and rotations of the square (hrnet_hip/augment.py) - and applies it to the cropped window of every LR
view and of HR / SM.  The draw is one extra `np.random.randint(0, MODES[mode])` per imageset, after `_pick_views` and `_corner`
(after `_pick_views` alone when no patches are cut), re-seeded like `_corner` when `seed` is set: a seeded run picks the same
views and corner with or without it, and with augmentation off no RNG call is added anywhere.  The transform is an addressing
change inside the gathers that run anyway (hrn_io_collate_a on the host, hrn_collate_device_a in the cache); the codes of the last
batch are kept in `last_augment` so that a caller can undo them (`augment.inverse`).

LR quality masks (`lr_masks`, else config["lr_masks"]; off by default): the per-view quality maps `QM*.png` of the views a batch
carries, in the order, window and orientation of its `lrs` - float32, 1.0 where the stored QM sample is non-zero (the rule of
`hr_map` for SM.png), zeros in padding slots - as a sixth item of every batch, ready to be the `lr_masks` of
`hrnet_hip.registration.register_views` / `register_scene`.  They ride in the gathers that build the batch anyway
(hrn_io_collate_m on the host, hrn_collate_device_m from a fourth arena in the cache) and draw nothing from the RNG.  With the
switch off no QM file is opened and every return value is what it was.  `save_clearance_scores` writes the `clearance.npy` the
loaders ask for from the same files.
"""
from collections import OrderedDict
import operator
import os
import re

import numpy as np
import torch
from torch.utils.data import Dataset

from hrnet_hip import augment as _augment
from hrnet_hip import binding, io_binding, resample
from hrnet_hip.resample import check_scale

_QM_FILE = re.compile(r"^QM(.*)\.png$", re.S)       # one quality map per LR view; the text between "QM" and ".png" is the view id


def get_patch(img, x, y, size=32):
    """Square window of the two trailing axes of `img`: rows x .. x+size-1, columns y .. y+size-1 (x is the ROW corner, as in
    the reference); leading axes (e.g. the view axis of an LR stack) are kept."""
    rows, cols = slice(x, x + size), slice(y, y + size)
    return img[..., rows, cols]


class ImageSet(OrderedDict):
    """The assets of one imageset (name, lr, hr, hr_map, clearances) as an ordered mapping whose repr lists one asset per line:
    key right-aligned to 10 columns, then shape / class / dtype for arrays and tensors, class and value for anything else."""

    def __repr__(self):
        def describe(value):
            kind = type(value).__name__
            if hasattr(value, "shape"):
                return f"{value.shape} {kind} ({value.dtype})"
            return f"{kind} ({value})"

        lines = ["name".rjust(10) + f" : {self['name']}"]
        lines.extend(key.rjust(10) + " : " + describe(value) for key, value in self.items())
        return "\n".join(lines)


def sample_clearest(clearances, n=None, beta=50, seed=None):
    """Draw `n` distinct view indices with probability softmax(beta * clearance / max clearance): beta = 0 is uniform, large beta
    approaches "the n clearest".  RNG contract (shared with the reference so that a seeded run picks the same views): an optional
    `np.random.seed(seed)`, then exactly one `np.random.choice(..., replace=False)` over the weights below, computed in the same
    floating-point order ((beta * c) / max c, exp, normalise)."""
    if seed is not None:
        np.random.seed(seed)
    weights = np.exp(np.divide(np.multiply(beta, clearances), np.max(clearances)))
    return np.random.choice(len(weights), size=n, replace=False, p=weights / np.sum(weights))


def _list_views(imset_dir):
    """(sorted view ids, clearances) of an imageset directory; no RNG."""
    ids = np.sort(np.array([m.group(1) for m in map(_QM_FILE.match, os.listdir(imset_dir)) if m]))
    score_file = os.path.join(imset_dir, "clearance.npy")
    if not os.path.isfile(score_file):
        raise Exception("please call the save_clearance.py before call DataLoader")
    return ids, np.load(score_file)


def _pick_views(scores, n_views, top_k, beta, seed):
    """Positions (into the sorted ids) of the views in use order: `top_k` > 0 -> a clearance-weighted sample of min(top_k, L)
    views (sample_clearest), else all views from the clearest down."""
    if top_k is not None and top_k > 0:
        return sample_clearest(scores, n=min(top_k, n_views), beta=beta, seed=seed)
    return np.flip(np.argsort(scores))


def _views_in_use_order(imset_dir, top_k, beta, seed):
    """(view ids, clearances) of an imageset in the order the model consumes them (_pick_views)."""
    ids, scores = _list_views(imset_dir)
    pick = _pick_views(scores, len(ids), top_k, beta, seed)
    return ids[pick], scores[pick]


def _corner(lr_side, patch_size, seed):
    """Random patch corner (row, column): an optional re-seed, then two `np.random.randint(0, side - patch)` draws, row first."""
    if seed is not None:
        np.random.seed(seed)
    limit = lr_side - patch_size
    row = np.random.randint(low=0, high=limit)
    col = np.random.randint(low=0, high=limit)
    return row, col


def _draw_code(mode, seed):
    """Augmentation code of one imageset: an optional re-seed (as _corner), then one `np.random.randint(0, MODES[mode])`."""
    if seed is not None:
        np.random.seed(seed)
    return int(np.random.randint(low=0, high=_augment.MODES[mode]))


def _ratio_error(name, lr_side, scale, found):
    """The ValueError for an imageset whose HR / SM files are not `scale` times its LR side."""
    return ValueError(f"{name}: HR / SM side is {found} but scale {scale} needs {scale * lr_side} ({scale} x the LR side {lr_side}); the host "
                      f"path does not resample - build a device cache with to_device(resample_targets=True)")


def _qm_mismatch(path, found, side):
    """The ValueError for a quality map that is not the size of its LR view."""
    return ValueError(f"{path} is {found[1]}x{found[0]} but its LR view is {side[1]}x{side[0]}")


def read_imageset(imset_dir, create_patches=False, patch_size=64, seed=None, top_k=None, beta=0., scale=3, augment=None, lr_masks=False):
    """ImageSet(name, lr uint16 (L,H,W), hr uint16 or None, hr_map bool, clearances) of one imageset directory, PNGs decoded by
    the native reader.  With `create_patches` one random `patch_size` window is cut from every LR view and the matching
    `scale`x window from SM / HR, whose files must be `scale` times the LR side (ValueError otherwise).  `augment` (a mode of
    hrnet_hip/augment.py): one code is drawn after the views and the corner and applied to lr, hr_map and hr.  `lr_masks`: a
    further key `lr_maps` after `clearances`, bool (L,H,W): QM*.png != 0 of the views of `lr`, in their order, window and code."""
    scale = check_scale(scale)
    mode = _augment.check_mode(augment)
    ids, scores = _views_in_use_order(imset_dir, top_k, beta, seed)
    asset = lambda name: os.path.join(imset_dir, name)
    lr = np.stack([io_binding.png_read(asset(f"LR{i}.png")) for i in ids]).astype(np.uint16, copy=False)
    lr_maps = None
    if lr_masks:
        lr_maps = []
        for i in ids:
            lr_maps.append(io_binding.png_read(asset(f"QM{i}.png")) != 0)
            if lr_maps[-1].shape != lr.shape[1:]:
                raise _qm_mismatch(asset(f"QM{i}.png"), lr_maps[-1].shape, lr.shape[1:])
        lr_maps = np.stack(lr_maps)
    hr_map = io_binding.png_read(asset("SM.png")) != 0
    hr = io_binding.png_read(asset("HR.png")).astype(np.uint16, copy=False) if os.path.exists(asset("HR.png")) else None
    for img in (hr_map, hr):
        if img is not None and img.shape != (scale * lr.shape[1], scale * lr.shape[2]):
            raise _ratio_error(os.path.basename(imset_dir), lr.shape[1], scale, img.shape[0])
    if create_patches:
        row, col = _corner(lr.shape[1], patch_size, seed)
        lr = get_patch(lr, row, col, patch_size)
        hr_map = get_patch(hr_map, scale * row, scale * col, scale * patch_size)
        if lr_maps is not None:
            lr_maps = get_patch(lr_maps, row, col, patch_size)
        if hr is not None:
            hr = get_patch(hr, scale * row, scale * col, scale * patch_size)
    if mode is not None:
        code = _draw_code(mode, seed)
        lr, hr_map = _augment.apply(lr, code), np.ascontiguousarray(_augment.apply(hr_map, code))
        if hr is not None:
            hr = np.ascontiguousarray(_augment.apply(hr, code))
        if lr_maps is not None:
            lr_maps = _augment.apply(lr_maps, code)
    out = ImageSet(name=os.path.basename(imset_dir), lr=np.array(lr), hr=hr, hr_map=hr_map, clearances=scores)
    if lr_maps is not None:
        out["lr_maps"] = np.array(lr_maps)
    return out


def save_clearance_scores(dataset_directories):
    """Write `clearance.npy` into every imageset directory of `dataset_directories`: per view, in sorted view-id order, the sum of
    the stored sample values of its QM*.png (uint16 samples summed by numpy.sum, so the saved array is uint64) - the score the
    loaders sort and sample the views by.  Returns the arrays, one per directory."""
    saved = []
    for d in dataset_directories:
        ids = np.sort(np.array([m.group(1) for m in map(_QM_FILE.match, os.listdir(d)) if m]))
        maps = np.array([io_binding.png_read(os.path.join(d, f"QM{i}.png")).astype(np.uint16, copy=False) for i in ids])
        scores = np.sum(maps, axis=(1, 2))
        np.save(os.path.join(d, "clearance.npy"), scores)
        saved.append(scores)
    return saved


class ImagesetDataset(Dataset):
    """Dataset over imageset directories.  `dataset[i]` (int), `dataset["imgsetXXXX"]` (name) -> one ImageSet of float32
    tensors (lr (L,S,S), hr / hr_map (kS,kS) with k = `scale`; test imagesets keep hr = None and a bool numpy hr_map); a slice
    -> a list.  `scale` (2, 3 or 4; None: config.get("scale", 3)) is the HR / LR ratio of the batches and, on this host path, of
    the files.  `augment` (None: config.get("augment"); then None / False / "none" off, "flip", "dihedral" or True): one flip /
    rotation code per imageset (module docstring); `last_augment` holds the codes of the last item or batch loaded (a list of
    ints, None while augmentation is off).  None defers to the config, so a dataset built from a config that carries the key
    is switched off with `augment=False`.  `lr_masks` (None: config.get("lr_masks", False)): items carry `lr_maps`, float32
    (L,S,S), and `load_batch` returns a sixth item, the (B,min_L,S,S) quality masks of the views in `lrs` (module docstring)."""

    def __init__(self, imset_dir, config, seed=None, top_k=-1, beta=0., scale=None, augment=None, lr_masks=None):
        super().__init__()
        self.scale = check_scale(config.get("scale", 3) if scale is None else scale)
        self.augment = _augment.check_mode(config.get("augment") if augment is None else augment)
        self.last_augment = None
        self.lr_masks = bool(config.get("lr_masks", False) if lr_masks is None else lr_masks)
        self.imset_dir = imset_dir
        self.name_to_dir = dict(zip(map(os.path.basename, imset_dir), imset_dir))
        self.create_patches, self.patch_size = config["create_patches"], config["patch_size"]
        self.seed, self.top_k, self.beta = seed, top_k, beta          # seed: re-seeds numpy's global RNG per imageset when set

    def __len__(self):
        return len(self.imset_dir)

    def _resolve(self, index):
        """Directories an index stands for, and whether the caller gets a bare ImageSet (int / name) or a list (slice)."""
        if isinstance(index, str):
            return [self.name_to_dir[index]], True
        if isinstance(index, slice):
            picked = self.imset_dir[index]
            return picked, len(picked) == 1
        if isinstance(index, int):
            return [self.imset_dir[operator.index(index)]], True
        raise KeyError("index must be int, string, or slice")

    def __getitem__(self, index):
        dirs, single = self._resolve(index)
        loaded = [self._load_one(d) for d in dirs]
        return loaded[0] if single else loaded

    def _plan(self, dir_):
        """Everything random / directory-dependent for one imageset, in the reference's RNG order."""
        idx_names, clearances = _views_in_use_order(dir_, self.top_k, self.beta, self.seed)
        lr_paths = [os.path.join(dir_, f"LR{i}.png") for i in idx_names]
        lr_side = io_binding.png_info(lr_paths[0])[0]
        corner = _corner(lr_side, self.patch_size, self.seed) if self.create_patches else (0, 0)
        code = _draw_code(self.augment, self.seed) if self.augment is not None else None
        hr_path = os.path.join(dir_, "HR.png") if os.path.exists(os.path.join(dir_, "HR.png")) else None
        qm_paths = [os.path.join(dir_, f"QM{i}.png") for i in idx_names] if self.lr_masks else None
        return dict(name=os.path.basename(dir_), lr_paths=lr_paths, clearances=clearances, lr_side=lr_side, corner=corner, hr=hr_path,
                    sm=os.path.join(dir_, "SM.png"), code=code, qm_paths=qm_paths)

    def _codes(self, plans):
        """Codes of a batch for io_binding.collate (None while augmentation is off), recorded in `last_augment`."""
        self.last_augment = [p["code"] for p in plans] if self.augment is not None else None
        return self.last_augment

    def _collate(self, plans, **kw):
        """io_binding.collate at the dataset's scale.  A failure is looked at only after the fact (no extra file read on the
        good path): if an HR / SM file of the batch is not scale x its LR side, that is the ValueError to raise."""
        if self.lr_masks:
            kw["qm_paths_per_set"] = [pl["qm_paths"] for pl in plans]
        try:
            return io_binding.collate(scale=self.scale, **kw)
        except io_binding.HrnetIoError as err:
            for pl in plans:
                for path in (pl["sm"], pl["hr"]):
                    if path is not None and os.path.exists(path):
                        w, h, _ = io_binding.png_info(path)
                        if (w, h) != (self.scale * pl["lr_side"],) * 2:
                            raise _ratio_error(pl["name"], pl["lr_side"], self.scale, w if w == h else f"{w}x{h}") from err
            raise

    def _load_one(self, dir_):
        pl = self._plan(dir_)
        patch = self.patch_size if self.create_patches else 0
        out = self._collate([pl], lr_paths_per_set=[pl["lr_paths"]], hr_paths=[pl["hr"]], sm_paths=[pl["sm"]], min_L=len(pl["lr_paths"]),
                            lr_size=pl["lr_side"], patch=patch, corners=[pl["corner"]], codes=self._codes([pl]))
        labelled = pl["hr"] is not None
        item = ImageSet(name=pl["name"], lr=torch.from_numpy(out["lrs"][0]), hr=torch.from_numpy(out["hrs"][0]) if labelled else None,
                        hr_map=torch.from_numpy(out["maps"][0]) if labelled else out["maps"][0].astype(bool), clearances=pl["clearances"])
        if self.lr_masks:
            item["lr_maps"] = torch.from_numpy(out["lr_masks"][0])
        return item

    def load_batch(self, indices, min_L, pin_memory=False, n_threads=0):
        """One collated batch (padded_lr (B,min_L,S,S), alphas (B,min_L), hrs (B,kS,kS) or [], hr_maps (B,kS,kS), names; k = scale)
        decoded straight into (optionally pinned) buffers by the native thread pool: __getitem__ + collateFunction in one call.
        With `lr_masks` on, a sixth item: the quality masks (B,min_L,S,S) of the views in padded_lr, zeros in padding slots."""
        plans = [self._plan(self.imset_dir[i] if isinstance(i, int) else self.name_to_dir[i]) for i in indices]
        side = plans[0]["lr_side"]
        if any(p["lr_side"] != side for p in plans):
            raise ValueError("imagesets of one batch must share the LR size")
        patch = self.patch_size if self.create_patches else 0
        S = patch if patch else side
        T = self.scale * S
        B = len(plans)
        have_hr = all(p["hr"] is not None for p in plans)
        mk = lambda *shape: torch.empty(shape, dtype=torch.float32, pin_memory=pin_memory)
        out = dict(lrs=mk(B, min_L, S, S), alphas=mk(B, min_L), hrs=mk(B, T, T) if have_hr else None, maps=mk(B, T, T))
        if self.lr_masks:
            out["lr_masks"] = mk(B, min_L, S, S)
        self._collate(plans, lr_paths_per_set=[p["lr_paths"] for p in plans], hr_paths=[p["hr"] for p in plans] if have_hr else None,
                      sm_paths=[p["sm"] for p in plans], min_L=min_L, lr_size=side, patch=patch, corners=[p["corner"] for p in plans], out=out,
                      n_threads=n_threads, codes=self._codes(plans))
        batch = out["lrs"], out["alphas"], out["hrs"] if have_hr else [], out["maps"], [p["name"] for p in plans]
        return batch + (out["lr_masks"],) if self.lr_masks else batch

    def to_device(self, device="cuda", n_threads=0, resample_targets=False):
        """Decode every imageset once into HBM and return a DeviceImagesetCache: `cache.load_batch(indices, min_L)` then
        builds each batch on the GPU with one kernel, bit-identical to `load_batch` and from the same numpy RNG draws.
        `resample_targets`: HR / SM files stored at another ratio than the dataset's scale (2, 3 or 4 times the LR side) are
        resampled to it on the device while the cache is built; without it such an imageset raises, as on the host path."""
        return DeviceImagesetCache(self, device=device, n_threads=n_threads, resample_targets=resample_targets)


def _round4(n):
    return (n + 3) // 4 * 4


class ImagesetIndex:
    """The host half of DeviceImagesetCache, no GPU: every imageset directory listed once, clearance.npy loaded once, the LR
    side and the stored HR / SM side read from one header each, and where each image lives in the three arenas (LR / HR
    uint16, SM uint8; every image starts at a multiple of 4 elements, as hrn_collate_device requires; with the dataset's `lr_masks`
    on, a fourth arena QM, uint8, at the LR arena's offsets: `qm_elems` == `lr_elems`, else 0).  HR / SM slots hold
    scale^2 side^2 samples, scale = dataset.scale.  `ratios[k]` is the ratio imageset k is stored at; one that differs from
    the scale needs `resample_targets` (the cache then resamples it into its slot), else it is the host path's ValueError.
    `plan()` turns a batch of indices into the kernel's plan table with exactly the numpy RNG calls ImagesetDataset._plan makes,
    in the same order; `plan_a()` returns the augmentation codes of the batch beside it (`last_augment` keeps them as a list)."""

    def __init__(self, dataset, resample_targets=False):
        self.dataset = dataset
        self.scale = scale = dataset.scale
        self.dirs = list(dataset.imset_dir)
        self.names = [os.path.basename(d) for d in self.dirs]
        self.position = dict(zip(self.names, range(len(self.dirs))))      # a repeated name resolves to its last directory, as name_to_dir
        self.ids, self.clearances, self.sides, self.lr_off, self.hr_off, self.sm_off, self.ratios = [], [], [], [], [], [], []
        lr_total = hr_total = sm_total = 0
        for d in self.dirs:
            ids, scores = _list_views(d)
            if len(ids) == 0:
                raise ValueError(f"{d}: no LR views")
            side = io_binding.png_info(os.path.join(d, f"LR{ids[0]}.png"))[0]
            self.ids.append(ids)
            self.clearances.append(scores)
            self.sides.append(side)
            slot = _round4(side * side)
            self.lr_off.append(lr_total + slot * np.arange(len(ids), dtype=np.int64))
            lr_total += slot * len(ids)
            have_hr = os.path.exists(os.path.join(d, "HR.png"))
            self.ratios.append(self._stored_ratio(d, side, have_hr, resample_targets))
            if have_hr:
                self.hr_off.append(hr_total)
                hr_total += _round4(scale * scale * side * side)
            else:
                self.hr_off.append(-1)
            self.sm_off.append(sm_total)
            sm_total += _round4(scale * scale * side * side)
        self.lr_elems, self.hr_elems, self.sm_elems = lr_total, hr_total, sm_total
        self.qm_elems = lr_total if dataset.lr_masks else 0          # the mask of the view at LR offset o lives at QM offset o
        self.last_augment = None

    def _stored_ratio(self, d, side, have_hr, resample_targets):
        """HR / LR ratio of the files of imageset `d`, from the SM (and HR) header: the scale itself, or with `resample_targets`
        any of 2, 3, 4."""
        found = [io_binding.png_info(os.path.join(d, f))[:2] for f in ["SM.png"] + (["HR.png"] if have_hr else [])]
        w, h = found[0]
        ok = all(wh == (w, h) for wh in found) and w == h and w % side == 0
        ratio = w // side if ok else 0
        if ratio != self.scale and not (resample_targets and ratio in resample.SCALES):
            shown = w if ok else " / ".join(f"{a}x{b}" for a, b in found)
            if resample_targets:
                raise ValueError(f"{os.path.basename(d)}: HR / SM side {shown} is not 2, 3 or 4 times the LR side {side}: cannot resample")
            raise _ratio_error(os.path.basename(d), side, self.scale, shown)
        return ratio

    def __len__(self):
        return len(self.dirs)

    def resolve(self, index):
        """Position of an int index or an imageset name (KeyError for an unknown name), as ImagesetDataset.load_batch."""
        return range(len(self.dirs))[index] if isinstance(index, int) else self.position[index]

    def plan(self, indices, min_L):
        """-> (plan (B, COLLATE_META + min_L) int64, names, S, have_hr) for hrn_collate_device: plan_a without the codes."""
        plan, _, names, S, have_hr = self.plan_a(indices, min_L)
        return plan, names, S, have_hr

    def plan_a(self, indices, min_L):
        """-> (plan (B, COLLATE_META + min_L) int64, codes (B,) int32 or None, names, S, have_hr) for hrn_collate_device_a.
        RNG: per imageset, in order, _pick_views (sample_clearest, or the clearance sort for top_k <= 0), then _corner and,
        with augmentation on, _draw_code, with the dataset's seed.  codes is None while augmentation is off."""
        ds = self.dataset
        rows, codes = [], []
        for i in indices:
            k = self.resolve(i)
            pick = _pick_views(self.clearances[k], len(self.ids[k]), ds.top_k, ds.beta, ds.seed)
            corner = _corner(self.sides[k], ds.patch_size, ds.seed) if ds.create_patches else (0, 0)
            if ds.augment is not None:
                codes.append(_draw_code(ds.augment, ds.seed))
            rows.append((k, pick, corner))
        self.last_augment = codes if ds.augment is not None else None
        side = self.sides[rows[0][0]]
        if any(self.sides[k] != side for k, _, _ in rows):
            raise ValueError("imagesets of one batch must share the LR size")
        patch = ds.patch_size if ds.create_patches else 0
        S = patch if patch else side
        have_hr = all(self.hr_off[k] >= 0 for k, _, _ in rows)
        plan = np.full((len(rows), binding.COLLATE_META + min_L), -1, np.int64)
        for b, (k, pick, (row, col)) in enumerate(rows):
            used = self.lr_off[k][pick[:min_L]]
            plan[b, :binding.COLLATE_META] = (self.hr_off[k] if have_hr else -1, self.sm_off[k], side, row if patch else 0,
                                              col if patch else 0)
            plan[b, binding.COLLATE_META:binding.COLLATE_META + len(used)] = used
        return plan, np.asarray(codes, np.int32) if ds.augment is not None else None, [self.names[k] for k, _, _ in rows], S, have_hr


class DeviceImagesetCache:
    """Every imageset of an ImagesetDataset decoded once and kept on the device (LR / HR as uint16, SM as uint8, allocated
    through torch's caching allocator), and batches built there by one hrn_collate_device_s launch each:

        cache = dataset.to_device("cuda", n_threads=16)
        lrs, alphas, hrs, hr_maps, names = cache.load_batch(indices, min_L)      # device tensors, no file I/O

    `load_batch` has the contract of ImagesetDataset.load_batch (same tuple, values bit-identical, hrs == [] when an imageset
    lacks HR.png, ValueError for mixed LR sizes, KeyError for an unknown name) and makes the same numpy RNG calls in the same
    order, so a seeded run picks the same views, patches and (with the dataset's `augment` on) flip / rotation codes on either
    path; `last_augment` holds the codes of the last batch (a list of ints, None while augmentation is off).  Per batch: the
    plan (Python, ImagesetIndex.plan_a), one small pinned host-to-device copy of the plan table (the codes ride in the same
    buffer) and one kernel, all enqueued on the current stream; no device-to-host copy and no synchronisation.  Memory: `nbytes`
    (2 B per LR / HR sample, 1 B per SM sample).

    With the dataset's `lr_masks` on, a fourth arena `qm` (uint8, 0 / 1, one byte per LR sample at the LR arena's offsets; `nbytes`
    counts it) is decoded beside the others, and `load_batch` / `batches` return the 6-tuple of ImagesetDataset.load_batch from the
    same single launch (hrn_collate_device_m).

    `resample_targets=True`: an imageset whose HR / SM files are stored at another ratio R than the dataset's scale is decoded
    at R into a staging buffer and resampled into its arena slot by hrn_resample_targets (hrnet_hip/resample.py gives the rule:
    Lanczos-3, widened when shrinking; a resampled SM sample is clear only if every source sample under its filter is), one
    launch per (LR side, R) and arena; imagesets stored at the scale are kept as decoded.  The staging buffers are gone once the
    cache is built; batches cost what they cost without resampling."""

    def __init__(self, dataset, device="cuda", n_threads=0, chunk_elems=1 << 26, resample_targets=False):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"DeviceImagesetCache needs a ROCm device, got '{self.device}' (the host path is ImagesetDataset.load_batch)")
        if not torch.cuda.is_available():
            raise RuntimeError("DeviceImagesetCache: device is cuda but no GPU is available")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        binding.load_library()
        self.index = idx = ImagesetIndex(dataset, resample_targets=resample_targets)
        self.scale = idx.scale
        self.last_augment = None
        dev = self.device
        self.lr = torch.empty(idx.lr_elems, dtype=torch.uint16, device=dev)
        self.hr = torch.empty(idx.hr_elems, dtype=torch.uint16, device=dev) if idx.hr_elems else None
        self.sm = torch.empty(idx.sm_elems, dtype=torch.uint8, device=dev)
        self.qm = torch.empty(idx.qm_elems, dtype=torch.uint8, device=dev) if idx.qm_elems else None
        tables = {}                                                # (side, R) -> resampling weight table, for the build only
        # decode in chunks of consecutive imagesets (contiguous ranges of each arena) to bound host memory
        start = 0
        while start < len(idx):
            stop, elems = start, 0
            while stop < len(idx) and (stop == start or elems < chunk_elems):
                elems += len(idx.ids[stop]) * idx.sides[stop] ** 2
                stop += 1
            self._decode(start, stop, n_threads, tables)
            start = stop

    def _decode(self, start, stop, n_threads, tables):
        idx, scale = self.index, self.scale
        lr_paths, lr_offs, lr_sides, qm_paths = [], [], [], []      # a mask shares offset and side with its LR view
        hr_paths, hr_offs, hr_sides, sm_paths, sm_offs, sm_sides = [], [], [], [], [], []
        hr_stage, sm_stage = [], []                                # (path, arena offset, LR side, stored ratio) of images to resample
        for k in range(start, stop):
            d, side, ratio = idx.dirs[k], idx.sides[k], idx.ratios[k]
            lr_paths += [os.path.join(d, f"LR{i}.png") for i in idx.ids[k]]
            lr_offs += list(idx.lr_off[k])
            lr_sides += [side] * len(idx.ids[k])
            if self.qm is not None:
                qm_paths += [os.path.join(d, f"QM{i}.png") for i in idx.ids[k]]
            if idx.hr_off[k] >= 0:
                if ratio == scale:
                    hr_paths.append(os.path.join(d, "HR.png"))
                    hr_offs.append(idx.hr_off[k])
                    hr_sides.append(scale * side)
                else:
                    hr_stage.append((os.path.join(d, "HR.png"), idx.hr_off[k], side, ratio))
            if ratio == scale:
                sm_paths.append(os.path.join(d, "SM.png"))
                sm_offs.append(idx.sm_off[k])
                sm_sides.append(scale * side)
            else:
                sm_stage.append((os.path.join(d, "SM.png"), idx.sm_off[k], side, ratio))
        is_clear = lambda a: (a != 0).astype(np.uint8)
        for paths, offs, sides, arena, to_host in ((lr_paths, lr_offs, lr_sides, self.lr, None), (hr_paths, hr_offs, hr_sides, self.hr, None),
                                                   (sm_paths, sm_offs, sm_sides, self.sm, is_clear), (qm_paths, lr_offs, lr_sides, self.qm, is_clear)):
            if not paths:
                continue
            # one contiguous host range from the first to the last image; slots of images to resample inside it are written
            # (as zeros) here and filled afterwards, on the same stream
            offs = np.asarray(offs, np.int64)
            lo = int(offs[0])
            hi = int(offs[-1]) + _round4(sides[-1] ** 2)
            host = np.zeros(hi - lo, np.uint16)
            io_binding.read_many(paths, host, offs - lo, sides, sides, n_threads=n_threads)
            if to_host is None:
                arena.view(torch.int16)[lo:hi].copy_(torch.from_numpy(host.view(np.int16)))
            else:
                arena[lo:hi].copy_(torch.from_numpy(to_host(host)))
        for stage, arena, to_host in ((hr_stage, self.hr, None), (sm_stage, self.sm, is_clear)):
            for side, ratio in sorted({(s, r) for _, _, s, r in stage}):
                group = [(p, o) for p, o, s, r in stage if (s, r) == (side, ratio)]
                n_in, slot = ratio * side, _round4((ratio * side) ** 2)
                host = np.zeros(slot * len(group), np.uint16)
                src_offs = slot * np.arange(len(group), dtype=np.int64)
                io_binding.read_many([p for p, _ in group], host, src_offs, [n_in] * len(group), [n_in] * len(group), n_threads=n_threads)
                if to_host is None:
                    staged = torch.from_numpy(host.view(np.int16)).to(self.device).view(torch.uint16)
                else:
                    staged = torch.from_numpy(to_host(host)).to(self.device)
                if (side, ratio) not in tables:
                    tables[side, ratio] = resample.weight_table(side, ratio, scale)
                jobs = np.stack([src_offs, np.asarray([o for _, o in group], np.int64)], axis=1)
                with torch.cuda.device(self.device):
                    for at in range(0, len(jobs), 65535):
                        binding.resample_targets(staged, arena, jobs[at:at + 65535], n_in, scale * side, tables[side, ratio])
                    staged.record_stream(torch.cuda.current_stream())

    def __len__(self):
        return len(self.index)

    @property
    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in (self.lr, self.hr, self.sm, self.qm) if t is not None)

    def load_batch(self, indices, min_L):
        """(lrs (B,min_L,S,S), alphas (B,min_L), hrs (B,kS,kS) or [], hr_maps (B,kS,kS), names) on the cache's device; k = scale.
        With the dataset's `lr_masks` on, a sixth item: lr_masks (B,min_L,S,S)."""
        plan, codes, names, S, have_hr = self.index.plan_a(indices, min_L)
        self.last_augment = self.index.last_augment
        B = len(names)
        with torch.cuda.device(self.device):
            codes_d = None
            if codes is None:
                plan_d = torch.from_numpy(plan).pin_memory().to(self.device, non_blocking=True)
            else:                                                  # one allocation, two pointers: plan rows, then B int32 codes
                words = plan.size
                host = np.zeros(words + (B + 1) // 2, np.int64)
                host[:words] = plan.ravel()
                host[words:].view(np.int32)[:B] = codes
                both = torch.from_numpy(host).pin_memory().to(self.device, non_blocking=True)
                plan_d, codes_d = both[:words].view(plan.shape), both[words:].view(torch.int32)[:B]
            mk = lambda *shape: torch.empty(shape, dtype=torch.float32, device=self.device)
            T = self.scale * S
            lrs, alphas, maps = mk(B, min_L, S, S), mk(B, min_L), mk(B, T, T)
            hrs = mk(B, T, T) if have_hr else None
            masks = mk(B, min_L, S, S) if self.qm is not None else None
            binding.collate_device(self.lr, self.hr, self.sm, plan_d, S, lrs, alphas, hrs, maps, scale=self.scale, codes=codes_d,
                                   qm_arena=self.qm, lr_masks=masks)
        batch = lrs, alphas, hrs if have_hr else [], maps, names
        return batch + (masks,) if masks is not None else batch

    def batches(self, index_lists, min_L):
        """Batches of `index_lists` in order, in the role of BatchPrefetcher.  Nothing needs a worker thread: a batch costs its
        plan and one launch on the current stream, which runs after the work already queued there (the previous step)."""
        for idx in index_lists:
            yield self.load_batch(list(idx), min_L)


class BatchPrefetcher:
    """Iterate over whole batches of an ImagesetDataset with the next batch's decode and host-to-device copy running
    while the caller computes on the current one.

        for lrs, alphas, hrs, hr_maps, names in BatchPrefetcher(dataset, batches, min_L, device="cuda"):
            ...

    `batches` is a sequence of index lists (what a BatchSampler yields).  A worker thread decodes batch n+1 with
    `load_batch(pin_memory=True)` - the native thread pool does the PNG work - and, for a CUDA device, enqueues the copies
    on a private stream; the consumer's stream waits on that copy's event only when it takes the batch, so PCIe traffic and
    decode overlap the kernels of batch n.  Tensors are handed over with `record_stream`, i.e. their memory is not reused
    before the consumer's queued work has finished.  With device=None or "cpu" it is a plain background decoder.
    Errors raised by the worker are re-raised in the consumer at the batch they belong to.  `last_augment` holds the augmentation
    codes of the batch most recently handed to the consumer (the dataset's own attribute runs ahead with the worker).  A dataset
    with `lr_masks` on yields 6-tuples; the masks are copied and handed over like the other tensors."""

    def __init__(self, dataset, batches, min_L, device=None, depth=2, n_threads=0):
        import queue
        import threading
        self.dataset, self.batches, self.min_L = dataset, [list(b) for b in batches], int(min_L)
        self.device = torch.device(device) if device is not None else None
        self.on_gpu = self.device is not None and self.device.type == "cuda"
        if self.on_gpu and not torch.cuda.is_available():
            raise RuntimeError("BatchPrefetcher: device is cuda but no GPU is available")
        self.n_threads = n_threads
        self.last_augment = None
        self._q = queue.Queue(maxsize=max(1, int(depth)))
        self._stop = threading.Event()
        self._thread = threading.Thread(target=self._work, name="hrn-batch-prefetch", daemon=True)
        self._started = False

    def __len__(self):
        return len(self.batches)

    def _work(self):
        stream = torch.cuda.Stream(device=self.device) if self.on_gpu else None
        try:
            for idx in self.batches:
                if self._stop.is_set():
                    return
                try:
                    lrs, alphas, hrs, maps, names, *masks = self.dataset.load_batch(idx, self.min_L, pin_memory=self.on_gpu,
                                                                                    n_threads=self.n_threads)
                    event = None
                    if self.on_gpu:
                        with torch.cuda.stream(stream):
                            lrs = lrs.to(self.device, non_blocking=True)
                            alphas = alphas.to(self.device, non_blocking=True)
                            maps = maps.to(self.device, non_blocking=True)
                            if isinstance(hrs, torch.Tensor):
                                hrs = hrs.to(self.device, non_blocking=True)
                            masks = [m.to(self.device, non_blocking=True) for m in masks]
                            event = torch.cuda.Event()
                            event.record(stream)
                    item = ("ok", ((lrs, alphas, hrs, maps, names, *masks), getattr(self.dataset, "last_augment", None)), event, stream)
                except Exception as exc:                     # handed to the consumer, in order
                    item = ("err", exc, None, None)
                while not self._stop.is_set():
                    try:
                        self._q.put(item, timeout=0.1)
                        break
                    except Exception:
                        continue
                if item[0] == "err":
                    return
        finally:
            while not self._stop.is_set():
                try:
                    self._q.put(("end", None, None, None), timeout=0.1)
                    break
                except Exception:
                    continue

    def __iter__(self):
        if self._started:
            raise RuntimeError("BatchPrefetcher can be iterated once")
        self._started = True
        self._thread.start()
        try:
            while True:
                kind, payload, event, stream = self._q.get()
                if kind == "end":
                    return
                if kind == "err":
                    raise payload
                if event is not None:
                    cur = torch.cuda.current_stream(self.device)
                    cur.wait_event(event)
                    for t in payload[0]:
                        if isinstance(t, torch.Tensor):
                            t.record_stream(cur)
                self.last_augment = payload[1]
                yield payload[0]
        finally:
            self.close()

    def close(self):
        self._stop.set()
        if self._thread.is_alive():
            self._thread.join(timeout=5.0)
