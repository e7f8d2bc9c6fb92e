"""Input-pipeline rate: the host path (ImagesetDataset.load_batch, BatchPrefetcher) against the HBM-resident cache
(DeviceImagesetCache, one hrn_collate_device launch per batch) on synthetic imagesets in the PROBA-V layout.

    python tools/loader_rate.py [--sets 64] [--threads 16] [--json out.json] [--no-prof] [--augment flip|dihedral] [--lr-masks]
                                [--full-frames] [--kernel-only]

Writes the imagesets to a temporary directory (the stdlib zlib PNG writer of tests/imageset_png.py; smooth 16-bit fields plus
noise, 19-35 views of 128x128, HR / SM 384x384), then per shape (B / top_k / min_L / patch):
  - the cache's build time and bytes,
  - each rate as the median, min and max of --repeats windows of at least 1.5 s, after an untimed warm-up of the same calls,
  - the host path split into planning (ImagesetDataset._plan: listing, clearance.npy, PNG header, RNG) and decoding
    (io_binding.collate on `--threads` threads),
  - batches/s of load_batch (pageable and pinned), of BatchPrefetcher(device="cuda") in steady state with an idle consumer and
    (first shape) with a consumer that spends one training step (26.2 / 55 ms) per batch, of cache.load_batch and cache.batches,
  - the kernel time of hrn_collate_device from `rocprofv3 --kernel-trace --stats` (a child process of this script).
`--augment MODE` measures the same with flip / rotate augmentation on (one code per imageset, hrnet_hip/augment.py), on both paths.
`--lr-masks` measures the same with the LR quality masks on (ImagesetDataset(lr_masks=True): one more PNG decode per view on the host
path, a fourth arena and hrn_collate_device_m in the cache), on both paths.  `--full-frames` loads whole 128 x 128 views instead of
patches; `--kernel-only` skips the rates and runs the rocprofv3 child alone.
Needs a ROCm device; prints one JSON object."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import _common
import numpy as np

_common.tests_on_path()
from imageset_png import write_png                 # the stdlib PNG writer the tests use  # noqa: E402

SHAPES = [dict(B=32, top_k=32, min_L=32, patch=64), dict(B=8, top_k=8, min_L=2, patch=64)]      # README step; shipped config.json
STEPS_MS = (26.2, 55.0)            # README: the training step at SHAPES[0] with HRNet + ShiftNet in bf16, and with HRNet in bf16x3
MIN_WINDOW_S = 1.5
AUGMENT = None                     # --augment: the datasets' augmentation mode
LR_MASKS = False                   # --lr-masks: the datasets carry the LR quality masks
FULL_FRAMES = False                # --full-frames: no patches


def smooth_field(rng, n, waves=6):
    y, x = np.mgrid[0:n, 0:n] / n
    f = np.zeros((n, n))
    for _ in range(waves):
        kx, ky, ph = rng.uniform(0.5, 4), rng.uniform(0.5, 4), rng.uniform(0, 2 * np.pi)
        f += rng.uniform(0.3, 1) * np.sin(2 * np.pi * (kx * x + ky * y) + ph)
    return f / np.abs(f).max()                                                 # in [-1, 1]


def write_imagesets(root, n_sets, seed=0):
    rng = np.random.Generator(np.random.PCG64(seed))
    dirs = []
    for s in range(n_sets):
        d = os.path.join(root, f"imgset{s:04d}")
        os.makedirs(d)
        hr = 14000 + 3000 * smooth_field(rng, 384)                             # radiance-like 16-bit values, far from 0 and 65535
        write_png(os.path.join(d, "HR.png"), np.clip(hr + rng.normal(0, 60, hr.shape), 0, 65535).astype(np.uint16), level=6)
        write_png(os.path.join(d, "SM.png"), ((smooth_field(rng, 384, 3) > -0.6) * 255).astype(np.uint8), level=6)
        lr_mean = hr.reshape(128, 3, 128, 3).mean(axis=(1, 3))
        n_views = int(rng.integers(19, 36))
        for v in range(n_views):
            lr = lr_mean * rng.uniform(0.97, 1.03) + rng.normal(0, 80, lr_mean.shape)
            write_png(os.path.join(d, f"LR{v:03d}.png"), np.clip(lr, 0, 65535).astype(np.uint16), level=6)
            write_png(os.path.join(d, f"QM{v:03d}.png"), ((smooth_field(rng, 128, 2) > -0.7) * 255).astype(np.uint8), level=6)
        np.save(os.path.join(d, "clearance.npy"), rng.uniform(0.5, 1.0, n_views))
        dirs.append(d)
    return dirs


def batch_lists(n_sets, B, n_batches, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return [[int(i) for i in rng.choice(n_sets, B, replace=False)] for _ in range(n_batches)]


def dataset(dirs, shape):
    import DataLoader as DL
    return DL.ImagesetDataset(dirs, {"create_patches": not FULL_FRAMES, "patch_size": shape["patch"]}, top_k=shape["top_k"], beta=50.0,
                              augment=AUGMENT, lr_masks=LR_MASKS)


def rate(n, seconds):
    return round(n / seconds, 2)


def spread(ms):
    """Median, min and max over the timed windows of the ms per batch (and the median as batches/s)."""
    med, lo, hi = _common.spread(ms)
    return dict(ms_median=round(med, 3), ms_min=round(lo, 3), ms_max=round(hi, 3), per_s_median=round(1e3 / med, 1), windows=len(ms))


def window(est_ms):
    """Batches per timed window: at least MIN_WINDOW_S of work, and at least 8 batches."""
    return max(8, int(np.ceil(1e3 * MIN_WINDOW_S / max(est_ms, 1e-3))))


def ms_per_call(fn, batches, sync=False):
    import torch
    t0 = time.perf_counter()
    for idx in batches:
        fn(idx)
    if sync:
        torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / len(batches)


def prefetcher_period(ds, batches, min_L, threads, consumer_ms=0.0, drop=4):
    """Steady-state ms between two batches that BatchPrefetcher hands to a consumer spending `consumer_ms` per batch (asleep,
    GIL released, like a consumer that waits on the GPU).  Timed from the take of batch `drop` to the take of the last one, so
    the thread start, stream creation and first pinned / device allocations of the prefetcher stay outside the window."""
    import torch
    import DataLoader as DL
    taken = []
    for _ in DL.BatchPrefetcher(ds, batches, min_L, device="cuda", n_threads=threads):
        taken.append(time.perf_counter())
        if consumer_ms:
            time.sleep(consumer_ms / 1e3)
    torch.cuda.synchronize()
    return 1e3 * (taken[-1] - taken[drop]) / (len(taken) - 1 - drop)


def measure(dirs, shape, threads, repeats, steps_ms):
    """Every rate below is the spread of `repeats` windows of at least MIN_WINDOW_S each, after an untimed warm-up of the same
    calls (page cache, library, pinned-memory and device caching allocators, the prefetcher's thread and stream)."""
    import torch
    from hrnet_hip import io_binding
    ds = dataset(dirs, shape)
    B, min_L, P = shape["B"], shape["min_L"], 128 if FULL_FRAMES else shape["patch"]
    out = dict(shape)
    seeds = iter(range(1000))
    batches = lambda n: batch_lists(len(dirs), B, n, next(seeds))
    # warm-up of the host path, also the estimate of a window's length
    est = ms_per_call(lambda idx: ds.load_batch(idx, min_L, n_threads=threads), batches(6))
    for pin in (False, True):
        ms_per_call(lambda idx: ds.load_batch(idx, min_L, pin_memory=pin, n_threads=threads), batches(4))
    n = window(est)
    # host path, planning and decoding apart
    buf = dict(lrs=np.empty((B, min_L, P, P), np.float32), alphas=np.empty((B, min_L), np.float32),
               hrs=np.empty((B, 3 * P, 3 * P), np.float32), maps=np.empty((B, 3 * P, 3 * P), np.float32))
    if LR_MASKS:
        buf["lr_masks"] = np.empty((B, min_L, P, P), np.float32)
    plan_ms, dec_ms = [], []
    for _ in range(repeats):
        t_plan = t_dec = 0.0
        for idx in batches(n):
            t0 = time.perf_counter()
            plans = [ds._plan(ds.imset_dir[i]) for i in idx]
            t1 = time.perf_counter()
            io_binding.collate([p["lr_paths"] for p in plans], [p["hr"] for p in plans], [p["sm"] for p in plans], min_L=min_L,
                               lr_size=plans[0]["lr_side"], patch=0 if FULL_FRAMES else P, corners=[p["corner"] for p in plans], out=buf,
                               n_threads=threads, codes=[p["code"] for p in plans] if AUGMENT else None,
                               qm_paths_per_set=[p["qm_paths"] for p in plans] if LR_MASKS else None)
            t_dec += time.perf_counter() - t1
            t_plan += t1 - t0
        plan_ms.append(1e3 * t_plan / n)
        dec_ms.append(1e3 * t_dec / n)
    out["host_plan"] = spread(plan_ms)
    out["host_decode"] = spread(dec_ms)
    out["host_load_batch"] = spread([ms_per_call(lambda idx: ds.load_batch(idx, min_L, n_threads=threads), batches(n))
                                     for _ in range(repeats)])
    out["host_load_batch_pinned"] = spread([ms_per_call(lambda idx: ds.load_batch(idx, min_L, pin_memory=True, n_threads=threads),
                                                        batches(n)) for _ in range(repeats)])
    prefetcher_period(ds, batches(8), min_L, threads)                         # untimed: the first prefetcher of the process
    out["host_prefetcher_idle"] = spread([prefetcher_period(ds, batches(4 + n), min_L, threads) for _ in range(repeats)])
    for step in steps_ms:
        m = window(step)
        out[f"host_prefetcher_step_{step:g}ms"] = spread([prefetcher_period(ds, batches(4 + m), min_L, threads, consumer_ms=step)
                                                          for _ in range(repeats)])
    # device path
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    cache = ds.to_device("cuda", n_threads=threads)
    torch.cuda.synchronize()
    out["cache_build_s"] = round(time.perf_counter() - t0, 3)
    out["cache_nbytes"] = cache.nbytes
    out["cache_sets"] = len(cache)
    est = ms_per_call(lambda idx: cache.load_batch(idx, min_L), batches(40), sync=True)     # warm-up
    n = window(est)
    out["cache_load_batch"] = spread([ms_per_call(lambda idx: cache.load_batch(idx, min_L), batches(n), sync=True)
                                      for _ in range(repeats)])

    def through_batches(lists):
        t0 = time.perf_counter()
        for _ in cache.batches(lists, min_L):
            pass
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / len(lists)

    out["cache_batches"] = spread([through_batches(batches(n)) for _ in range(repeats)])
    # the planner alone (Python, RNG, plan table): what the device path costs the host per batch
    out["cache_plan"] = spread([ms_per_call(lambda idx: cache.index.plan(idx, min_L), batches(n)) for _ in range(repeats)])
    out["output_bytes_per_batch"] = 4 * B * ((2 if LR_MASKS else 1) * min_L * P * P + min_L + 2 * 9 * P * P)
    return out


def kernel_only(dirs, threads, n_batches):
    """Child under rocprofv3: build the cache and launch `n_batches` batches per shape."""
    import torch
    for shape in SHAPES:
        cache = dataset(dirs, shape).to_device("cuda", n_threads=threads)
        for idx in batch_lists(len(dirs), shape["B"], n_batches, 3):
            cache.load_batch(idx, shape["min_L"])
        torch.cuda.synchronize()
        del cache


def kernel_stats(data_dir, threads, n_batches):
    """Per shape in turn the kernel names are the same, so the two shapes run as two child processes."""
    res = {}
    for k, shape in enumerate(SHAPES):
        with tempfile.TemporaryDirectory() as prof:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", prof, "-o", "lr", "--",
                   sys.executable, os.path.abspath(__file__), "--child", data_dir, "--threads", str(threads), "--shape", str(k),
                   "--batches", str(n_batches)] + (["--augment", AUGMENT] if AUGMENT else []) + (["--lr-masks"] if LR_MASKS else []) + (
                       ["--full-frames"] if FULL_FRAMES else [])
            r = subprocess.run(cmd, cwd=prof, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                raise RuntimeError(f"rocprofv3 run failed ({r.returncode}): {r.stderr[-2000:]}")
            files = glob.glob(os.path.join(prof, "**", "*kernel_stats.csv"), recursive=True)
            if not files:
                raise RuntimeError("rocprofv3 wrote no kernel_stats.csv")
            for row in csv.DictReader(open(files[0])):
                if "collate_kernel" in row["Name"] or "collate_mask_kernel" in row["Name"]:
                    res[f"B{shape['B']}_minL{shape['min_L']}"] = dict(name=row["Name"], calls=int(row["Calls"]),
                                                                     avg_us=round(float(row["AverageNs"]) / 1e3, 2),
                                                                     min_us=round(float(row["MinNs"]) / 1e3, 2),
                                                                     max_us=round(float(row["MaxNs"]) / 1e3, 2))
    return res


PARSER = _common.parser(__doc__, sets=64, threads=16, json=None, no_prof=False, batches=200, repeats=5, lr_masks=False, full_frames=False,
                        kernel_only=False)
PARSER.add_argument("--augment", default=None, choices=["flip", "dihedral"])
PARSER.add_argument("--child", default=None, help=argparse.SUPPRESS)                   # kernel_stats' child under rocprofv3: the data directory
PARSER.add_argument("--shape", type=int, default=None, help=argparse.SUPPRESS)         # ... and which of SHAPES it runs


def main():
    a = PARSER.parse_args()
    global AUGMENT, LR_MASKS, FULL_FRAMES
    AUGMENT, LR_MASKS, FULL_FRAMES = a.augment, a.lr_masks, a.full_frames
    _common.require_gpu("loader_rate")
    if a.child:
        dirs = sorted(glob.glob(os.path.join(a.child, "imgset*")))
        global SHAPES
        SHAPES = [SHAPES[a.shape]] if a.shape is not None else SHAPES
        kernel_only(dirs, a.threads, a.batches)
        return
    from hrnet_hip import binding, io_binding
    binding.load_library()
    io_binding.load_library()
    with tempfile.TemporaryDirectory() as root:
        t0 = time.perf_counter()
        dirs = write_imagesets(root, a.sets)
        lr_png = [os.path.getsize(p) for p in glob.glob(os.path.join(root, "*", "LR*.png"))]
        res = dict(sets=a.sets, threads=a.threads, augment=a.augment, lr_masks=a.lr_masks, full_frames=a.full_frames, synthetic_pngs=True, write_s=round(time.perf_counter() - t0, 1),
                   lr_views=len(lr_png), lr_png_kb=round(np.mean(lr_png) / 1024, 1),
                   hr_png_kb=round(np.mean([os.path.getsize(os.path.join(d, "HR.png")) for d in dirs]) / 1024, 1),
                   repeats=a.repeats, min_window_s=MIN_WINDOW_S,
                   shapes=[] if a.kernel_only else [measure(dirs, s, a.threads, a.repeats, STEPS_MS if k == 0 else ())
                                                    for k, s in enumerate(SHAPES)])
        if not a.no_prof:
            res["collate_kernel"] = kernel_stats(root, a.threads, a.batches)
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
