"""Synthetic PROBA-V imagesets (LRxxx.png / QMxxx.png per view, SM.png, HR.png, clearance.npy) written with a stdlib zlib
PNG writer, so that nothing depends on Pillow."""
import os
import struct
import zlib

import numpy as np


def write_png(path, a, level=1):
    """Non-interlaced grayscale PNG of a 2-D uint8 (8-bit) or uint16 (16-bit, big-endian samples) array, filter type 0."""
    a = np.ascontiguousarray(a)
    depth = 16 if a.dtype == np.uint16 else 8
    rows = a.astype(">u2" if depth == 16 else np.uint8).reshape(a.shape[0], -1).view(np.uint8)
    raw = np.concatenate([np.zeros((a.shape[0], 1), np.uint8), rows], axis=1).tobytes()

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data))

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", a.shape[1], a.shape[0], depth, 0, 0, 0, 0))
                + chunk(b"IDAT", zlib.compress(raw, level)) + chunk(b"IEND", b""))


def write_imageset(root, name, n_views, lr=128, with_hr=True, seed=0, lr_views=None, hr=None):
    """One imageset directory: `n_views` 16-bit LR views (or the given `lr_views`), 8-bit quality maps, an 8-bit status map,
    a 16-bit HR image (or the given `hr`) unless `with_hr` is False, and random clearances."""
    rng = np.random.Generator(np.random.PCG64(seed))
    d = os.path.join(root, name)
    os.makedirs(d)
    for v in range(n_views):
        a = lr_views[v] if lr_views is not None else rng.integers(0, 16000, (lr, lr), dtype=np.uint16)
        if lr_views is None:
            a[3:9, 5:40] = 65535                                   # saturated patch: the top of the 16-bit range
        write_png(os.path.join(d, f"LR{v:03d}.png"), a)
        write_png(os.path.join(d, f"QM{v:03d}.png"), (rng.random((lr, lr)) > 0.2).astype(np.uint8) * 255)
    sm = (rng.random((3 * lr, 3 * lr)) > 0.1) * rng.integers(1, 256, (3 * lr, 3 * lr))   # any non-zero sample counts as clear
    write_png(os.path.join(d, "SM.png"), sm.astype(np.uint8))
    if with_hr:
        write_png(os.path.join(d, "HR.png"), hr if hr is not None else rng.integers(0, 20000, (3 * lr, 3 * lr), dtype=np.uint16))
    np.save(os.path.join(d, "clearance.npy"), rng.random(n_views))
    return d
