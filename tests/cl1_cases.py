"""The input sets of tests/test_gpu_cl1_loss.py, shared with tests/test_cl1_host.py, which asserts on the CPU the conditions the GPU
comparisons rely on (no near-tie between the two best offsets, no |e| near a sign flip), so that the GPU file excludes no sample.  The
generators are those of tests/test_gpu_shift_loss.py.  No test logic here."""
import numpy as np
import torch

B = 3
# the tolerances of tests/test_gpu_cl1_loss.py (its docstring): relative on out and the statistics; of the max-norm per element of d_srs
TOL = 1e-5
GRAD_TOL = 1e-6
SHAPES = [(20, 20), (37, 53), (53, 37), (96, 96)]     # one tile; odd and rectangular; two tile rows; three tile rows
BORDERS = [0, 1, 3]
WIDE = [((40, 300), 8), ((70, 139), 5)]               # the widest halo and three tile columns; a second tile column
TALL = [((280, 24), 8), ((1900, 12), 1)]              # one column of 9 tiles, added as one run: eight tiles at a time and a tail of one;
#                                                       one column of 60 tiles, added in runs of 2, of which only the first 30 hold tiles
EPS = (0.0, float(np.float32(1e-3)))                  # the C ABI takes eps as a float: the restatement gets the same number


def random(H, W, seed, lo=0.0, hi=1.0):
    rng = np.random.Generator(np.random.PCG64(seed))
    srs = (lo + (hi - lo) * rng.random((B, H, W))).astype(np.float32)
    hrs = rng.random((B, H, W), dtype=np.float32)
    maps = (rng.random((B, H, W)) > 0.1).astype(np.float32)
    return tuple(torch.from_numpy(x) for x in (srs, hrs, maps))


def planted(H, W, border, seed):
    """srs iid uniform; the hrs window at the planted offset is the SR centre crop + N(0, 1e-3^2), the rest uniform.  One planted offset
    per sample: (0, 2 border), (border, border), (2 border, 0)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    srs = rng.random((B, H, W), dtype=np.float32)
    hrs = rng.random((B, H, W), dtype=np.float32)
    maps = (rng.random((B, H, W)) > 0.1).astype(np.float32)
    h, w = H - 2 * border, W - 2 * border
    plant = [(0, 2 * border), (border, border), (2 * border, 0)]
    for b, (u, v) in enumerate(plant):
        hrs[b, u:u + h, v:v + w] = srs[b, border:border + h, border:border + w] + 1e-3 * rng.standard_normal((h, w)).astype(np.float32)
    return tuple(torch.from_numpy(x) for x in (srs, hrs, maps)), plant


def weighted(H, W, seed):
    """maps in {0, 0.5, 1}: a weight, not a mask"""
    srs, hrs, _ = random(H, W, seed)
    rng = np.random.Generator(np.random.PCG64(seed + 1))
    return srs, hrs, torch.from_numpy(rng.integers(0, 3, (B, H, W)).astype(np.float32) * 0.5)


def case(kind, shape, border):
    """-> ((srs, hrs, maps), clip) of the named input set"""
    H, W = shape
    if kind == "rand":
        return random(H, W, 11 + border), False
    if kind == "clip":
        return random(H, W, 61 + border, -0.2, 1.2), True
    if kind == "plant":
        return planted(H, W, border, 51 + border)[0], False
    if kind == "wide":
        return random(H, W, 95 + border), False
    if kind == "weight":
        return weighted(H, W, 131 + border), False
    raise KeyError(kind)


# every input set the GPU file compares against the restatement: (kind, shape, border)
CASES = ([(kind, shape, border) for kind in ("rand", "clip", "plant") for shape in SHAPES for border in BORDERS]
         + [("wide", shape, border) for shape, border in WIDE] + [("weight", (37, 53), 3), ("weight", (96, 96), 1)]
         + [("rand", shape, border) for shape, border in TALL])
