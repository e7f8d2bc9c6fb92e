"""What the cSSIM tests share (tests/test_gpu_cssim.py, tests/test_gpu_cssim_pin.py on the GPU, tests/test_cssim_pin_host.py on the CPU):
the scene and reference caches, the call through `binding.shift_cssim`, the comparison of every offset's score, `out` and `stats` with the
fp64 restatement (tests/cssim_ref.py), and the cases of the pinning pass with their bounds - the CPU test proves about each GPU case
what the GPU test relies on, so both read the cases from here."""
import numpy as np

import cssim_ref as R
from kernel_bounds import CSSIM_BOUND, CSSIM_TOL_PIN

TH, TW = 16, {"gaussian": 54, "uniform": 58}          # csrc/cssim.hip: CS_TH, CS_WIN - T + 1
TOL = 2e-6                                            # tests/test_gpu_cssim.py's bound (its docstring)
SHIFT = (1, -2)
PIN_GAP = 10 * CSSIM_BOUND                            # k* is compared where the restatement's best offset leads by this much

_scenes, _refs = {}, {}


def scene_batch(B, H, W, seed=0):
    """B samples of cssim_ref.scene (15 % holes and a blob), computed once"""
    key = (B, H, W, seed)
    if key not in _scenes:
        xs = [R.scene(1000 * seed + 17 * H + W + b, H, W, SHIFT) for b in range(B)]
        _scenes[key] = tuple(np.stack([x[i] for x in xs]) for i in range(3))
    return _scenes[key]


def clear_batch(B, H, W, level, contrast, mask, seed=0):
    """B samples of cssim_ref.scene_clear, computed once"""
    key = (B, H, W, level, contrast, mask, seed)
    if key not in _scenes:
        xs = [R.scene_clear(1000 * seed + 17 * H + W + b, H, W, level, contrast, mask, SHIFT) for b in range(B)]
        _scenes[key] = tuple(np.stack([x[i] for x in xs]) for i in range(3))
    return _scenes[key]


def ref(x, border, window, clip=True, correct_bias=True, data_range=1.0, key=None):
    """the restatement per sample, computed once per input set: -> (scores (B,nk), k (B,), bias (B,nk), n (B,nk))"""
    key = (key, border, window, clip, correct_bias, data_range)
    if key[0] is None or key not in _refs:
        rs = [R.shift_cssim(s, h, m, border, window, clip, correct_bias, data_range) for s, h, m in zip(*x)]
        out = tuple(np.stack([np.asarray(r[i]) for r in rs]) for i in range(4))
        if key[0] is None:
            return out
        _refs[key] = out
    return _refs[key]


def gpu(x, border, window, **kw):
    import util
    from hrnet_hip import binding
    out, stats, scores = binding.shift_cssim(*(util.dev(a) for a in x), border_w=border, window=window, **kw)
    return out.cpu().numpy(), stats.cpu().numpy(), scores.cpu().numpy()


def compare(x, border, window, what, key=None, tol=TOL, min_gap=1e-3, got=None, **kw):
    """every offset's score, then out / stats; -> the largest |difference| of a finite score.  got: a result of `gpu` to compare instead
    of a new call's."""
    scores, k, bias, n = ref(x, border, window, key=key, **kw)
    out, stats, got = gpu(x, border, window, **kw) if got is None else got
    fin = np.isfinite(scores)
    assert np.array_equal(np.isneginf(got), np.isneginf(scores)), what
    assert np.array_equal(np.isnan(got), np.isnan(scores)), what
    err = float(np.abs(got[fin] - scores[fin]).max()) if fin.any() else 0.0
    print(f"cssim {what}: max |gpu - fp64| over {fin.sum()} scores = {err:.3e}")
    assert err <= tol, what
    for b in range(len(k)):
        if k[b] < 0:
            assert np.isnan(out[b]) and np.isnan(stats[b, 2]) and tuple(stats[b, [0, 1, 3]]) == (0.0, 0.0, -1.0), (what, b)
            continue
        assert R.gap(scores[b]) >= min_gap, (what, b, "the scene does not separate its best offset: replace the seed")
        assert stats[b, 3] == k[b] and stats[b, 0] == n[b, k[b]], (what, b)
        assert abs(stats[b, 1] - bias[b, k[b]]) <= 1e-12 + 1e-12 * abs(bias[b, k[b]]), (what, b)
        assert abs(stats[b, 2] - scores[b, k[b]]) <= tol and out[b] == np.float32(stats[b, 2]), (what, b)
    return err


# ----------------------------------------------------------------------------- the pinning pass: its cases
# A case is (id, family, scene, B, H, W, border, window); scene is ("holes",) or ("clear", level, contrast, mask).  PIN_SEEDS replaces
# the seed of the scenes whose best offset led the runner-up by less than PIN_GAP.
def map_frame(window, border, rows, cols):
    """the frame whose map is `rows` x `cols`"""
    T = R.TAPS[window]
    return rows + T - 1 + 2 * border, cols + T - 1 + 2 * border


def _pin_cases():
    cases = []
    # 1. conditioning: bright / grey / dark low-contrast frames, clear, with a blob, with the left third masked
    for B, H, W in ((2, 24, 24), (1, 49, 71)):
        for window in ("gaussian", "uniform"):
            for level, contrast, masks in ((0.9, 0.05, R.MASKS), (0.5, 0.05, R.MASKS), (0.05, 0.05, R.MASKS), (0.9, 0.005, ("clear",))):
                for mask in masks:
                    cases.append((f"cond-{H}x{W}-{window}-L{level}-c{contrast}-{mask}", "conditioning", ("clear", level, contrast, mask),
                                  B, H, W, 3, window))
    # 2. every instance the shipped tests leave out: borders 4..7, the map one pixel more than one tile along both axes
    for window in ("gaussian", "uniform"):
        for border in (4, 5, 6, 7):
            H, W = map_frame(window, border, TH + 1, TW[window] + 1)
            scene = ("holes",) if border % 2 == 0 else ("clear", 0.9, 0.05, "blob")
            cases.append((f"inst-b{border}-{window}-{scene[0]}", "instances", scene, 1, H, W, border, window))
    # 3. a tile that is interior along x: 3 x 3 tiles with remainders of 1
    for window in ("gaussian", "uniform"):
        H, W = map_frame(window, 3, 2 * TH + 1, 2 * TW[window] + 1)
        for scene in (("holes",), ("clear", 0.9, 0.05, "edge")):
            cases.append((f"seam-{H}x{W}-{window}-{scene[0]}", "seams", scene, 1, H, W, 3, window))
    # 4. the pre-pass's run of 2048 crop pixels: one short of a run, a run exactly, a run and two pixels (three waves of zeros)
    for h, w in ((23, 89), (32, 64), (25, 82)):
        for window in ("gaussian", "uniform"):
            cases.append((f"runs-{h * w}-{window}", "runs", ("holes",), 1, h + 6, w + 6, 3, window))
    return cases


# id -> the seed that replaces 0 (tests/test_cssim_pin_host.py asserts the gaps)
PIN_SEEDS = {"cond-24x24-gaussian-L0.9-c0.05-blob": 15, "cond-24x24-gaussian-L0.5-c0.05-blob": 1, "cond-24x24-gaussian-L0.9-c0.005-clear": 126,
             "cond-24x24-uniform-L0.9-c0.005-clear": 21, "cond-49x71-uniform-L0.05-c0.05-edge": 1}
PIN_CASES = _pin_cases()
FAMILIES = ("conditioning", "instances", "seams", "runs")


def pin_input(case):
    cid, _, scene, B, H, W, border, window = case
    seed = PIN_SEEDS.get(cid, 0)
    return scene_batch(B, H, W, seed) if scene[0] == "holes" else clear_batch(B, H, W, scene[1], scene[2], scene[3], seed)


def pin_ref(case):
    cid, _, _, B, H, W, border, window = case
    return ref(pin_input(case), border, window, key=("pin", cid))
