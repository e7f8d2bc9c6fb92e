"""The cases of the observation-model tests (tests/test_observe_host.py on the CPU, tests/test_gpu_observe.py on the device), made once:
the six shapes of tests/shift_add_cases.py x three scales x the seven kinds of shifts, and over them - by a fixed mixing of the case's
index, so that every value meets every scale and every kind of shift - the four kinds of masks, the three kinds of alphas and
`brightness` on / off.  The restatement's results are cached with the case: a reference is computed once and shared.

Shifts are in LR pixels.  "random" draws within 3.5 px where the frame has at least 8 samples a side and within 1 px in the 5 x 7 frames,
so that every view of a non-degenerate case keeps valid samples (a shift of 3.5 px moves the footprint by up to 14 HR pixels)."""
import functools

import numpy as np

import observe_ref as O
import shift_add_cases as SC

TH, TW = SC.TH, SC.TW
SHAPES, SCALES, SHIFTS, MASKS, ALPHAS, EPS = SC.SHAPES, SC.SCALES, SC.SHIFTS, SC.MASKS, SC.ALPHAS, SC.EPS
DEGENERATE = [(2, 1, 1, 1), (1, 3, 2, 5)]            # no sample's S + 5 rows fit into S H: nothing is valid


def plan():
    """-> [(shape, scale, shifts, masks, alphas, brightness)], 126 cases"""
    out = []
    for si, shape in enumerate(SHAPES):
        for ci, scale in enumerate(SCALES):
            for k, kind in enumerate(SHIFTS):
                out.append((shape, scale, kind, MASKS[(k + 2 * ci + si) % 4], ALPHAS[(k + ci + 2 * si) % 3], bool((k + ci + si) % 2)))
    return out


def case_id(c):
    shape, scale, kind, masks, alphas, brightness = c
    return f"{'x'.join(map(str, shape))}-x{scale}-{kind}-{masks}-{alphas}-{'beta' if brightness else 'plain'}"


def special_view(c):
    """the view a case sets apart: the far / NaN one, or None"""
    return c[0][1] // 2 if c[2] in ("far", "nan") else None


def must_count(c, x, b, v):
    """whether view v of sample b has to keep counted pixels: it counts, and the case did not hide or move it away on purpose"""
    shape, scale, kind, mkind, akind, brightness = c
    if shape in DEGENERATE or v == special_view(c) or (mkind == "one-view" and v == shape[1] - 1):
        return False
    if mkind == "block" and min(shape[2:]) < 8:          # in the 5 x 7 frames the hidden block is the whole valid interior at small shifts
        return False
    return O.view_counts(x["alphas"], x["shifts"], b, v)


@functools.lru_cache(maxsize=None)
def inputs(c):
    """-> dict of numpy f32 inputs: hr (B,SH,SW), lrs, masks (or None), alphas (or None), shifts, g (a gradient for the views), gl (one for
    the loss).  A case is drawn again (the next salt of its seed) until every view that must count keeps a counted pixel."""
    for salt in range(64):
        x = _draw(c, salt)
        cm = O.counted_map(x["lrs"].shape, x["masks"], x["alphas"], x["shifts"], c[1])
        B, V = c[0][:2]
        if all(cm[b, v].any() for b in range(B) for v in range(V) if must_count(c, x, b, v)):
            return x
    raise AssertionError(f"{case_id(c)}: no draw in which every counting view keeps a counted pixel")


def _draw(c, salt):
    shape, scale, kind, mkind, akind, brightness = c
    B, V, H, W = shape
    rng = np.random.Generator(np.random.PCG64(1000 * sum((k + 1) * ord(ch) for k, ch in enumerate(case_id(c))) + salt))
    hr = rng.uniform(0.05, 1.0, (B, scale * H, scale * W)).astype(np.float32)
    lrs = rng.uniform(0.05, 1.0, shape).astype(np.float32)
    reach = 3.5 if min(H, W) >= 8 else 1.0
    rand = rng.uniform(-reach, reach, (B, V, 2)).astype(np.float32)
    if kind == "zeros":
        shifts = np.zeros((B, V, 2), np.float32)
    elif kind == "whole":
        shifts = rng.choice(np.array([-2, -1, 1, 2], np.float32), (B, V, 2))
    elif kind == "halves":
        shifts = rng.choice(np.array([-2.5, -1.5, -0.5, 0.5, 1.5, 2.5], np.float32), (B, V, 2))
    elif kind == "whole-eps":
        shifts = (rng.choice(np.array([-2, -1, 0, 1, 2], np.float64), (B, V, 2)) + rng.choice(np.array([-EPS, EPS]), (B, V, 2))).astype(np.float32)
    else:
        shifts = rand
        if kind == "far":
            shifts[:, V // 2] = (300.0, -300.0)
        if kind == "nan":
            shifts[:, V // 2, 1] = np.nan
    masks = None
    if mkind == "random":
        masks = (rng.uniform(0, 1, shape) >= 0.3).astype(np.float32)
    elif mkind == "one-view":
        masks = np.ones(shape, np.float32)
        masks[:, V - 1] = 0
    elif mkind == "block":
        masks = (rng.uniform(0, 1, shape) >= 0.1).astype(np.float32) * rng.choice(np.array([1.0, 2.0, -1.0], np.float32), shape)
        ys, xs = SC.block_of(H, W)
        masks[:, :, ys, xs] = 0
    alphas = None
    if akind == "some-zero":
        alphas = (rng.uniform(0, 1, (B, V)) >= 0.4).astype(np.float32) * rng.choice(np.array([1.0, 0.5], np.float32), (B, V))
        alphas[:, 0] = 1
    elif akind == "sample-zero":
        alphas = np.ones((B, V), np.float32)
        alphas[B - 1] = 0
    g = rng.uniform(-1, 1, shape).astype(np.float32)
    gl = rng.uniform(0.5, 2.0, (B,)).astype(np.float32)
    return dict(hr=hr, lrs=lrs, masks=masks, alphas=alphas, shifts=shifts, g=g, gl=gl)


@functools.lru_cache(maxsize=None)
def reference(c):
    """-> dict of the restatement's results: views, valid, T_views (hrn_observe); everything of observe_ref.loss; d_srs, T_d_srs (the
    loss' gradient times gl); d_hr, T_d_hr (observe's backward at g); x1, T_x1 (one back-projection step, step 1)"""
    shape, scale, kind, mkind, akind, brightness = c
    x = inputs(c)
    views, valid, T_views = O.forward(x["hr"], x["shifts"], scale)
    out = dict(views=views, valid=valid, T_views=T_views)
    out.update(O.loss(x["hr"], x["lrs"], x["masks"], x["alphas"], x["shifts"], scale, brightness))
    gl = x["gl"].astype(np.float64)[:, None, None]
    out["d_srs"], out["T_d_srs"] = gl * out["grad"], gl * out["T_grad"]
    out["d_hr"], out["T_d_hr"] = O.adjoint(np.where(valid, x["g"].astype(np.float64), 0.0), x["shifts"], scale)
    out["x1"], out["T_x1"], _ = O.step(x["hr"], x["lrs"], x["masks"], x["alphas"], x["shifts"], scale, 1.0, brightness)
    return out
