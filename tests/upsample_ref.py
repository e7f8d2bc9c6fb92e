"""The fp64 numpy restatement of hrn_upsample / hrn_upsample_backward (include/hrnet_hip.h): per-axis matrices of the bicubic
interpolation at an integer scale, forward M_H f M_W^T, adjoint M_H^T g M_W, and the sums of absolute terms T of the project's bound
|got - want| <= C T.  rounded=True takes the tap weights through fp32 as the library does (the device and this file then share their
weights and differ in summation alone); rounded=False keeps them in fp64, for the comparison with torch's own bicubic."""
import numpy as np


def phase_weights(scale, a, rounded=True):
    """-> (i (scale,) int, w (scale, 4) fp64): phase p of an axis reads the source indices m + i[p] - 1 .. m + i[p] + 2 with weights w[p]"""
    a = float(np.float32(a)) if rounded else float(a)
    w1 = lambda x: ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0
    w2 = lambda x: ((a * x - 5.0 * a) * x + 8.0 * a) * x - 4.0 * a
    i = np.zeros(scale, np.int64)
    w = np.zeros((scale, 4), np.float64)
    for p in range(scale):
        x = (p + 0.5) / scale - 0.5
        i[p] = int(np.floor(x))
        t = x - i[p]
        w[p] = (w2(t + 1.0), w1(t), w1(1.0 - t), w2(2.0 - t))
    return i, (w.astype(np.float32).astype(np.float64) if rounded else w)


def axis_matrix(n, scale, a, rounded=True):
    """(scale n, n) fp64: row j holds output j's four tap weights at the CLAMPED source indices (taps that clamp onto one index add up)"""
    i, w = phase_weights(scale, a, rounded)
    M = np.zeros((scale * n, n), np.float64)
    for j in range(scale * n):
        m, p = divmod(j, scale)
        for c in range(4):
            M[j, min(max(m + i[p] - 1 + c, 0), n - 1)] += w[p, c]
    return M


def _mats(H, W, scale, a, rounded):
    return axis_matrix(H, scale, a, rounded), axis_matrix(W, scale, a, rounded)


def forward(f, scale, a=-0.75, base=None, rounded=True):
    """f (..., H, W) -> (..., scale H, scale W) fp64 = base + M_H f M_W^T"""
    f = np.asarray(f, np.float64)
    MH, MW = _mats(f.shape[-2], f.shape[-1], scale, a, rounded)
    out = MH @ f @ MW.T
    return out if base is None else out + np.asarray(base, np.float64)


def adjoint(g, scale, a=-0.75, rounded=True):
    """g (..., scale H, scale W) -> (..., H, W) fp64 = M_H^T g M_W"""
    g = np.asarray(g, np.float64)
    MH, MW = _mats(g.shape[-2] // scale, g.shape[-1] // scale, scale, a, rounded)
    return MH.T @ g @ MW


def t_forward(f, scale, a=-0.75, base=None):
    """the sum of the absolute terms of every output element: |M_H| |f| |M_W|^T (+ |base|)"""
    f = np.asarray(f, np.float64)
    MH, MW = _mats(f.shape[-2], f.shape[-1], scale, a, True)
    T = np.abs(MH) @ np.abs(f) @ np.abs(MW).T
    return T if base is None else T + np.abs(np.asarray(base, np.float64))


def t_adjoint(g, scale, a=-0.75):
    g = np.asarray(g, np.float64)
    MH, MW = _mats(g.shape[-2] // scale, g.shape[-1] // scale, scale, a, True)
    return np.abs(MH).T @ np.abs(g) @ np.abs(MW)
