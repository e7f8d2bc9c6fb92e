"""The fp64 numpy restatement of hrn_shift_add / hrn_shift_add_backward (include/hrnet_hip.h): per view and axis a dense (S n, n) weight
matrix k(i - (y + d)) built from the fp32 tap coordinate d and the fp32-rounded tap weights the library forms, N += Wy (m x) Wx^T,
D += Wy m Wx^T, the output (N + prior b) / (D + prior) with its fallback, the sums of absolute terms T of the project's bound
|got - want| <= C T, and the adjoint by the transposed matrices.  The device and this file share their weights (and, in the adjoint, the
fp32 decision of the fallback on the fp32 `weight` both are given) and differ in summation alone."""
import numpy as np

MIN_DEN = 2.0 ** -20          # out = base where D + prior is below it
MIN_TAP = 2.0 ** -60          # a tap weight below it is taken as 0
MAX_SHIFT = 256.0             # a tap coordinate at or beyond +-256 is taken as +-256


def kernel(u, sigma):
    """k(u) = exp(-u^2 / (2 sigma^2)) cos^2(pi u / 4) for |u| < 2, else 0; fp64"""
    u = np.asarray(u, np.float64)
    k = np.exp(-(u * u) / (2.0 * sigma * sigma)) * np.cos(np.pi * u / 4.0) ** 2
    return np.where(np.abs(u) < 2.0, k, 0.0)


def tap_coord(shift, scale):
    """-> d (scale,) float32: t_p + shift, formed in fp64 from the fp32 shift, rounded to fp32, clamped to +-256"""
    t = (np.arange(scale, dtype=np.float64) + 0.5) / scale - 0.5
    d = (t + np.float64(np.float32(shift))).astype(np.float32)
    return np.clip(d, np.float32(-MAX_SHIFT), np.float32(MAX_SHIFT))


def round_weights(k):
    """fp64 weights -> what the library keeps: below 2^-60 zero, else rounded to fp32 (returned as fp64)"""
    return np.where(k < MIN_TAP, 0.0, k).astype(np.float32).astype(np.float64)


def taps(shift, scale, sigma):
    """-> (n (scale,) int, w (scale, 4) fp64): phase p reads the view indices m + n[p] - 1 .. m + n[p] + 2 with the weights w[p]"""
    sigma = float(np.float32(sigma))
    d = tap_coord(shift, scale)
    n = np.floor(d)
    f = d.astype(np.float64) - n.astype(np.float64)   # exact in fp64 (not in fp32: d + 1 of a small negative d rounds)
    u = np.arange(-1, 3, dtype=np.float64)[None, :] - f[:, None]
    return n.astype(np.int64), round_weights(kernel(u, sigma))


def axis_matrix(n, scale, shift, sigma, rows=None):
    """(scale n, n) fp64, the DENSE form: element (Y = S m + p, i) = k(i - (m + d_p)) with d_p the shared fp32 coordinate; taps outside
    the frame do not exist.  A non-finite shift gives the zero matrix.  rows: only these output rows Y, (len(rows), n)."""
    rows = range(scale * n) if rows is None else rows
    M = np.zeros((len(rows), n), np.float64)
    if not np.isfinite(np.float32(shift)):
        return M
    sigma = float(np.float32(sigma))
    d = tap_coord(shift, scale).astype(np.float64)
    i = np.arange(n, dtype=np.float64)
    for r, Y in enumerate(rows):
        m, p = divmod(Y, scale)
        M[r] = round_weights(kernel(i - (m + d[p]), sigma))
    return M


def axis_matrix_taps(n, scale, shift, sigma):
    """the same matrix from the four taps per phase (n = floor(d), f = d - n): what the kernel walks"""
    M = np.zeros((scale * n, n), np.float64)
    if not np.isfinite(np.float32(shift)):
        return M
    nn, w = taps(shift, scale, sigma)
    for Y in range(scale * n):
        m, p = divmod(Y, scale)
        for o in range(4):
            i = m + int(nn[p]) + o - 1
            if 0 <= i < n:
                M[Y, i] += w[p, o]
    return M


def _counts(alphas, shifts, b, v):
    return (alphas is None or alphas[b, v] != 0) and bool(np.isfinite(np.asarray(shifts[b, v], np.float32)).all())


def sums(views, masks, alphas, shifts, scale, sigma):
    """-> (N, D, A) (B, S H, S W) fp64: the weighted sums of m x, of m and of |m x|"""
    views = np.asarray(views, np.float64)
    B, V, H, W = views.shape
    N = np.zeros((B, scale * H, scale * W), np.float64)
    D, A = np.zeros_like(N), np.zeros_like(N)
    for b in range(B):
        for v in range(V):
            if not _counts(alphas, shifts, b, v):
                continue
            Wy, Wx = axis_matrix(H, scale, shifts[b, v, 0], sigma), axis_matrix(W, scale, shifts[b, v, 1], sigma)
            m = np.ones((H, W)) if masks is None else (np.asarray(masks[b, v]) != 0).astype(np.float64)
            mx = np.where(m != 0, views[b, v], 0.0)
            N[b] += Wy @ mx @ Wx.T
            D[b] += Wy @ m @ Wx.T
            A[b] += Wy @ np.abs(mx) @ Wx.T
    return N, D, A


def forward(views, masks, alphas, shifts, scale, sigma, prior, base=None):
    """-> (out, D, T, den): out = (N + prior b) / (D + prior) where den = D + prior >= 2^-20, else b; T = (A + prior |b|) / den there
    and |b| in the fallback (an exact copy)"""
    prior = float(np.float32(prior))
    N, D, A = sums(views, masks, alphas, shifts, scale, sigma)
    b = np.zeros_like(N) if base is None else np.asarray(base, np.float64)
    den = D + prior
    ok = den >= MIN_DEN
    safe = np.where(ok, den, 1.0)
    out = np.where(ok, (N + prior * b) / safe, b)
    T = np.where(ok, (A + prior * np.abs(b)) / safe, 0.0)
    return out, D, T, den


def excluded(den):
    """the pixels left out of a comparison: D + prior within a factor of two of the fallback's threshold"""
    return (den >= 2.0 ** -21) & (den <= 2.0 ** -19)


def q_of(d_out, weight, prior):
    """q = d_out / (weight + prior) where the fp32 sum weight + prior >= 2^-20, else 0: -> (q fp64, ok).  weight: the fp32 array the
    backward is given; the decision is the fp32 one the device makes, the quotient fp64 of the fp32 denominator's operands."""
    w32, p32 = np.asarray(weight, np.float32), np.float32(prior)
    ok = (w32 + p32) >= np.float32(MIN_DEN)
    den = w32.astype(np.float64) + np.float64(p32)
    return np.where(ok, np.asarray(d_out, np.float64) / np.where(ok, den, 1.0), 0.0), ok


def adjoint(d_out, weight, masks, alphas, shifts, V, H, W, scale, sigma, prior):
    """-> (d_views, T_views (B,V,H,W), d_base, T_base (B,SH,SW)) fp64: d_views = [counts][clear] Wy^T q Wx, d_base = prior q or d_out"""
    q, ok = q_of(d_out, weight, prior)
    B = q.shape[0]
    dv, Tv = np.zeros((B, V, H, W), np.float64), np.zeros((B, V, H, W), np.float64)
    for b in range(B):
        for v in range(V):
            if not _counts(alphas, shifts, b, v):
                continue
            Wy, Wx = axis_matrix(H, scale, shifts[b, v, 0], sigma), axis_matrix(W, scale, shifts[b, v, 1], sigma)
            m = np.ones((H, W)) if masks is None else (np.asarray(masks[b, v]) != 0).astype(np.float64)
            dv[b, v] = m * (Wy.T @ q[b] @ Wx)
            Tv[b, v] = m * (Wy.T @ np.abs(q[b]) @ Wx)
    p = float(np.float32(prior))
    g = np.asarray(d_out, np.float64)
    return dv, Tv, np.where(ok, p * q, g), np.where(ok, p * np.abs(q), 0.0)
