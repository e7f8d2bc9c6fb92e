"""The fp64 numpy restatement of the observation model (include/hrnet_hip.h: hrn_observe, hrn_consistency_residual / _finish,
hrn_observe_adjoint): per view and axis a dense (L, S L) matrix whose row i holds the S + 5 weights w_j at the HR indices S i + n - 2 + j
(zero rows where the sample is not valid), built from registration_ref.split / taps; also the tap form, which walks the S point samples
of an LR pixel's box and the six taps of each.  Forward A = Ay x Ax^T, the adjoint by the transposed matrices, the loss with its analytic
gradient, one back-projection step, and for every output T, the sum of the absolute values of its terms, for the project's bound
|got - want| <= C T.  The device and this file share their weights (fp32-rounded) and every decision (floor of an fp32 value, mask tests)
and differ in summation alone."""
import numpy as np

import registration_ref as RR

MAX_COORD = 256.0             # the clamp of split_and_taps; a view whose unclamped |c| reaches it has no valid sample


def coord(shift, scale):
    """c = -S d: fp64 product of the fp32 shift, rounded to fp32 (not clamped)"""
    return np.float32(-np.float64(scale) * np.float64(np.float32(shift)))


def weights_unrounded(f, scale):
    """w_j = (1 / S) sum_k t_{j-2-k}(f), j = 0 .. S + 4, fp64"""
    t = RR.taps(f)
    w = np.zeros(scale + 5, np.float64)
    for k in range(scale):
        w[k:k + 6] += t
    return w / scale


def axis_weights(shift, scale):
    """-> (n int, w (S + 5,) fp64 holding fp32 values, reach bool): the view's weight vector on one axis"""
    c = coord(shift, scale)
    reach = bool(np.abs(c) < MAX_COORD)
    n, f = RR.split(np.clip(c, np.float32(-MAX_COORD), np.float32(MAX_COORD)))
    return n, weights_unrounded(f, scale).astype(np.float32).astype(np.float64), reach


def valid_axis(L, scale, n, reach=True):
    """(L,) bool: sample i is valid iff 0 <= S i + n - 2 and S i + n + S + 2 <= S L - 1"""
    i = np.arange(L, dtype=np.int64)
    return (scale * i + n - 2 >= 0) & (scale * i + n + scale + 2 <= scale * L - 1) & reach


def axis_matrix(L, scale, shift, rows=None):
    """(L, S L) fp64, the DENSE form; a non-finite shift gives the zero matrix.  rows: only these samples i, (len(rows), S L)."""
    rows = range(L) if rows is None else rows
    M = np.zeros((len(rows), scale * L), np.float64)
    if not np.isfinite(np.float32(shift)):
        return M
    n, w, reach = axis_weights(shift, scale)
    ok = valid_axis(L, scale, n, reach)
    for r, i in enumerate(rows):
        if ok[i]:
            M[r, scale * i + n - 2:scale * i + n + scale + 3] = w
    return M


def axis_matrix_taps(L, scale, shift):
    """the same matrix from the definition's words, unrounded: sample i = the mean of S point samples at the HR coordinates
    S (i - d) + k = S i + k + n + f, each read with the six taps t_o(f) at the rows S i + k + n + o"""
    M = np.zeros((L, scale * L), np.float64)
    if not np.isfinite(np.float32(shift)):
        return M
    c = coord(shift, scale)
    n, f = RR.split(np.clip(c, np.float32(-MAX_COORD), np.float32(MAX_COORD)))
    t = RR.taps(f)
    ok = valid_axis(L, scale, n, bool(np.abs(c) < MAX_COORD))
    for i in range(L):
        if not ok[i]:
            continue
        for k in range(scale):
            for o in range(-2, 4):
                M[i, scale * i + k + n + o] += t[o + 2] / scale
    return M


def view_counts(alphas, shifts, b, v):
    return (alphas is None or alphas[b, v] != 0) and bool(np.isfinite(np.asarray(shifts[b, v], np.float32)).all())


def matrices(shifts, b, v, H, W, scale):
    return axis_matrix(H, scale, shifts[b, v, 0]), axis_matrix(W, scale, shifts[b, v, 1])


def valid_map(shifts, b, v, H, W, scale):
    """(H, W) bool"""
    if not np.isfinite(np.asarray(shifts[b, v], np.float32)).all():
        return np.zeros((H, W), bool)
    (ny, _, ry), (nx, _, rx) = axis_weights(shifts[b, v, 0], scale), axis_weights(shifts[b, v, 1], scale)
    return np.outer(valid_axis(H, scale, ny, ry and rx), valid_axis(W, scale, nx, ry and rx))


def forward(hr, shifts, scale):
    """hrn_observe -> (views, valid, T) (B,V,H,W): A_v hr where valid, 0 elsewhere; T = |A_v| |hr|"""
    hr = np.asarray(hr, np.float64)
    B, SH, SW = hr.shape
    V, H, W = shifts.shape[1], SH // scale, SW // scale
    views, T = np.zeros((B, V, H, W)), np.zeros((B, V, H, W))
    valid = np.zeros((B, V, H, W), bool)
    for b in range(B):
        for v in range(V):
            Ay, Ax = matrices(shifts, b, v, H, W, scale)
            views[b, v], T[b, v] = Ay @ hr[b] @ Ax.T, np.abs(Ay) @ np.abs(hr[b]) @ np.abs(Ax).T
            valid[b, v] = valid_map(shifts, b, v, H, W, scale)
    return views, valid, T


def counted_map(lr_shape, masks, alphas, shifts, scale):
    B, V, H, W = lr_shape
    c = np.zeros(lr_shape, bool)
    for b in range(B):
        for v in range(V):
            if view_counts(alphas, shifts, b, v):
                c[b, v] = valid_map(shifts, b, v, H, W, scale) & (True if masks is None else np.asarray(masks[b, v]) != 0)
    return c


def adjoint(r, shifts, scale, T_r=None):
    """-> (G, T_G) (B,SH,SW): G = sum_v Ay^T r_v Ax, T_G the same of |A| and |r| (or of the given T_r).  The matrices' zero rows take
    care of what is not valid; masks and alphas are the caller's (r is 0 where nothing is counted)."""
    r = np.asarray(r, np.float64)
    T_r = np.abs(r) if T_r is None else T_r
    B, V, H, W = r.shape
    G, T = np.zeros((B, scale * H, scale * W)), np.zeros((B, scale * H, scale * W))
    for b in range(B):
        for v in range(V):
            Ay, Ax = matrices(shifts, b, v, H, W, scale)
            G[b] += Ay.T @ r[b, v] @ Ax
            T[b] += np.abs(Ay).T @ T_r[b, v] @ np.abs(Ax)
    return G, T


def loss(srs, lrs, masks, alphas, shifts, scale, brightness=True):
    """-> dict: e, T_e, counted, n (B,V), beta, T_beta (B,V), r, T_r, L, T_L (B,), vb (B,), G, T_G = sum_v A_v^T r_v, grad, T_grad =
    dL_b/dx (B,SH,SW).  T_e = |A| |x| + |y|; T_beta = sum T_e / n; T_r = counted (T_e + T_beta); T_L = sum T_r^2 / sum n."""
    srs, lrs = np.asarray(srs, np.float64), np.asarray(lrs, np.float64)
    B, V, H, W = lrs.shape
    Ax_, _, TA = forward(srs, shifts, scale)
    cm = counted_map(lrs.shape, masks, alphas, shifts, scale)
    e = np.where(cm, Ax_ - lrs, 0.0)
    T_e = np.where(cm, TA + np.abs(lrs), 0.0)
    n = cm.sum((2, 3)).astype(np.float64)
    safe = np.where(n > 0, n, 1.0)
    beta = np.where(n > 0, -e.sum((2, 3)) / safe, 0.0) if brightness else np.zeros((B, V))
    T_beta = np.where(n > 0, T_e.sum((2, 3)) / safe, 0.0) if brightness else np.zeros((B, V))
    r = np.where(cm, e + beta[:, :, None, None], 0.0)
    T_r = np.where(cm, T_e + T_beta[:, :, None, None], 0.0)
    tot = n.sum(1)
    st = np.where(tot > 0, tot, 1.0)
    L = np.where(tot > 0, (r * r).sum((1, 2, 3)) / st, 0.0)
    T_L = np.where(tot > 0, (T_r * T_r).sum((1, 2, 3)) / st, 0.0)
    G, T_G = adjoint(r, shifts, scale, T_r)
    cf = np.where(tot > 0, 2.0 / st, 0.0)[:, None, None]
    return dict(e=e, T_e=T_e, counted=cm, n=n.astype(np.int64), beta=beta, T_beta=T_beta, r=r, T_r=T_r, L=L, T_L=T_L, vb=(n > 0).sum(1), G=G,
                T_G=T_G, grad=cf * G, T_grad=cf * T_G)


def step(x, lrs, masks, alphas, shifts, scale, step=1.0, brightness=True):
    """one back-projection step -> (x', T, L of x): x' = x - step (S^2 / V_b) sum_v A_v^T r_v(x); T = |x| + step (S^2 / V_b) T_G"""
    x = np.asarray(x, np.float64)
    s = loss(x, lrs, masks, alphas, shifts, scale, brightness)
    vb = s["vb"].astype(np.float64)
    cf = np.where(vb > 0, np.float64(np.float32(step)) * scale * scale / np.where(vb > 0, vb, 1.0), 0.0)[:, None, None]
    return x - cf * s["G"], np.abs(x) + cf * s["T_G"], s["L"]


def back_project(x, lrs, masks, alphas, shifts, scale, iters, step_=1.0, brightness=True):
    """-> (x after iters steps, losses (iters, B): the loss of the frame each step started from)"""
    x = np.asarray(x, np.float64)
    losses = np.zeros((iters, x.shape[0]))
    for t in range(iters):
        x, _, losses[t] = step(x, lrs, masks, alphas, shifts, scale, step_, brightness)
    return x, losses


def top_eigenvalue(shape, masks, alphas, shifts, scale, iters=60, seed=0):
    """power iteration on (S^2 / V_b) sum_v A_v^T M_v A_v (brightness off: the projection only lowers it) -> the largest eigenvalue of
    sample 0"""
    B, V, H, W = shape
    rng = np.random.Generator(np.random.PCG64(seed))
    x = rng.standard_normal((1, scale * H, scale * W))
    cm = counted_map(shape, masks, alphas, shifts, scale)
    vb = max(int((cm[0].sum((1, 2)) > 0).sum()), 1)
    lam = 0.0
    for _ in range(iters):
        y = np.where(cm[:1], forward(x, shifts[:1], scale)[0], 0.0)
        z = adjoint(y, shifts[:1], scale)[0] * (scale * scale / vb)
        lam = float(np.sqrt((z * z).sum() / (x * x).sum()))
        x = z / np.sqrt((z * z).sum())
    return lam
