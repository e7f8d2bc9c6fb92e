"""The fp64 numpy restatement of the observation model's derivative in the shifts (include/hrnet_hip.h: hrn_observe_shift_grad,
hrn_shift_normal, hrn_shift_normal_finish), on observe_ref's matrices: per view and axis a second dense (L, S L)
matrix whose row i holds the S + 5 derivative weights omega_j = -sum_k k'_{j-2-k}(f) where observe_ref's holds w_j, k' being
warp_ref.dtaps' formula.  From them the derivative images D_y = Oy x Ax^T, D_x = Ay x Ox^T, the gradients to the shifts of `observe` and of the
consistency loss, the normal equations of a view, the damped Gauss-Newton update, and the alternating scheme (one data step, one shift
step) that `reconstruct_joint` runs.  Every output comes with T, the same sums over absolute values, for the bound |got - want| <= C T;
the T of a centred quantity is built from its UNCENTRED terms (the centred ones cancel).

`variant` turns one part of the definition into the mistake that part guards against (the tests' controls): "w" (w in place of omega),
"sign" (omega's sign), "nonorm" (k' without its normalisation term), "uncentred" (D not centred with `brightness`), "swap" (dy / dx).
No test logic here."""
import numpy as np

import observe_ref as O
import registration_ref as RR
import robust_ref as RB
import warp_ref as WR

MIN_WEIGHT = 3.0              # a view whose sum p is below this keeps its shift
VARIANTS = ("w", "sign", "nonorm", "uncentred", "swap")


_LD = np.longdouble
_PI = _LD("3.14159265358979323846264338327950288")


def _sinc_ld(t):
    """sinc and sinc' in extended precision; warp_ref's series below |t| = 1e-2"""
    z = _PI * t
    safe = np.where(t == 0, _LD(1), t)
    s = np.where(t == 0, _LD(1), np.sin(_PI * safe) / (_PI * safe))
    ds = np.where(np.abs(t) < _LD("1e-2"), _PI * z * (-_LD(1) / 3 + z * z * (_LD(1) / 30 - z * z / 840)), (np.cos(z) - s) / safe)
    return s, ds


def dtaps(f, normalise=True):
    """warp_ref.dtaps - k'_o = (u'_o - k_o sum u') / sum u - evaluated in extended precision and rounded to fp64 once, so that each tap
    is (nearly) the correctly rounded value and their sum is 0 to the rounding of six values of order 1.  (warp_ref's fp64 evaluation
    carries a few ulps per tap; the two agree to 1e-15, tests/test_observe_shift_host.py.)"""
    x = RR.TAPS.astype(_LD) - _LD(np.float64(f))
    a, da = _sinc_ld(x)
    b, db = _sinc_ld(x / 3)
    out = np.abs(x) >= 3
    u, du = np.where(out, _LD(0), a * b), np.where(out, _LD(0), -(da * b + a * db / 3))
    k = du / u.sum() if not normalise else (du - (u / u.sum()) * du.sum()) / u.sum()
    return k.astype(np.float64)


def slopes_unrounded(f, scale, variant=None):
    """omega_j = dw_j / dd = -sum_k k'_{j-2-k}(f), j = 0 .. S + 4, fp64 (c = -S d: the S cancels the box mean's 1 / S)"""
    if variant == "w":
        return O.weights_unrounded(f, scale)
    dk = dtaps(f, normalise=variant != "nonorm")
    om = np.zeros(scale + 5, np.float64)
    for k in range(scale):
        om[k:k + 6] -= dk
    return -om if variant == "sign" else om


def axis_slopes(shift, scale, variant=None):
    """-> omega (S + 5,) fp64 holding fp32 values"""
    c = O.coord(shift, scale)
    n, f = RR.split(np.clip(c, np.float32(-O.MAX_COORD), np.float32(O.MAX_COORD)))
    return slopes_unrounded(f, scale, variant).astype(np.float32).astype(np.float64)


def slope_matrix(L, scale, shift, rows=None, variant=None):
    """observe_ref.axis_matrix with omega in place of w: (L, S L) fp64, zero rows where the sample is not valid or the shift not finite"""
    rows = range(L) if rows is None else rows
    M = np.zeros((len(rows), scale * L), np.float64)
    if not np.isfinite(np.float32(shift)):
        return M
    n, _, reach = O.axis_weights(shift, scale)
    om = axis_slopes(shift, scale, variant)
    ok = O.valid_axis(L, scale, n, reach)
    for r, i in enumerate(rows):
        if ok[i]:
            M[r, scale * i + n - 2:scale * i + n + scale + 3] = om
    return M


def derivative(hr, shifts, scale, variant=None):
    """-> (D (B,V,2,H,W), T_D): D[:, :, 0] = D_y, [:, :, 1] = D_x, 0 where not valid; T_D = |omega| |w| |x|"""
    hr = np.asarray(hr, np.float64)
    B, SH, SW = hr.shape
    V, H, W = shifts.shape[1], SH // scale, SW // scale
    D, T = np.zeros((B, V, 2, H, W)), np.zeros((B, V, 2, H, W))
    for b in range(B):
        for v in range(V):
            ok = O.valid_map(shifts, b, v, H, W, scale)
            if not ok.any():
                continue
            Ay, Ax = O.matrices(shifts, b, v, H, W, scale)
            Oy, Ox = slope_matrix(H, scale, shifts[b, v, 0], variant=variant), slope_matrix(W, scale, shifts[b, v, 1], variant=variant)
            x, ax = hr[b], np.abs(hr[b])
            pair = [(Oy @ x @ Ax.T, np.abs(Oy) @ ax @ np.abs(Ax).T), (Ay @ x @ Ox.T, np.abs(Ay) @ ax @ np.abs(Ox).T)]
            if variant == "swap":
                pair = pair[::-1]
            for a in range(2):
                D[b, v, a], T[b, v, a] = np.where(ok, pair[a][0], 0.0), np.where(ok, pair[a][1], 0.0)
    return D, T


def d_shifts_observe(hr, g, shifts, scale, variant=None):
    """observe's backward to the shifts -> (d_shifts (B,V,2), T): sum over valid i of g_i D_a,i"""
    D, T_D = derivative(hr, shifts, scale, variant)
    _, valid, _ = O.forward(hr, shifts, scale)
    gv = np.where(valid, np.asarray(g, np.float64), 0.0)[:, :, None]
    return (gv * D).sum((3, 4)), (np.abs(gv) * T_D).sum((3, 4))


def d_shifts_loss(hr, lrs, masks, alphas, shifts, scale, brightness=True, gain=None, variant=None, s=None):
    """the consistency loss' gradient to the shifts -> (d_shifts (B,V,2), T): gain_b (2 / sum n) sum counted r_i D_a,i"""
    s = O.loss(hr, lrs, masks, alphas, shifts, scale, brightness) if s is None else s
    D, T_D = derivative(hr, shifts, scale, variant)
    tot = s["n"].sum(1).astype(np.float64)
    cf = np.where(tot > 0, 2.0 / np.where(tot > 0, tot, 1.0), 0.0) * (1.0 if gain is None else np.asarray(gain, np.float64))
    cf = cf[:, None, None]
    return cf * (s["r"][:, :, None] * D).sum((3, 4)), np.abs(cf) * (s["T_r"][:, :, None] * T_D).sum((3, 4))


def normal(hr, lrs, masks, alphas, shifts, scale, brightness=True, beta_prev=None, delta=0.1, variant=None, s=None):
    """-> (normal (B,V,8) = [P, g_y, g_x, H_yy, H_yx, H_xx, beta, q], T (B,V,8)).  beta_prev (B,V): Welsch weights of e + beta_prev.
    T: every sum with p -> T_p (p itself in plain mode, robust_ref's T_w otherwise), e -> T_e, D -> T_D, beta -> T_beta, each minus a plus;
    a quotient by P keeps P, times T_P / P where p itself carries an error (the quotient's own first-order term)."""
    s = O.loss(hr, lrs, masks, alphas, shifts, scale, brightness) if s is None else s
    D, T_D = derivative(hr, shifts, scale, variant)
    cm, e, T_e = s["counted"], s["e"], s["T_e"]
    if beta_prev is None:
        p = cm.astype(np.float64)
        T_p = p
    else:
        rt = RB.robust_terms(s, beta_prev, np.abs(np.asarray(beta_prev, np.float64)), delta, brightness)
        p, T_p = rt["w"], rt["T_w"]
    D = np.where(cm[:, :, None], D, 0.0)
    T_D = np.where(cm[:, :, None], T_D, 0.0)
    sm = lambda a: a.sum((-2, -1))
    P, T_P = sm(p), sm(T_p)
    live = P >= RB.MIN_WEIGHT
    safe = np.where(live, P, 1.0)
    centre = live & bool(brightness)
    Se, T_Se, See = sm(p * e), sm(T_p * T_e), sm(p * e * e)
    Sa, T_Sa = sm(p[:, :, None] * D), sm(T_p[:, :, None] * T_D)                       # (B,V,2)
    Sea, T_Sea = sm((p * e)[:, :, None] * D), sm((T_p * T_e)[:, :, None] * T_D)
    Sab = np.stack([sm(p * D[:, :, 0] * D[:, :, 0]), sm(p * D[:, :, 0] * D[:, :, 1]), sm(p * D[:, :, 1] * D[:, :, 1])], -1)
    T_Sab = np.stack([sm(T_p * T_D[:, :, 0] * T_D[:, :, 0]), sm(T_p * T_D[:, :, 0] * T_D[:, :, 1]), sm(T_p * T_D[:, :, 1] * T_D[:, :, 1])], -1)
    infl = np.where(live, T_P / safe, 1.0)
    beta = np.where(centre, -Se / safe, 0.0)
    T_beta = np.where(centre, T_Se / safe * infl, 0.0)
    uncentred = variant == "uncentred"
    m = np.where(centre[..., None] & (not uncentred), Sa / safe[..., None], 0.0)
    T_m = np.where(centre[..., None], T_Sa / safe[..., None] * infl[..., None], 0.0)
    rest = Se + beta * P
    g = Sea + beta[..., None] * Sa - m * rest[..., None]
    T_g = T_Sea + T_beta[..., None] * T_Sa + T_m * (T_Se + T_beta * T_P)[..., None]
    ia, ib = np.array([0, 0, 1]), np.array([0, 1, 1])
    Hm = Sab - m[..., ia] * Sa[..., ib]
    T_H = T_Sab + T_m[..., ia] * T_Sa[..., ib]
    q = See + 2.0 * beta * Se + beta * beta * P
    T_q = sm(T_p * (T_e + T_beta[:, :, None, None]) ** 2)
    out = np.concatenate([P[..., None], g, Hm, beta[..., None], np.maximum(q, 0.0)[..., None]], -1)
    T = np.concatenate([T_P[..., None], T_g, T_H, T_beta[..., None], T_q[..., None]], -1)
    return out, T


def view_kept(alphas, shifts, scale, fixed=None):
    """(B,V) bool: the views whose shift the update may not touch whatever their sums: fixed, not counting, or out of reach"""
    B, V = shifts.shape[:2]
    keep = np.zeros((B, V), bool)
    for b in range(B):
        for v in range(V):
            reach = O.view_counts(alphas, shifts, b, v) and all(np.abs(O.coord(shifts[b, v, a], scale)) < O.MAX_COORD for a in range(2))
            keep[b, v] = not reach or (fixed is not None and bool(fixed[b, v]))
    return keep


def update(nrm, shifts, keep, damping=1e-3, max_step=0.5):
    """the Levenberg-damped Gauss-Newton step in fp64 from normal (B,V,8) -> (shifts' (B,V,2) f32 with kept views' BITS, step (B,V,2) fp64,
    moved (B,V) bool).  damping and max_step are taken as the fp32 values the C ABI receives."""
    damping, max_step = np.float64(np.float32(damping)), np.float64(np.float32(max_step))
    shifts = np.asarray(shifts, np.float32)
    out = shifts.copy()
    B, V = shifts.shape[:2]
    steps, moved = np.zeros((B, V, 2)), np.zeros((B, V), bool)
    for b in range(B):
        for v in range(V):
            P, gy, gx, Hyy, Hyx, Hxx = (np.float64(t) for t in nrm[b, v, :6])
            if keep[b, v] or not P >= MIN_WEIGHT:
                continue
            lam = damping * (Hyy + Hxx) * 0.5
            a, d = Hyy + lam, Hxx + lam
            det = a * d - Hyx * Hyx
            if not (det > 0.0 and np.isfinite(det)):
                continue
            sy, sx = -(d * gy - Hyx * gx) / det, -(a * gx - Hyx * gy) / det
            m = max(abs(sy), abs(sx))
            if m > max_step:
                sy, sx = sy * (max_step / m), sx * (max_step / m)
            if not (np.isfinite(sy) and np.isfinite(sx)):
                continue
            steps[b, v], moved[b, v] = (sy, sx), True
            out[b, v] = np.float32(np.float64(shifts[b, v, 0]) + sy), np.float32(np.float64(shifts[b, v, 1]) + sx)
    return out, steps, moved


def fixed_mask(fixed, B, V):
    """`fixed` as the Python functions take it - a view index, None, or (B,V) bool - -> (B,V) bool"""
    if fixed is None:
        return np.zeros((B, V), bool)
    if np.ndim(fixed) == 0:
        m = np.zeros((B, V), bool)
        m[:, int(fixed)] = True
        return m
    return np.asarray(fixed, bool)


def refine_shifts(sr, lrs, masks, alphas, shifts, scale, iters=2, damping=1e-3, max_step=0.5, fixed=0, brightness=True):
    """`iters` Gauss-Newton steps on the shifts with the frame held (plain weights) -> shifts' f32"""
    shifts = np.asarray(shifts, np.float32)
    fm = fixed_mask(fixed, *shifts.shape[:2])
    for _ in range(iters):
        nrm, _ = normal(sr, lrs, masks, alphas, shifts, scale, brightness)
        shifts, _, _ = update(nrm, shifts, view_kept(alphas, shifts, scale, fm), damping, max_step)
    return shifts


def reconstruct_joint(x, lrs, masks, alphas, shifts, scale, iters=30, refine_every=1, refine_from=1, damping=1e-3, max_step=0.5, fixed=0,
                      step=1.0, brightness=True, robust=False, delta=0.1, lam=0.0, P=2, alpha=0.7, eps=0.02):
    """robust_ref.reconstruct's loop with a shift update beside the data step of iteration t (0-based) when refine_every > 0,
    t >= refine_from and (t - refine_from) % refine_every == 0 - and, in Welsch mode, t >= 1, since the update's weights need a
    beta_prev.  Both read the frame and the shifts the iteration started from -> (x, shifts f32)."""
    x = np.asarray(x, np.float64)
    shifts = np.asarray(shifts, np.float32)
    fm = fixed_mask(fixed, *shifts.shape[:2])
    state = None
    c = np.float64(np.float32(np.float64(step) * np.float64(lam)))
    for t in range(iters):
        refine = refine_every > 0 and t >= refine_from and (t - refine_from) % refine_every == 0 and not (robust and t == 0)
        new = shifts
        if refine:
            nrm, _ = normal(x, lrs, masks, alphas, shifts, scale, brightness, state[0] if robust else None, delta)
            new, _, _ = update(nrm, shifts, view_kept(alphas, shifts, scale, fm), damping, max_step)
        x, _, info = RB.data_step(x, lrs, masks, alphas, shifts, scale, step, brightness, robust, delta, state)
        state = info["state"]
        if lam > 0:
            x, _ = RB.btv_step(x, c, P, alpha, eps)
        shifts = new
    return x, shifts
