"""The fp64 numpy restatement of the robust, regularised reconstruction (include/hrnet_hip.h: hrn_robust_sums / _finish / _apply,
hrn_btv_step / _backward / _value), on top of tests/observe_ref.py: the Welsch-weighted data step, the bilateral-TV
prior R with its gradient g, the half-step, the step-size rule and the driver loop of `hrnet_hip.observation.reconstruct` - and for every
output T, the sum of the absolute values of its terms, for the project's bound |got - want| <= C T.

Through a non-linear function the bound takes the function's Lipschitz constant times the argument's T plus the value's own magnitude:
exp(-u^2) has |d/du| <= sqrt(2 / e) = 0.858, phi' has 1 / eps and |phi'| <= 1, phi has 1.  The device and this file share the fp32 inputs,
the fp32-rounded weights alpha^k and every decision (`counted`, the 2^-60 threshold on sum w is far from any value the cases reach)."""
import numpy as np

import observe_ref as O

MIN_WEIGHT = 2.0 ** -60
EXP_LIPSCHITZ = float(np.sqrt(2.0 / np.e))
DATA_EIGENVALUE = 1.02


# ----------------------------------------------------------------------------- bilateral TV
def displacements(P):
    return [(l, m) for l in range(-P, P + 1) for m in range(-P, P + 1) if (l, m) != (0, 0)]


def btv_weights(P, alpha):
    """{k: alpha^k formed in fp64 from the fp32 alpha and rounded to fp32 once}, k = 0 .. 2 P"""
    a = np.float64(np.float32(alpha))
    return {k: np.float64(np.float32(a ** k)) for k in range(2 * P + 1)}


def weight_sum(P, alpha):
    """W = sum_{(l,m) != 0} alpha^(|l|+|m|), unrounded"""
    return sum(float(alpha) ** (abs(l) + abs(m)) for l, m in displacements(P))


def step_bound(step, lam, P, alpha, eps):
    return step * (DATA_EIGENVALUE + 4.0 * lam * weight_sum(P, alpha) / eps)


def _pairs(x, l, m):
    """the views (x_p, x_{p-(l,m)}) over the pixels p whose partner lies inside the frame, and the slices of p and of the partner"""
    H, W = x.shape[-2:]
    ys, yq = (slice(l, H), slice(0, H - l)) if l >= 0 else (slice(0, H + l), slice(-l, H))
    xs, xq = (slice(m, W), slice(0, W - m)) if m >= 0 else (slice(0, W + m), slice(-m, W))
    if abs(l) >= H or abs(m) >= W:
        return None
    return (Ellipsis, ys, xs), (Ellipsis, yq, xq)


def btv_value(x, P, alpha, eps):
    """x (..., H, W) -> (R, T_R) (...,): R as the definition writes it (every unordered pair twice); T = sum w (|x_p| + |x_q| + phi)"""
    x = np.asarray(x, np.float64)
    eps = np.float64(np.float32(eps))
    w = btv_weights(P, alpha)
    R, T = np.zeros(x.shape[:-2]), np.zeros(x.shape[:-2])
    for l, m in displacements(P):
        pr = _pairs(x, l, m)
        if pr is None:
            continue
        t = x[pr[0]] - x[pr[1]]
        phi = np.sqrt(t * t + eps * eps) - eps
        wk = w[abs(l) + abs(m)]
        R += wk * phi.sum((-2, -1))
        T += wk * (np.abs(x[pr[0]]) + np.abs(x[pr[1]]) + phi).sum((-2, -1))
    return R, T


def btv_grad(x, P, alpha, eps):
    """x (..., H, W) -> (g, T): for each d, g_p += w_d phi'(x_p - x_{p-d}) and g_{p-d} -= w_d phi'(.), as the definition writes it;
    T_p = sum over the in-frame neighbours q of p of w (1 + (|x_p| + |x_q|) / eps)"""
    x = np.asarray(x, np.float64)
    eps = np.float64(np.float32(eps))
    w = btv_weights(P, alpha)
    g, T = np.zeros_like(x), np.zeros_like(x)
    for l, m in displacements(P):
        pr = _pairs(x, l, m)
        if pr is None:
            continue
        t = x[pr[0]] - x[pr[1]]
        d = t / np.sqrt(t * t + eps * eps)
        wk = w[abs(l) + abs(m)]
        g[pr[0]] += wk * d
        g[pr[1]] -= wk * d
        T[pr[0]] += wk * (1.0 + (np.abs(x[pr[0]]) + np.abs(x[pr[1]])) / eps)
    return g, T


def btv_step(x, c, P, alpha, eps):
    """-> (x - c g, T = |x| + |c| T_g); c broadcasts over the planes"""
    x = np.asarray(x, np.float64)
    g, T = btv_grad(x, P, alpha, eps)
    c = np.asarray(c, np.float64).reshape((-1,) + (1, 1)) if np.ndim(c) else np.float64(c)
    return x - c * g, np.abs(x) + np.abs(c) * T


# ----------------------------------------------------------------------------- the robust data term
def robust_terms(s, beta_prev, T_beta_prev, delta, brightness=True):
    """s: observe_ref.loss of the frame; beta_prev, T_beta_prev (B,V) -> dict: w, T_w (B,V,H,W); sw, swe, sq (B,V); beta, T_beta,
    inlier, T_inlier (B,V); r, T_r = w (e + beta) (B,V,H,W); loss, T_loss (B,) = sum_v sq / sum_v sw"""
    delta = np.float64(np.float32(delta))
    cm, e, T_e = s["counted"], s["e"], s["T_e"]
    bp, T_bp = np.asarray(beta_prev, np.float64)[:, :, None, None], np.asarray(T_beta_prev, np.float64)[:, :, None, None]
    u = (e + bp) / delta
    w = np.where(cm, np.exp(-u * u), 0.0)
    T_w = np.where(cm, EXP_LIPSCHITZ * (T_e + T_bp) / delta + w, 0.0)
    sw, swe, sq = w.sum((2, 3)), (w * e).sum((2, 3)), (w * (e + bp) ** 2).sum((2, 3))
    T_sw, T_swe = T_w.sum((2, 3)), (T_w * np.abs(e) + w * T_e).sum((2, 3))
    live = (sw >= MIN_WEIGHT) & bool(brightness)
    safe = np.where(sw >= MIN_WEIGHT, sw, 1.0)
    beta = np.where(live, -swe / safe, 0.0)
    T_beta = np.where(live, (T_swe + np.abs(beta) * T_sw) / safe, 0.0)
    n = s["n"].astype(np.float64)
    inlier = np.where(n > 0, sw / np.where(n > 0, n, 1.0), 0.0)
    T_inlier = np.where(n > 0, T_sw / np.where(n > 0, n, 1.0), 0.0)
    r = w * (e + beta[:, :, None, None])
    T_r = T_w * np.abs(e + beta[:, :, None, None]) + w * (T_e + T_beta[:, :, None, None])
    tw, tq = sw.sum(1), sq.sum(1)
    T_sq = (T_w * (e + bp) ** 2 + 2.0 * w * np.abs(e + bp) * (T_e + T_bp)).sum((1, 2, 3))
    ok = tw >= MIN_WEIGHT
    st = np.where(ok, tw, 1.0)
    loss = np.where(ok, tq / st, 0.0)
    T_loss = np.where(ok, (T_sq + loss * T_sw.sum(1)) / st, 0.0)
    return dict(w=w, T_w=T_w, sw=sw, swe=swe, sq=sq, beta=beta, T_beta=T_beta, inlier=inlier, T_inlier=T_inlier, r=r, T_r=T_r, loss=loss,
                T_loss=T_loss)


def data_step(x, lrs, masks, alphas, shifts, scale, step=1.0, brightness=True, robust=False, delta=0.1, state=None):
    """one data step -> (x', T, info): info holds s (observe_ref.loss of x), the robust terms `rt` (or None) and the next state
    (beta_prev, T_beta_prev).  state None: the plain mean bias of this frame (zeros without brightness)."""
    x = np.asarray(x, np.float64)
    s = O.loss(x, lrs, masks, alphas, shifts, scale, brightness)
    vb = s["vb"].astype(np.float64)
    cf = np.where(vb > 0, np.float64(np.float32(step)) * scale * scale / np.where(vb > 0, vb, 1.0), 0.0)[:, None, None]
    if not robust:
        return x - cf * s["G"], np.abs(x) + cf * s["T_G"], dict(s=s, rt=None, state=None)
    bp, T_bp = (s["beta"], s["T_beta"]) if state is None else state
    rt = robust_terms(s, bp, T_bp, delta, brightness)
    G, T_G = O.adjoint(rt["r"], shifts, scale, rt["T_r"])
    return x - cf * G, np.abs(x) + cf * T_G, dict(s=s, rt=rt, state=(rt["beta"], rt["T_beta"]))


def reconstruct(x, lrs, masks, alphas, shifts, scale, iters, step=1.0, brightness=True, robust=True, delta=0.1, lam=4e-4, P=2, alpha=0.7,
                eps=0.02):
    """the driver loop -> (x, trace (iters, B, 3), T): trace = (plain loss, weighted loss, lam R / pixels) of the frame each iteration
    started from; T = the sum over the iterations of the steps' own T (the data operator does not expand an error - its eigenvalues lie
    in [0, 1.02] - and neither does the half-step under the step-size rule, so the steps' errors add)."""
    x = np.asarray(x, np.float64)
    B = x.shape[0]
    trace = np.zeros((iters, B, 3))
    T = np.zeros_like(x)
    state = None
    c = np.float64(np.float32(np.float64(step) * np.float64(lam)))
    for t in range(iters):
        if lam > 0:
            trace[t, :, 2] = np.float64(np.float32(lam)) * btv_value(x, P, alpha, eps)[0] / (x.shape[1] * x.shape[2])
        x, Tx, info = data_step(x, lrs, masks, alphas, shifts, scale, step, brightness, robust, delta, state)
        state = info["state"]
        trace[t, :, 0] = info["s"]["L"]
        trace[t, :, 1] = info["rt"]["loss"] if robust else info["s"]["L"]
        T += Tx
        if lam > 0:
            x, Tb = btv_step(x, c, P, alpha, eps)
            T += Tb
    return x, trace, T
