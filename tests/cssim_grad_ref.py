"""The gradient of cSSIM with respect to sr (include/hrnet_hip.h) restated in fp64 numpy in the DIRECT form: X = m g,
Y = m (s + b), five filtered fields, alpha / beta / gamma as the header writes them, the adjoint as a zero-padded correlation, the bias
attached.  The kernel (csrc/cssim_bwd.hip) centres its fields per tile, factors S_c and works in tiles; this does none of it, so the two
share only the definition.  Also: the same score composed in torch fp64 for autograd, a float32 MODEL of the kernel's centred algebra
(a model, not a reference and not the kernel, as cssim_ref.shift_cssim_f32 is), wrong variants of the restatement as controls, and the
case list that tests/test_cssim_loss_host.py (CPU) and tests/test_gpu_cssim_loss.py (GPU) share."""
import numpy as np

import cssim_cases as C
import cssim_ref as R

OR, WIN, RUN = 16, 64, 4                              # csrc/cssim_bwd.hip: CB_OR, CB_WIN, CB_RUN (the GPU test asserts them)
OC = {w: WIN - 2 * (T - 1) for w, T in R.TAPS.items()}         # crop columns of a backward tile: 44 (gaussian), 52 (uniform)

CONTROLS = ("bias_detached", "adjoint_tap_dropped", "adjoint_valid", "cov_norm_left_out", "neighbouring_offset", "pass_ignored")


def adjoint_full(F, taps):
    """the adjoint of cssim_ref.filter_valid: (mh, mw) -> (mh + T - 1, mw + T - 1), out[q] = sum_o taps[o] F[q - o], F zero outside"""
    T = len(taps)
    P = np.pad(F, T - 1)
    h, w = F.shape[0] + T - 1, F.shape[1] + T - 1
    rows = sum(taps[o] * P[T - 1 - o:T - 1 - o + h] for o in range(T))
    return sum(taps[o] * rows[:, T - 1 - o:T - 1 - o + w] for o in range(T))


def crops(sr, hr, hr_map, k, border, clip, dtype=np.float64):
    """-> (s clamped, g, m, pass) on the crop at the offset k"""
    sr, hr = np.asarray(sr, dtype), np.asarray(hr, dtype)
    H, W = sr.shape
    h, w = H - 2 * border, W - 2 * border
    u, v = divmod(int(k), 2 * border + 1)
    raw = sr[border:border + h, border:border + w]
    s = np.where(np.isnan(raw), raw, np.clip(raw, 0, 1)).astype(dtype) if clip else raw
    with np.errstate(invalid="ignore"):
        ok = ((raw >= 0) & (raw <= 1)) if clip else np.ones((h, w), bool)
    return s, hr[u:u + h, v:v + w], (np.asarray(hr_map)[u:u + h, v:v + w] != 0).astype(dtype), ok


def grad(sr, hr, hr_map, k, border=3, window_name="gaussian", clip=False, correct_bias=True, data_range=1.0, control=None):
    """One sample: d score_k / d sr with k held fixed, (H, W) fp64; all zeros for k < 0.  control: one of CONTROLS, the gradient with
    that one thing wrong."""
    assert control is None or control in CONTROLS, control
    H, W = np.asarray(sr).shape
    out = np.zeros((H, W))
    if k < 0:
        return out
    nb = 2 * border + 1
    if control == "neighbouring_offset":
        u, v = divmod(int(k), nb)
        k = u * nb + (v + 1 if v + 1 < nb else v - 1)
    taps, cn = R.window(window_name)
    s, g, m, ok = crops(sr, hr, hr_map, k, border, clip)
    n = m.sum()
    b = (m * (g - s)).sum() / n if correct_bias else 0.0
    X, Y = m * g, m * (s + b)
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    a, c = R.filter_valid(X, taps), R.filter_valid(Y, taps)
    vx = cn * (R.filter_valid(X * X, taps) - a * a)
    vy = cn * (R.filter_valid(Y * Y, taps) - c * c)
    vxy = cn * (R.filter_valid(X * Y, taps) - a * c)
    A1, A2, B1, B2 = 2 * a * c + c1, 2 * vxy + c2, a * a + c * c + c1, vx + vy + c2
    S_c = 2 * a * A2 / (B1 * B2) - 2 * c * A1 * A2 / (B1 * B1 * B2)
    S_vy = -A1 * A2 / (B1 * B2 * B2)
    S_vxy = 2 * A1 / (B1 * B2)
    cnd = 1.0 if control == "cov_norm_left_out" else cn
    beta, gamma = 2 * cnd * S_vy, cnd * S_vxy
    alpha = S_c - beta * c - gamma * a
    if control == "adjoint_valid":
        T = len(taps)
        assert min(a.shape) >= T, "the control needs a map of at least T x T"
        adj = lambda F: np.pad(R.filter_valid(F, taps[::-1]), T - 1)
    elif control == "adjoint_tap_dropped":
        short = taps.copy()
        short[-1] = 0.0
        adj = lambda F: adjoint_full(F, short)
    else:
        adj = lambda F: adjoint_full(F, taps)
    D = (adj(alpha) + Y * adj(beta) + X * adj(gamma)) / a.size
    M = (m * D).sum() / n if correct_bias and control != "bias_detached" else 0.0
    passed = np.ones_like(m) if control == "pass_ignored" else ok.astype(np.float64)
    out[border:border + s.shape[0], border:border + s.shape[1]] = passed * m * (D - M)
    return out


def grad_autograd(sr, hr, hr_map, k, border=3, window_name="gaussian", clip=False, correct_bias=True, data_range=1.0):
    """The same gradient by torch fp64 autograd through the direct composition of the score at the offset k, the bias attached."""
    import torch
    taps, cn = R.window(window_name)
    T = len(taps)
    sr_t = torch.tensor(np.asarray(sr, np.float64), requires_grad=True)
    H, W = sr_t.shape
    h, w = H - 2 * border, W - 2 * border
    u, v = divmod(int(k), 2 * border + 1)
    g = torch.tensor(np.asarray(hr, np.float64))[u:u + h, v:v + w]
    m = torch.tensor((np.asarray(hr_map) != 0).astype(np.float64))[u:u + h, v:v + w]
    s = sr_t[border:border + h, border:border + w]
    if clip:
        s = torch.clamp(s, 0.0, 1.0)
    b = (m * (g - s)).sum() / m.sum() if correct_bias else 0.0
    X, Y = m * g, m * (s + b)

    def filt(a):
        rows = sum(float(taps[o]) * a[o:o + h - T + 1] for o in range(T))
        return sum(float(taps[o]) * rows[:, o:o + w - T + 1] for o in range(T))
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    mx, my = filt(X), filt(Y)
    vx, vy, vxy = cn * (filt(X * X) - mx * mx), cn * (filt(Y * Y) - my * my), cn * (filt(X * Y) - mx * my)
    score = (((2 * mx * my + c1) * (2 * vxy + c2)) / ((mx * mx + my * my + c1) * (vx + vy + c2))).mean()
    score.backward()
    return sr_t.grad.numpy()


def grad_f32(sr, hr, hr_map, k, bias, n, border=3, window_name="gaussian", clip=False, correct_bias=True, data_range=1.0, form="centred"):
    """A MODEL of csrc/cssim_bwd.hip's arithmetic in float32 numpy, NOT a reference: its tiles (16 x (64 - 2 (T - 1)) crop pixels from a
    window of 64 columns), its per-tile centre, its six filtered fields, its factored S_c, its fp32 alpha' / beta / gamma, its fp64 mean
    M.  It is not the kernel either: numpy fuses no multiply-add and sums in another order.  bias, n: the forward's fp64 bias* and n*.
    form="uncentred": alpha + beta Y + gamma X on the uncentred fields, S_c as the header writes it - what the kernel must not do."""
    f32 = np.float32
    H, W = np.asarray(sr).shape
    out = np.zeros((H, W), f32)
    if k < 0:
        return out
    taps64, cov_norm = R.window(window_name)
    taps, cn = taps64.astype(f32), f32(cov_norm)
    flip = taps[::-1].copy()
    delta = f32(taps64.sum() ** 2 - 1.0)
    T = len(taps)
    halo = T - 1
    s_all, g_all, m_all, ok = crops(sr, hr, hr_map, k, border, clip, f32)
    h, w = s_all.shape
    mh, mw = h - T + 1, w - T + 1
    c1, c2 = f32(f32(0.01) * f32(data_range)) ** 2, f32(f32(0.03) * f32(data_range)) ** 2
    oc = WIN - 2 * halo
    mr, mc = OR + halo, WIN - halo
    irp = -(-mr // RUN) * RUN + halo
    pad = lambda a: np.pad(a, ((halo, irp + OR), (halo, WIN + oc)))         # staged row r of a tile is crop row y0 - halo + r
    S, G, Mk = pad(s_all), pad(g_all), pad(m_all)
    D = np.zeros((h, w), f32)
    two = f32(2)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for y0 in range(0, h, OR):
            for x0 in range(0, w, oc):
                s, g, m = S[y0:y0 + irp, x0:x0 + WIN], G[y0:y0 + irp, x0:x0 + WIN], Mk[y0:y0 + irp, x0:x0 + WIN]
                cnt = m.sum(dtype=np.float64)
                cen = f32((m * g).sum(dtype=np.float64) / cnt) if cnt > 0 and form == "centred" else f32(0)
                cen = cen if np.isfinite(cen) else f32(0)
                x, t = m * (g - cen), s - f32(np.float64(cen) - bias)
                y = m * t
                ww = R._filter32(f32(1) - m, taps) - delta
                ax, axx = R._filter32(x, taps), R._filter32(x * x, taps)
                ay, ayy, axy = R._filter32(y, taps), R._filter32(y * y, taps), R._filter32(x * y, taps)
                cp, cw = cen * (f32(1) - ww), cen * ww
                e = cp * cw
                mux, muy = ax + cp, ay + cp
                vx = cn * (((axx - ax * ax) + (two * cw) * ax) + e)
                vy = cn * (((ayy - ay * ay) + (two * cw) * ay) + e)
                vxy = cn * (((axy - ax * ay) + cw * (ax + ay)) + e)
                a1, b1 = two * mux * muy + c1, mux * mux + (muy * muy + c1)
                a2, b2 = two * vxy + c2, (vx + vy) + c2
                i1, i2 = f32(1) / b1, f32(1) / b2
                r1, r2 = a1 * i1, a2 * i2
                if form == "centred":
                    sc = ((two * r2) * (ax - ay)) * ((mux * (mux + muy) + c1) * (i1 * i1))
                else:
                    sc = two * mux * a2 / (b1 * b2) - two * muy * a1 * a2 / (b1 * b1 * b2)
                beta = (f32(-2) * cn) * ((r1 * i2) * r2)
                gamma = (two * cn) * (r1 * i2)
                alpha = (sc - beta * (ay - cw)) - gamma * (ax - cw)
                gy = (y0 - halo + np.arange(alpha.shape[0]))[:, None]
                gx = (x0 - halo + np.arange(alpha.shape[1]))[None, :]
                inside = (gy >= 0) & (gy < mh) & (gx >= 0) & (gx < mw)
                fa, fb, fg = (R._filter32(np.where(inside, q, f32(0))[:mr, :mc], flip) for q in (alpha, beta, gamma))
                assert fa.shape == (OR, oc) and fa.dtype == np.float32
                d = (fa + y[halo:halo + OR, halo:halo + oc] * fb) + x[halo:halo + OR, halo:halo + oc] * fg
                rows, cols = min(OR, h - y0), min(oc, w - x0)
                D[y0:y0 + rows, x0:x0 + cols] = d[:rows, :cols]
    M = float((m_all.astype(np.float64) * D).sum() / n) if correct_bias else 0.0
    val = ((D.astype(np.float64) - M) / (mh * mw)).astype(f32)
    out[border:border + h, border:border + w] = np.where(ok & (m_all != 0), val, f32(0))
    return out


def rel_err(got, want):
    """max |got - want| over the sample's max |gradient|"""
    return float(np.abs(np.asarray(got, np.float64) - want).max() / np.abs(want).max())


# ----------------------------------------------------------------------------- the cases
# (id, family, input, border, window, options): input is a key of `case_input`; options the keyword arguments clip / correct_bias.
def crop_frame(window, border, rows, cols):
    """the frame whose crop is `rows` x `cols`"""
    return rows + 2 * border, cols + 2 * border


def _cases():
    cases = []
    for window, T in R.TAPS.items():
        cases.append((f"one-pixel-map-{window}", "shapes", ("holes", 2, 6 + T, 6 + T), 3, window, {}))
        for B, H, W in ((2, 24, 24), (1, 49, 71)):
            cases.append((f"holes-{H}x{W}-{window}", "holes", ("holes", B, H, W), 3, window, {}))
        H, W = crop_frame(window, 3, OR + 1, OC[window] + 1)
        cases.append((f"tile+1-{window}", "shapes", ("holes", 1, H, W), 3, window, {}))
        H, W = crop_frame(window, 3, 2 * OR + 1, 2 * OC[window] + 1)
        cases.append((f"two-tiles+1-{window}-holes", "shapes", ("holes", 1, H, W), 3, window, {}))
        cases.append((f"two-tiles+1-{window}-clear", "shapes", ("clear", 1, H, W, 0.9, 0.05, "edge"), 3, window, {}))
        cases.append((f"border0-{window}", "borders", ("holes", 2, 24, 30), 0, window, {}))
        cases.append((f"border8-{window}", "borders", ("holes", 1, 43, 81), 8, window, {}))
        cases.append((f"no-bias-{window}", "options", ("holes", 2, 24, 24), 3, window, {"correct_bias": False}))
        cases.append((f"clip-{window}", "options", ("rescaled", 2, 24, 40), 3, window, {"clip": True}))
        cases.append((f"clip-no-bias-{window}", "options", ("rescaled", 2, 24, 40), 3, window, {"clip": True, "correct_bias": False}))
    for c in C.PIN_CASES:                                 # level 0.9, 0.5, 0.05 at contrast 0.05 (clear, blob, edge); 0.9 at 0.005 clear
        if c[1] == "conditioning":
            cases.append((c[0], "conditioning", ("pin", c[0]), c[6], c[7], {}))
    return cases


SEEDS = {}                                            # id -> the seed that replaces 0 where the best offset led by less than PIN_GAP
CASES = _cases()
FAMILIES = ("shapes", "holes", "borders", "options", "conditioning")
_PIN = {c[0]: c for c in C.PIN_CASES}
_refs = {}


def case_input(case):
    cid, _, inp, *_ = case
    seed = SEEDS.get(cid, 0)
    if inp[0] == "pin":
        return C.pin_input(_PIN[inp[1]])
    if inp[0] == "clear":
        return C.clear_batch(inp[1], inp[2], inp[3], inp[4], inp[5], inp[6], seed)
    s, h, m = C.scene_batch(inp[1], inp[2], inp[3], seed)
    if inp[0] == "rescaled":                              # 1.3 srs - 0.1 of the scene stretched to [0, 1] (it spans about [0.1, 0.8], which
        lo, hi = s.min(), s.max()                         # 1.3 srs - 0.1 alone would leave unclamped): pixels clamped at both ends
        s = (np.float32(1.3) * ((s - lo) / (hi - lo)) - np.float32(0.1)).astype(np.float32)
    return s, h, m


def case_ref(case):
    """-> (forward reference (scores, k, bias, n) per sample, [gradient of the score (H, W) fp64 per sample]), computed once"""
    cid, _, inp, border, window, opt = case
    if cid not in _refs:
        x = case_input(case)
        kw = dict(clip=opt.get("clip", False), correct_bias=opt.get("correct_bias", True))
        fwd = C.ref(x, border, window, key=("loss", cid), **kw)
        _refs[cid] = (fwd, [grad(x[0][b], x[1][b], x[2][b], fwd[1][b], border, window, **kw) for b in range(len(x[0]))])
    return _refs[cid]
