"""GPU (-m gpu): the kernels of the robust, regularised reconstruction (csrc/robust_sr.hip: hrn_robust_sums, hrn_robust_finish,
hrn_robust_apply, hrn_btv_step, hrn_btv_backward, hrn_btv_value) against the fp64 restatement (tests/robust_ref.py) under the project's
bound |got - want| <= C T, C = 1e-5 (tests/kernel_bounds.py).

Data kernels: the 126 cases of tests/observe_cases.py (six shapes around the tile, every scale, every kind of shift, masks, alphas,
brightness on and off), delta alternating between 0.5 and 0.1; T goes through exp with its Lipschitz bound 0.858 times the argument's T.
Checked per case: beta, the inlier fraction (sum w / n_v: the weights' own check), the weighted loss, r', one full robust step; exact zeros
where nothing counts; sentinels behind every output; and on the batched cases two runs bit-equal, a sample alone equal to itself in its
batch, appended alpha-0 views changing no bit.
Bilateral TV: planes 1 x 1, 1 x 7, 5 x 3, 2 x 2 and sides at the 16 x 64 tile - 1, the tile, + 1 and + P (odd widths: rows alternate in
16-byte alignment), P = 1, 2, 3, three planes; the step, the backward and the value with T_p = sum_q w (1 + (|x_p| + |x_q|) / eps); exact
zeros among equal neighbours; out == x refused.
The driver against back_project's bits and against ten iterations of the restatement; the dispatcher ops; a frame past 2^31 elements."""
import ctypes

import numpy as np
import pytest
import torch

import kernel_bounds as KB
import kt
import observe_cases as OC
import observe_ref as O
import robust_ref as RB
import util
from hrnet_hip import binding

pytestmark = pytest.mark.gpu

PLAN = OC.plan()
_dev = lambda a: None if a is None else util.dev(a)
I32, F64 = torch.int32, torch.float64
ALPHA, EPS = 0.7, 0.02
needed = {}                                               # family -> the largest C any case needed (printed)


def _rc(rc, *guarded):
    torch.cuda.synchronize()
    assert rc == 0, binding.load_library().hrn_last_error()
    assert all(g.guard_ok() for g in guarded), "a write outside an output"


def _close(tag, got, want, T, layout="b y x"):
    got, want, T = got.double(), torch.from_numpy(np.asarray(want, np.float64)), torch.from_numpy(np.asarray(T, np.float64))
    assert bool(torch.isfinite(got).all()), f"{tag}: a non-finite value"
    c_used = float(((got - want).abs() / (T + 1e-300)).max()) if got.numel() else 0.0
    fam = tag.split()[0]
    needed[fam] = max(needed.get(fam, 0.0), c_used)
    return KB._assert_close(tag, "f32", got, want, T, layout=layout)


def _delta(c):
    return (0.5, 0.1)[PLAN.index(c) % 2]


def _robust(x, scale, brightness, delta):
    """residual + finish, then sums, finish, apply and the adjoint's step, all into guarded outputs -> dict of CPU tensors"""
    B, V, H, W = x["lrs"].shape
    lib = kt.lib()
    nbytes = lib.hrn_observe_workspace_bytes(B, V, H, W)
    assert nbytes == lib.hrn_robust_workspace_bytes(B, V, H, W)
    ws, rws = KB.Guarded((nbytes // 8,), F64), KB.Guarded((nbytes // 8,), F64)
    g = dict(residual=KB.Guarded((B, V, H, W)), beta0=KB.Guarded((B, V)), count=KB.Guarded((B, V), I32), ssr=KB.Guarded((B, V), F64),
             loss0=KB.Guarded((B,)), n_views=KB.Guarded((B,), I32), coef_loss=KB.Guarded((B,)), coef_step=KB.Guarded((B,)),
             beta=KB.Guarded((B, V)), inlier=KB.Guarded((B, V)), loss=KB.Guarded((B,)), weighted=KB.Guarded((B, V, H, W)),
             x1=KB.Guarded((B, scale * H, scale * W)))
    h, lrs, masks, alphas, shifts = _dev(x["hr"]), _dev(x["lrs"]), _dev(x["masks"]), _dev(x["alphas"]), _dev(x["shifts"])
    s = kt._stream()
    _rc(lib.hrn_consistency_residual(kt._p(h), kt._p(lrs), kt._p(masks), kt._p(alphas), kt._p(shifts), g["residual"].ptr, ws.ptr, nbytes, B, V, H, W,
                                     scale, s), ws, g["residual"])
    _rc(lib.hrn_consistency_finish(ws.ptr, nbytes, g["beta0"].ptr, g["count"].ptr, g["ssr"].ptr, g["loss0"].ptr, g["n_views"].ptr,
                                   g["coef_loss"].ptr, g["coef_step"].ptr, B, V, H, W, scale, 1.0, int(brightness), s), ws)
    _rc(lib.hrn_robust_sums(g["residual"].ptr, kt._p(masks), kt._p(alphas), kt._p(shifts), g["beta0"].ptr, rws.ptr, nbytes, B, V, H, W, scale,
                            delta, s), rws, g["residual"], g["beta0"])
    _rc(lib.hrn_robust_finish(rws.ptr, nbytes, g["count"].ptr, g["beta"].ptr, g["inlier"].ptr, g["loss"].ptr, B, V, H, W, int(brightness), s),
        rws, g["beta"], g["inlier"], g["loss"], g["count"])
    _rc(lib.hrn_robust_apply(g["residual"].ptr, kt._p(masks), kt._p(alphas), kt._p(shifts), g["beta0"].ptr, g["beta"].ptr, g["weighted"].ptr, B, V,
                             H, W, scale, delta, s), g["weighted"], g["residual"], g["beta"])
    _rc(lib.hrn_observe_adjoint(g["weighted"].ptr, kt._p(masks), kt._p(alphas), kt._p(shifts), None, g["coef_step"].ptr, None, kt._p(h),
                                g["x1"].ptr, B, V, H, W, scale, s), *g.values())
    return {k: v.get() for k, v in g.items()}


@pytest.mark.parametrize("c", PLAN, ids=OC.case_id)
def test_data_kernels_against_the_restatement(c):
    shape, scale, kind, mkind, akind, brightness = c
    x, ref, tag, delta = OC.inputs(c), OC.reference(c), OC.case_id(c), _delta(c)
    rt = RB.robust_terms(ref, ref["beta"], ref["T_beta"], delta, brightness)
    x1, T_x1, _ = RB.data_step(x["hr"], x["lrs"], x["masks"], x["alphas"], x["shifts"], scale, 1.0, brightness, robust=True, delta=delta)
    g = _robust(x, scale, brightness, delta)
    counted = torch.from_numpy(ref["counted"])
    _close(f"beta {tag}", g["beta"], rt["beta"], rt["T_beta"], "b v")
    _close(f"inlier {tag}", g["inlier"], rt["inlier"], rt["T_inlier"], "b v")
    _close(f"wloss {tag}", g["loss"], rt["loss"], rt["T_loss"], "b")
    _close(f"weighted {tag}", g["weighted"], rt["r"], rt["T_r"], "b v y x")
    _close(f"step {tag}", g["x1"], x1, T_x1)
    assert bool((g["weighted"][~counted] == 0).all())
    none = torch.from_numpy(ref["n"] == 0)
    assert bool((g["beta"][none] == 0).all()) and bool((g["inlier"][none] == 0).all()) and (brightness or not g["beta"].any())
    assert bool((g["loss"][torch.from_numpy(ref["n"].sum(1) == 0)] == 0).all())
    same = torch.from_numpy(ref["vb"] == 0)
    assert torch.equal(g["x1"][same], torch.from_numpy(x["hr"])[same])
    assert bool(((g["inlier"] >= 0) & (g["inlier"] <= 1)).all())


BATCHED = [c for c in PLAN if c[0][0] == 2 and c[0] not in OC.DEGENERATE and c[2] in ("random", "nan", "whole-eps")]
_bits = lambda p, q: torch.equal(p.contiguous().reshape(-1).view(torch.uint8), q.contiguous().reshape(-1).view(torch.uint8))


@pytest.mark.parametrize("c", BATCHED[::2], ids=OC.case_id)
def test_data_kernels_are_reproducible_and_independent_of_the_batch_and_of_appended_views(c):
    shape, scale, kind, mkind, akind, brightness = c
    B, V, H, W = shape
    x, delta = OC.inputs(c), _delta(c)
    a, again = _robust(x, scale, brightness, delta), _robust(x, scale, brightness, delta)
    assert all(_bits(a[k], again[k]) for k in a)
    for b in range(B):
        one = {k: (None if v is None else v[b:b + 1]) for k, v in x.items()}
        o = _robust(one, scale, brightness, delta)
        assert all(_bits(o[k][0], a[k][b]) for k in a), b
    rng = np.random.Generator(np.random.PCG64(78))
    more = dict(x)
    more["lrs"] = np.concatenate([x["lrs"], rng.uniform(0, 1, (B, 3, H, W)).astype(np.float32)], 1)
    more["masks"] = None if x["masks"] is None else np.concatenate([x["masks"], np.ones((B, 3, H, W), np.float32)], 1)
    more["alphas"] = np.concatenate([np.ones((B, V), np.float32) if x["alphas"] is None else x["alphas"], np.zeros((B, 3), np.float32)], 1)
    extra = rng.uniform(-2, 2, (B, 3, 2)).astype(np.float32)
    extra[:, 1, 0] = np.nan
    more["shifts"] = np.concatenate([x["shifts"], extra], 1)
    m = _robust(more, scale, brightness, delta)
    for k in ("loss", "x1"):
        assert _bits(m[k], a[k]), k
    for k in ("beta", "inlier", "weighted"):
        assert _bits(m[k][:, :V], a[k]) and not m[k][:, V:].any(), k


# ----------------------------------------------------------------------------- bilateral TV
TH, TW = binding.BTV_TILE
SMALL = [(1, 1), (1, 7), (5, 3), (2, 2)]


def _btv_shapes(P):
    return SMALL + [(TH - 1, TW - 1), (TH, TW), (TH + 1, TW + 1), (TH + P, TW + P), (TH + 1, TW - 1), (2 * TH + 1, 2 * TW + 3)]


def _plane(shape, seed):
    """three planes in [0, 1] with a block of exactly equal values in each (where the frame has room for one)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    x = rng.uniform(0, 1, (3,) + shape).astype(np.float32)
    H, W = shape
    if H >= 12 and W >= 12:
        x[:, 2:12, W - 12:W - 2] = np.float32(0.625)
    return x


def _btv_run(fn, x, c, P):
    n, SH, SW = x.shape
    out = KB.Guarded(x.shape)
    xd, cd = _dev(x), _dev(c)
    _rc(getattr(kt.lib(), fn)(kt._p(xd), kt._p(cd), out.ptr, n, SH, SW, P, ALPHA, EPS, kt._stream()), out)
    return out.get()


def _btv_value(x, P, gain):
    n, SH, SW = x.shape
    lib = kt.lib()
    nbytes = lib.hrn_btv_workspace_bytes(n, SH, SW)
    assert nbytes == 8 * n * -(-SH // TH) * -(-SW // TW)
    ws, val = KB.Guarded((nbytes // 8,), F64), KB.Guarded((n,))
    xd = _dev(x)
    _rc(lib.hrn_btv_value(kt._p(xd), val.ptr, ws.ptr, nbytes, n, SH, SW, P, ALPHA, EPS, gain, kt._stream()), ws, val)
    return val.get()


@pytest.mark.parametrize("P", [1, 2, 3])
def test_btv_kernels_against_the_restatement(P):
    for k, shape in enumerate(_btv_shapes(P)):
        tag = f"P{P}-{shape[0]}x{shape[1]}"
        x = _plane(shape, 100 * P + k)
        c = np.array([0.004, 0.0004, 0.01], np.float32)
        g, T = RB.btv_grad(x, P, ALPHA, EPS)
        c64 = c.astype(np.float64)[:, None, None]
        step = _btv_run("hrn_btv_step", x, c, P)
        _close(f"btv_step {tag}", step, x.astype(np.float64) - c64 * g, np.abs(x) + c64 * T, "n y x")
        back = _btv_run("hrn_btv_backward", x, c, P)
        _close(f"btv_backward {tag}", back, c64 * g, c64 * T, "n y x")
        R, T_R = RB.btv_value(x, P, ALPHA, EPS)
        gain = 0.5
        _close(f"btv_value {tag}", _btv_value(x, P, gain), gain * R / (shape[0] * shape[1]), gain * T_R / (shape[0] * shape[1]), "n")
        # equal neighbours: exactly 0, and x unchanged there
        H, W = shape
        if H >= 12 and W >= 12:
            inner = (slice(None), slice(2 + P, 12 - P), slice(W - 12 + P, W - 2 - P))
            assert not g[inner].any() and not back[inner].any() and torch.equal(step[inner], torch.from_numpy(x)[inner])
        if shape == (1, 1):
            assert not back.any() and torch.equal(step, torch.from_numpy(x)) and not _btv_value(x, P, gain).any()
        # reproducible, and a plane alone is itself in the batch
        assert _bits(_btv_run("hrn_btv_step", x, c, P), step)
        for n in range(3):
            assert _bits(_btv_run("hrn_btv_step", x[n:n + 1], c[n:n + 1], P)[0], step[n]), n
            assert _bits(_btv_value(x[n:n + 1], P, gain)[0], _btv_value(x, P, gain)[n]), n


def test_btv_step_refuses_to_work_in_place():
    x = _dev(_plane((20, 70), 1))
    c = _dev(np.ones(3, np.float32))
    before = x.clone()
    lib = kt.lib()
    for fn in (lib.hrn_btv_step, lib.hrn_btv_backward):
        assert fn(kt._p(x), kt._p(c), kt._p(x), 3, 20, 70, 2, ALPHA, EPS, kt._stream()) == -2 and b"alias" in lib.hrn_last_error()
        assert fn(kt._p(x), kt._p(c), ctypes.c_void_p(x.data_ptr() + 4 * 20 * 70), 2, 20, 70, 2, ALPHA, EPS, kt._stream()) == -2
    torch.cuda.synchronize()
    assert torch.equal(x, before)


# ----------------------------------------------------------------------------- the driver
MID = [c for c in PLAN if c[0] == (2, 5, 17, 63) and c[2] == "random"]


@pytest.mark.parametrize("c", MID, ids=OC.case_id)
def test_driver_against_back_project_and_ten_iterations_of_the_restatement(c):
    from hrnet_hip import observation
    shape, scale, kind, mkind, akind, brightness = c
    x = OC.inputs(c)
    lrs, masks, alphas, shifts, hr = (_dev(x[k]) for k in ("lrs", "masks", "alphas", "shifts", "hr"))
    plain, trace = observation.reconstruct(hr, lrs, shifts, masks, alphas, scale, iters=4, brightness=brightness, robust=None, lam=0.0,
                                           return_trace=True)
    bp, losses = observation.back_project(hr, lrs, shifts, masks, alphas, scale, iters=4, brightness=brightness, return_loss=True)
    assert _bits(plain, bp) and _bits(trace[:, :, 0].contiguous(), losses) and _bits(trace[:, :, 1].contiguous(), losses) and not trace[:, :, 2].any()
    zero, none = observation.reconstruct(hr, lrs, shifts, masks, alphas, scale, iters=0, return_trace=True)
    assert _bits(zero, hr) and zero.data_ptr() != hr.data_ptr() and tuple(none.shape) == (0, shape[0], 3)
    four = observation.reconstruct(hr[:, None], lrs, shifts, masks, alphas, scale, iters=2, brightness=brightness)
    assert tuple(four.shape) == (shape[0], 1) + tuple(hr.shape[1:]) and not four.requires_grad
    for robust, lam in (("welsch", 4e-4), ("welsch", 0.0), (None, 4e-4)):
        delta = 0.5
        sr, trace = observation.reconstruct(hr, lrs, shifts, masks, alphas, scale, iters=10, brightness=brightness, robust=robust, delta=delta,
                                            lam=lam, return_trace=True)
        want, wtrace, T = RB.reconstruct(x["hr"], x["lrs"], x["masks"], x["alphas"], x["shifts"], scale, 10, 1.0, brightness, robust is not None,
                                         delta, lam, 2, ALPHA, EPS)
        tag = f"driver {OC.case_id(c)} {robust} lam={lam:g}"
        _close(tag, sr.cpu(), want, T)
        got = trace.cpu().double().numpy()
        assert trace.is_cuda and got.shape == wtrace.shape
        live = wtrace > 0
        rel = np.abs(got - wtrace)[live] / wtrace[live]
        print(f"{tag}: trace within {rel.max():.2e} relative; plain loss {got[0, 0, 0]:.4e} -> {got[-1, 0, 0]:.4e}")
        assert rel.max() <= 1e-4 and not got[~live].any()
        silent = observation.reconstruct(hr, lrs, shifts, masks, alphas, scale, iters=10, brightness=brightness, robust=robust, delta=delta, lam=lam)
        assert _bits(silent, sr)


def test_a_sample_in_which_nothing_counts_still_takes_the_prior_half_step():
    from hrnet_hip import observation
    c = MID[0]
    x = OC.inputs(c)
    lrs, shifts, hr = (_dev(x[k]) for k in ("lrs", "shifts", "hr"))
    alphas = torch.ones(lrs.shape[:2], device="cuda")
    alphas[1] = 0
    sr = observation.reconstruct(hr, lrs, shifts, None, alphas, c[1], iters=1, lam=4e-4)
    want, T = RB.btv_step(x["hr"][1:], np.float32(4e-4), 2, ALPHA, EPS)
    _close("driver nothing-counts", sr[1:].cpu(), want, T)
    assert not torch.equal(sr[1], hr[1])


def test_ops_pass_opcheck_and_btv_loss_has_the_restatements_gradient():
    from hrnet_hip import observation
    ops = torch.ops.hrnet_hip
    checks = ("test_schema", "test_faketensor", "test_autograd_registration")
    c = MID[0]
    shape, scale, kind, mkind, akind, brightness = c
    x = OC.inputs(c)
    hr, lrs, masks, alphas, shifts = (_dev(x[k]) for k in ("hr", "lrs", "masks", "alphas", "shifts"))
    torch.library.opcheck(ops.reconstruct.default, (hr, lrs, masks, alphas, shifts, scale, 2, 1.0, brightness, True, 0.1, 4e-4, 2, 0.7, 0.02, True),
                          test_utils=checks)
    torch.library.opcheck(ops.reconstruct.default, (hr, lrs, None, None, shifts, scale, 0, 0.5, False, False, 0.1, 0.0, 1, 1.0, 0.1, False),
                          test_utils=checks)
    torch.library.opcheck(ops.btv_loss_train.default, (hr, 2, 0.7, 0.02), test_utils=checks)
    torch.library.opcheck(ops.btv_loss_train.default, (hr.clone().requires_grad_(True), 3, 0.5, 0.1), test_utils=checks)
    gl = _dev(x["gl"])
    torch.library.opcheck(ops.btv_loss_backward.default, (gl, hr, 2, 0.7, 0.02), test_utils=checks)
    for P in (1, 2, 3):
        xr = hr.clone().requires_grad_(True)
        L = observation.btv_loss(xr, P, ALPHA, EPS)
        R, T_R = RB.btv_value(x["hr"], P, ALPHA, EPS)
        pixels = hr.shape[1] * hr.shape[2]
        _close(f"btv_loss P{P}", L.detach().cpu(), R / pixels, T_R / pixels, "b")
        (L * gl).sum().backward()
        g, T = RB.btv_grad(x["hr"], P, ALPHA, EPS)
        w = x["gl"].astype(np.float64)[:, None, None] / pixels
        _close(f"btv_loss_grad P{P}", xr.grad.cpu(), w * g, w * T)
        L4 = observation.btv_loss(hr[:, None], P, ALPHA, EPS)
        assert torch.equal(L4, L.detach())


def _grad64(f, P):
    """the restatement's g and T of one fp64 plane on the device (tests/robust_ref.py's btv_grad, word by word)"""
    w = RB.btv_weights(P, ALPHA)
    eps = float(np.float32(EPS))
    g, T = torch.zeros_like(f), torch.zeros_like(f)
    for l, m in RB.displacements(P):
        pr = RB._pairs(f, l, m)
        t = f[pr[0][1:]] - f[pr[1][1:]]
        d = t / torch.sqrt(t * t + eps * eps)
        wk = float(w[abs(l) + abs(m)])
        g[pr[0][1:]] += wk * d
        g[pr[1][1:]] -= wk * d
        T[pr[0][1:]] += wk * (1.0 + (f[pr[0][1:]].abs() + f[pr[1][1:]].abs()) / eps)
    return g, T


def test_btv_step_beyond_2_31_elements():
    """57 planes of 6144 x 6144: 2.15e9 elements (past 2^31) in 8.6e9 bytes (past 2^32), 2.1 million tiles walked by a grid of 2^16
    workgroups.  32 sampled rows - the first and last, the rows beside the tile seams, and random ones - of plane 0, the last plane and the
    planes every boundary falls into, against the restatement formed in fp64 on the device."""
    n, side, P = 57, 6144, 2
    KB._need(24)
    pool = KB._Pool()
    try:
        per = side * side
        assert n * per > 1 << 31 and 4 * n * per > 1 << 32
        x = pool.big(n, (side, side), KB.F32, fill="rand", seed=17, scale=0.25)
        out = pool.big(n, (side, side), KB.F32, fill="sent")
        rng = np.random.Generator(np.random.PCG64(58))
        c_np = rng.uniform(0.001, 0.01, n).astype(np.float32)
        c = pool.keep(util.dev(c_np))
        before = x.checksum()
        rc = kt.lib().hrn_btv_step(x.ptr, kt._p(c), out.ptr, n, side, side, P, ALPHA, EPS, kt._stream())
        torch.cuda.synchronize()
        assert rc == 0, binding.load_library().hrn_last_error()
        assert x.guards_intact() and x.checksum() == before and out.guards_intact()
        planes = KB.boundary_images(n, per, 4)
        assert planes[0] == 0 and planes[-1] == n - 1 and len(planes) >= 4
        rows = sorted({0, 1, side - 2, side - 1, TH - 1, TH, side // 2 - 1, side // 2} | set(int(r) for r in rng.integers(0, side, 24)))
        for k in planes:
            f = x.raw[2 * k * per:2 * (k + 1) * per].view(torch.float32).view(side, side).double()
            g, T = _grad64(f, P)
            ck = float(c_np[k])
            want, bound = (f - ck * g)[rows], (f.abs() + ck * T)[rows]
            got = out.raw[2 * k * per:2 * (k + 1) * per].view(torch.float32).view(side, side)[rows].double()
            ratio = float(((got - want).abs() / (KB.C * bound + 1e-300)).max())
            print(f"btv_step, plane {k}: max error / bound {ratio:.3e}; C needed {ratio * KB.C:.2e}")
            assert ratio <= 1.0, k
            del f, g, T, want, bound, got
    finally:
        pool.free()


def test_print_the_constants_needed():
    """(runs last in this file) the largest C each family of outputs needed, for DESIGN.md section 7u"""
    for fam, c in sorted(needed.items()):
        print(f"C needed, {fam}: {c:.2e}")
    assert all(c <= KB.C for c in needed.values())
