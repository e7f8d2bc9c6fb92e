"""GPU (-m gpu): the observation model's kernels (csrc/observe.hip: hrn_observe, hrn_consistency_residual, hrn_consistency_finish,
hrn_observe_adjoint) against the fp64 restatement (tests/observe_ref.py) under the project's bound |got - want| <= C T, C = 1e-5
(tests/kernel_bounds.py), T the restatement's sum of absolute terms: the 126 cases of tests/observe_cases.py - six shapes around the
kernels' tile, every scale, whole, half, almost-whole, random, far and NaN shifts, four kinds of masks, three of alphas, brightness on and
off.  No pixel is left out: the only decisions are the floor of an fp32 value and mask tests, which both sides take identically.  Checked
per case: views with valid exact; L_b and beta_v with n_v and V_b exact; the residual; d_srs; observe's backward; one back-projection
step, also in place.  Further: exact zeros where nothing counts, sentinels behind every output, reproducibility, independence of the
batch and of appended alpha-0 views, iters = 0, the losses of ten iterations, the adjoint identity, the dispatcher ops with their autograd
formulas, and frames past 2^31 elements."""
import numpy as np
import pytest
import torch

import kernel_bounds as KB
import kt
import observe_cases as OC
import observe_ref as O
import util
from hrnet_hip import binding

pytestmark = pytest.mark.gpu

PLAN = OC.plan()
_dev = lambda a: None if a is None else util.dev(a)
I32, F64 = torch.int32, torch.float64


def test_the_cases_use_the_kernels_tile():
    assert binding.OBSERVE_TILE == (OC.TH, OC.TW)


def _rc(rc, *guarded):
    torch.cuda.synchronize()
    assert rc == 0, binding.load_library().hrn_last_error()
    assert all(g.guard_ok() for g in guarded), "a write outside an output"


def _observe(hr, shifts, scale):
    """hrn_observe into sentinel-guarded outputs -> (views, valid), both Guarded"""
    B, SH, SW = hr.shape
    V, H, W = shifts.shape[1], SH // scale, SW // scale
    views, valid = KB.Guarded((B, V, H, W)), KB.Guarded((B, V, H, W))
    h, s = _dev(hr), _dev(shifts)
    _rc(kt.lib().hrn_observe(kt._p(h), kt._p(s), views.ptr, valid.ptr, B, V, H, W, scale, kt._stream()), views, valid)
    return views, valid


def _residual(x, hr, scale, brightness, step=1.0):
    """hrn_consistency_residual + hrn_consistency_finish -> dict of Guarded: residual, beta, count, ssr, loss, n_views, coef_loss, coef_step"""
    B, V, H, W = x["lrs"].shape
    lib = kt.lib()
    nbytes = lib.hrn_observe_workspace_bytes(B, V, H, W)
    assert nbytes == 24 * B * V * -(-H // OC.TH) * -(-W // OC.TW)
    ws = KB.Guarded((nbytes // 8,), F64)
    g = dict(residual=KB.Guarded((B, V, H, W)), beta=KB.Guarded((B, V)), count=KB.Guarded((B, V), I32), ssr=KB.Guarded((B, V), F64),
             loss=KB.Guarded((B,)), n_views=KB.Guarded((B,), I32), coef_loss=KB.Guarded((B,)), coef_step=KB.Guarded((B,)))
    h, lrs, masks, alphas, shifts = _dev(hr), _dev(x["lrs"]), _dev(x["masks"]), _dev(x["alphas"]), _dev(x["shifts"])
    _rc(lib.hrn_consistency_residual(kt._p(h), kt._p(lrs), kt._p(masks), kt._p(alphas), kt._p(shifts), g["residual"].ptr, ws.ptr, nbytes, B, V, H, W,
                                     scale, kt._stream()), ws, g["residual"])
    _rc(lib.hrn_consistency_finish(ws.ptr, nbytes, g["beta"].ptr, g["count"].ptr, g["ssr"].ptr, g["loss"].ptr, g["n_views"].ptr, g["coef_loss"].ptr,
                                   g["coef_step"].ptr, B, V, H, W, scale, step, int(brightness), kt._stream()), ws, *g.values())
    return g


def _adjoint(residual, x, scale, beta=None, coef=None, gain=None, frame=None, inplace=False, masked=True):
    """hrn_observe_adjoint -> out (Guarded).  residual, beta, coef, gain: CPU tensors / arrays or None; frame: x of the epilogue (CPU)"""
    B, V, H, W = residual.shape
    t = lambda a: None if a is None else (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).float().cuda().contiguous()
    r, bt, cf, gn, fr = t(residual), t(beta), t(coef), t(gain), t(frame)
    masks, alphas = (_dev(x["masks"]), _dev(x["alphas"])) if masked else (None, None)
    shifts = _dev(x["shifts"])
    out = KB.Guarded((B, scale * H, scale * W), v=torch.as_tensor(frame) if inplace else None)
    xp = out.ptr if inplace else kt._p(fr)
    _rc(kt.lib().hrn_observe_adjoint(kt._p(r), kt._p(masks), kt._p(alphas), kt._p(shifts), kt._p(bt), kt._p(cf), kt._p(gn), xp, out.ptr, B, V, H, W,
                                     scale, kt._stream()), out)
    return out


def _close(tag, got, want, T, layout="b y x"):
    got, want, T = got.double(), torch.from_numpy(np.asarray(want, np.float64)), torch.from_numpy(np.asarray(T, np.float64))
    assert bool(torch.isfinite(got).all()), f"{tag}: a non-finite value"
    return KB._assert_close(tag, "f32", got, want, T, layout=layout)


@pytest.mark.parametrize("c", PLAN, ids=OC.case_id)
def test_every_output_against_the_restatement(c):
    shape, scale, kind, mkind, akind, brightness = c
    B, V, H, W = shape
    x, ref = OC.inputs(c), OC.reference(c)
    tag = OC.case_id(c)
    # hrn_observe
    views, valid = _observe(x["hr"], x["shifts"], scale)
    assert torch.equal(valid.get() != 0, torch.from_numpy(ref["valid"])) and bool(((valid.get() == 0) | (valid.get() == 1)).all())
    _close(f"views {tag}", views.get(), ref["views"], ref["T_views"], "b v y x")
    assert bool((views.get()[torch.from_numpy(~ref["valid"])] == 0).all())
    # the residual and the finish launch
    g = _residual(x, x["hr"], scale, brightness)
    counted = torch.from_numpy(ref["counted"])
    assert torch.equal(g["count"].get().long(), torch.from_numpy(ref["n"])) and torch.equal(g["n_views"].get().long(), torch.from_numpy(ref["vb"]))
    _close(f"residual {tag}", g["residual"].get(), ref["e"], ref["T_e"], "b v y x")
    assert bool((g["residual"].get()[~counted] == 0).all())
    _close(f"beta {tag}", g["beta"].get(), ref["beta"], ref["T_beta"], "b v")
    _close(f"loss {tag}", g["loss"].get(), ref["L"], ref["T_L"], "b")
    _close(f"ssr {tag}", g["ssr"].get(), (ref["r"] ** 2).sum((2, 3)), (ref["T_r"] ** 2).sum((2, 3)), "b v")
    tot = ref["n"].sum(1).astype(np.float64)
    nothing = torch.from_numpy(tot == 0)
    assert bool((g["loss"].get()[nothing] == 0).all()) and bool((g["coef_loss"].get()[nothing] == 0).all())
    assert bool((g["coef_step"].get()[torch.from_numpy(ref["vb"] == 0)] == 0).all())
    assert bool((g["beta"].get()[torch.from_numpy(ref["n"] == 0)] == 0).all()) and (brightness or not g["beta"].get().any())
    some = tot > 0
    assert np.allclose(g["coef_loss"].get().numpy()[some], 2.0 / tot[some], rtol=1e-6, atol=0)
    assert np.allclose(g["coef_step"].get().numpy()[ref["vb"] > 0], scale * scale / ref["vb"][ref["vb"] > 0], rtol=1e-6, atol=0)
    # the loss' gradient, from the device's own residual, beta and coefficient
    d_srs = _adjoint(g["residual"].get(), x, scale, g["beta"].get(), g["coef_loss"].get(), x["gl"])
    _close(f"d_srs {tag}", d_srs.get(), ref["d_srs"], ref["T_d_srs"])
    assert bool((d_srs.get()[nothing] == 0).all()) and bool((d_srs.get()[torch.from_numpy(ref["T_d_srs"] == 0)] == 0).all())
    # observe's backward: the incoming gradient as the residual, nothing else
    d_hr = _adjoint(x["g"], x, scale, masked=False)
    _close(f"d_hr {tag}", d_hr.get(), ref["d_hr"], ref["T_d_hr"])
    # one back-projection step, apart and in place: the same bits
    x1 = _adjoint(g["residual"].get(), x, scale, g["beta"].get(), g["coef_step"].get(), None, frame=x["hr"])
    _close(f"x1 {tag}", x1.get(), ref["x1"], ref["T_x1"])
    same = torch.from_numpy(ref["vb"] == 0)
    assert torch.equal(x1.get()[same], torch.from_numpy(x["hr"])[same])
    x1i = _adjoint(g["residual"].get(), x, scale, g["beta"].get(), g["coef_step"].get(), None, frame=x["hr"], inplace=True)
    assert torch.equal(x1i.bits(), x1.bits())


@pytest.mark.parametrize("c", PLAN[3::5], ids=OC.case_id)
def test_adjoint_identity_of_the_device_results(c):
    """<A x, [valid] g> = <x, A^T [valid] g>, the device's results summed in fp64"""
    shape, scale, kind, mkind, akind, brightness = c
    x, ref = OC.inputs(c), OC.reference(c)
    views, valid = _observe(x["hr"], x["shifts"], scale)
    d_hr = _adjoint(x["g"], x, scale, masked=False)
    g, hr = x["g"].astype(np.float64), x["hr"].astype(np.float64)
    lhs, rhs = float((views.get().double().numpy() * g).sum()), float((hr * d_hr.get().double().numpy()).sum())
    bound = KB.C * (float((ref["T_views"] * np.abs(g)).sum()) + float((np.abs(hr) * ref["T_d_hr"]).sum()))
    print(f"{OC.case_id(c)}: <A x, g> - <x, A^T g> = {lhs - rhs:.3e}, bound {bound:.3e}")
    assert abs(lhs - rhs) <= bound


BATCHED = [c for c in PLAN if c[0][0] == 2 and c[0] not in OC.DEGENERATE and c[2] in ("random", "nan", "whole-eps")]


def _all_bits(x, scale, brightness):
    g = _residual(x, x["hr"], scale, brightness)
    d = _adjoint(g["residual"].get(), x, scale, g["beta"].get(), g["coef_loss"].get(), x["gl"])
    x1 = _adjoint(g["residual"].get(), x, scale, g["beta"].get(), g["coef_step"].get(), None, frame=x["hr"])
    views, valid = _observe(x["hr"], x["shifts"], scale)
    out = {k: v.get() for k, v in g.items()}
    out.update(d_srs=d.get(), x1=x1.get(), views=views.get(), valid=valid.get())
    return out


@pytest.mark.parametrize("c", BATCHED[::2], ids=OC.case_id)
def test_runs_are_bit_equal_and_a_sample_does_not_depend_on_its_batch_or_on_appended_views(c):
    shape, scale, kind, mkind, akind, brightness = c
    B, V, H, W = shape
    x = OC.inputs(c)
    a, again = _all_bits(x, scale, brightness), _all_bits(x, scale, brightness)
    bits = lambda p, q: torch.equal(p.contiguous().reshape(-1).view(torch.uint8), q.contiguous().reshape(-1).view(torch.uint8))
    assert all(bits(a[k], again[k]) for k in a)
    for b in range(B):
        one = {k: (None if v is None else v[b:b + 1]) for k, v in x.items()}
        o = _all_bits(one, scale, brightness)
        assert all(bits(o[k][0], a[k][b]) for k in a), b
    # three more views with alpha 0 (random data, clear masks, shifts of every kind, one NaN): no bit of a sample's results moves
    rng = np.random.Generator(np.random.PCG64(77))
    more = dict(x)
    more["lrs"] = np.concatenate([x["lrs"], rng.uniform(0, 1, (B, 3, H, W)).astype(np.float32)], 1)
    more["masks"] = None if x["masks"] is None else np.concatenate([x["masks"], np.ones((B, 3, H, W), np.float32)], 1)
    more["alphas"] = np.concatenate([np.ones((B, V), np.float32) if x["alphas"] is None else x["alphas"], np.zeros((B, 3), np.float32)], 1)
    extra = rng.uniform(-2, 2, (B, 3, 2)).astype(np.float32)
    extra[:, 1, 0] = np.nan
    more["shifts"] = np.concatenate([x["shifts"], extra], 1)
    m = _all_bits(more, scale, brightness)
    for k in ("loss", "n_views", "coef_loss", "coef_step", "d_srs", "x1"):
        assert bits(m[k], a[k]), k
    for k in ("residual", "beta", "count", "ssr"):
        assert bits(m[k][:, :V], a[k]) and not m[k][:, V:].any(), k
    assert bits(m["views"][:, :V], a["views"])


@pytest.mark.parametrize("scale", OC.SCALES)
def test_ten_iterations_on_a_mid_size_case(scale):
    """the device's losses of ten iterations do not increase and are the restatement's within 1e-4 relative; iters = 0 returns sr0's bits"""
    from hrnet_hip import observation
    c = next(c for c in PLAN if c[0] == OC.SHAPES[4] and c[1] == scale and c[2] == "random")
    shape, _, kind, mkind, akind, brightness = c
    x = OC.inputs(c)
    lrs, masks, alphas, shifts, hr = (_dev(x[k]) for k in ("lrs", "masks", "alphas", "shifts", "hr"))
    sr, losses = observation.back_project(hr, lrs, shifts, masks, alphas, scale, iters=10, brightness=brightness, return_loss=True)
    want_x, want = O.back_project(x["hr"], x["lrs"], x["masks"], x["alphas"], x["shifts"], scale, 10, 1.0, brightness)
    got = losses.cpu().double().numpy()
    print(f"x{scale}: device losses of sample 0 {got[:, 0]}, restatement {want[:, 0]}")
    assert losses.is_cuda and tuple(losses.shape) == (10, shape[0])
    live = want[0] > 0
    assert live.any() and np.all(np.diff(got, axis=0) <= 0) and np.all(np.diff(want, axis=0) <= 0)
    assert np.all(np.abs(got - want)[:, live] <= 1e-4 * want[:, live])
    assert not got[:, ~live].any()
    assert float((sr.cpu().double() - torch.from_numpy(want_x)).abs().max()) <= 1e-4
    zero, none = observation.back_project(hr, lrs, shifts, masks, alphas, scale, iters=0, return_loss=True)
    assert torch.equal(zero.view(torch.int32), hr.view(torch.int32)) and zero.data_ptr() != hr.data_ptr() and tuple(none.shape) == (0, shape[0])
    four = observation.back_project(hr[:, None], lrs, shifts, masks, alphas, scale, iters=2, brightness=brightness)
    two = observation.back_project(hr, lrs, shifts, masks, alphas, scale, iters=2, brightness=brightness)
    assert tuple(four.shape) == (shape[0], 1) + tuple(hr.shape[1:]) and torch.equal(four[:, 0], two)


def test_ops_pass_opcheck_and_their_gradients_are_the_restatements():
    from hrnet_hip import observation
    ops = torch.ops.hrnet_hip
    checks = ("test_schema", "test_faketensor", "test_autograd_registration")
    c = next(c for c in PLAN if c[0] == OC.SHAPES[4] and c[1] == 3 and c[2] == "random")
    shape, scale, kind, mkind, akind, brightness = c
    x, ref = OC.inputs(c), OC.reference(c)
    hr, lrs, masks, alphas, shifts, g, gl = (_dev(x[k]) for k in ("hr", "lrs", "masks", "alphas", "shifts", "g", "gl"))
    torch.library.opcheck(ops.observe.default, (hr, shifts, scale), test_utils=checks)
    torch.library.opcheck(ops.observe.default, (hr.clone().requires_grad_(True), shifts, scale), test_utils=checks)
    torch.library.opcheck(ops.observe_backward.default, (g, shifts, scale), test_utils=checks)
    torch.library.opcheck(ops.consistency_loss_train.default, (hr, lrs, masks, alphas, shifts, scale, brightness), test_utils=checks)
    torch.library.opcheck(ops.consistency_loss_train.default, (hr.clone().requires_grad_(True), lrs, None, None, shifts, scale, True), test_utils=checks)
    loss, residual, beta, count, coef = ops.consistency_loss_train(hr, lrs, masks, alphas, shifts, scale, brightness)
    torch.library.opcheck(ops.consistency_loss_backward.default, (gl, residual, beta, coef, masks, alphas, shifts, scale), test_utils=checks)
    torch.library.opcheck(ops.back_project.default, (hr, lrs, masks, alphas, shifts, scale, 2, 1.0, brightness), test_utils=checks)
    torch.library.opcheck(ops.back_project.default, (hr, lrs, None, None, shifts, scale, 0, 0.5, False), test_utils=checks)
    # the ops are the C entry points
    dev = _residual(x, x["hr"], scale, brightness)
    assert torch.equal(loss.cpu(), dev["loss"].get()) and torch.equal(residual.cpu(), dev["residual"].get()) and torch.equal(beta.cpu(), dev["beta"].get())
    assert torch.equal(count.cpu(), dev["count"].get()) and torch.equal(coef.cpu(), dev["coef_loss"].get())
    # autograd through hrnet_hip.observation: d_srs and observe's backward are the restatement's
    xr = hr.clone().requires_grad_(True)
    L = observation.consistency_loss(xr, lrs, shifts, masks, alphas, scale, brightness)
    assert torch.equal(L, loss)
    (L * gl).sum().backward()
    _close("op d_srs", xr.grad.cpu(), ref["d_srs"], ref["T_d_srs"])
    assert lrs.grad is None and shifts.grad is None
    L4, res, bt, cnt = observation.consistency_loss(hr[:, None], lrs, shifts, masks, alphas, scale, brightness, return_residual=True)
    assert torch.equal(L4, loss) and torch.equal(res, residual) and torch.equal(bt, beta) and torch.equal(cnt, count) and not res.requires_grad
    xr2 = hr.clone().requires_grad_(True)
    views, valid = observation.observe(xr2, shifts, scale)
    assert not valid.requires_grad and torch.equal(valid.cpu() != 0, torch.from_numpy(ref["valid"]))
    _close("op views", views.detach().cpu(), ref["views"], ref["T_views"], "b v y x")
    views.backward(g)
    _close("op d_hr", xr2.grad.cpu(), ref["d_hr"], ref["T_d_hr"])
    # back_project is its three launches, and carries no gradient
    sr, losses = observation.back_project(xr, lrs, shifts, masks, alphas, scale, iters=1, brightness=brightness, return_loss=True)
    _close("op x1", sr.cpu(), ref["x1"], ref["T_x1"])
    assert not sr.requires_grad and torch.equal(losses[0], loss)


def test_frames_beyond_2_31_elements():
    """57 samples of one 2048 x 2048 view at x3: hr and d_hr hold 57 x 6144^2 = 2.15e9 elements (past 2^31) in 8.6e9 bytes (past 2^32),
    934k tiles walked by a grid of 2^16 workgroups.  hrn_observe reads the big frame, hrn_observe_adjoint writes one; 32 sampled rows -
    the first and last, the rows beside the tile seams, and random ones - of sample 0, the last sample and the samples every boundary
    falls into, against the restatement formed in fp64 on the device (its matrices are tests/observe_ref.py's)."""
    n, side, scale = 57, 2048, 3
    KB._need(22)
    pool = KB._Pool()
    try:
        SH = scale * side
        per = SH * SH
        assert n * per > 1 << 31 and 4 * n * per > 1 << 32
        hr = pool.big(n, (SH, SH), KB.F32, fill="rand", seed=13, scale=0.5)
        rng = np.random.Generator(np.random.PCG64(57))
        shifts_np = rng.uniform(-1.5, 1.5, (n, 1, 2)).astype(np.float32)
        shifts = pool.keep(util.dev(shifts_np))
        views = pool.keep(torch.full((n, 1, side, side), float("nan"), device="cuda"))
        valid = pool.keep(torch.full((n, 1, side, side), float("nan"), device="cuda"))
        before = hr.checksum()
        rc = kt.lib().hrn_observe(hr.ptr, kt._p(shifts), kt._p(views), kt._p(valid), n, 1, side, side, scale, kt._stream())
        torch.cuda.synchronize()
        assert rc == 0, binding.load_library().hrn_last_error()
        assert hr.guards_intact() and hr.checksum() == before
        planes = KB.boundary_images(n, per, 4)
        assert planes[0] == 0 and planes[-1] == n - 1 and len(planes) >= 4
        rows = sorted({0, 1, side - 2, side - 1, OC.TH - 1, OC.TH, side // 2 - 1, side // 2} | set(int(r) for r in rng.integers(0, side, 24)))
        mats = {}
        for k in planes:
            Ay = torch.from_numpy(O.axis_matrix(side, scale, shifts_np[k, 0, 0], rows=rows)).cuda()
            Ax = torch.from_numpy(O.axis_matrix(side, scale, shifts_np[k, 0, 1])).cuda()
            f = hr.raw[2 * k * per:2 * (k + 1) * per].view(torch.float32).view(SH, SH).double()
            want, T = Ay @ f @ Ax.T, Ay.abs() @ f.abs() @ Ax.abs().T
            got = views[k, 0][rows].double()
            ratio = float(((got - want).abs() / (KB.C * T + 1e-300)).max())
            print(f"views, sample {k}: max error / bound {ratio:.3e}; C needed {ratio * KB.C:.2e}")
            assert ratio <= 1.0 and float((T > 0).double().mean()) >= 0.75, k      # (four of the sampled rows are border rows: not valid)
            assert torch.equal(valid[k, 0][rows] != 0, T > 0)
            del f, want, T, got, Ay, Ax
        # the adjoint of the views themselves (finite everywhere, 0 where not valid), written into a second frame of that size
        d_hr = pool.big(n, (SH, SH), KB.F32, fill="sent")
        rc = kt.lib().hrn_observe_adjoint(kt._p(views), None, None, kt._p(shifts), None, None, None, None, d_hr.ptr, n, 1, side, side, scale, kt._stream())
        torch.cuda.synchronize()
        assert rc == 0, binding.load_library().hrn_last_error()
        assert d_hr.guards_intact()
        hrows = sorted({0, 1, SH - 2, SH - 1, scale * OC.TH - 1, scale * OC.TH, SH // 2 - 1, SH // 2} | set(int(r) for r in rng.integers(0, SH, 24)))
        for k in planes:
            Ay = torch.from_numpy(O.axis_matrix(side, scale, shifts_np[k, 0, 0])).cuda()
            Ax = torch.from_numpy(O.axis_matrix(side, scale, shifts_np[k, 0, 1])).cuda()
            r = views[k, 0].double()
            want, T = Ay.T[hrows] @ r @ Ax, Ay.T[hrows].abs() @ r.abs() @ Ax.abs()
            got = d_hr.raw[2 * k * per:2 * (k + 1) * per].view(torch.float32).view(SH, SH)[hrows].double()
            ratio = float(((got - want).abs() / (KB.C * T + 1e-300)).max())
            print(f"d_hr, sample {k}: max error / bound {ratio:.3e}; C needed {ratio * KB.C:.2e}")
            assert ratio <= 1.0, k
            assert bool((got[T == 0] == 0).all())
            del r, want, T, got, Ay, Ax
    finally:
        pool.free()
