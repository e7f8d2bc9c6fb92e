"""GPU (-m gpu): the observation model's derivative in the shifts (csrc/observe_shift.hip: hrn_observe_shift_grad / _grad_finish,
hrn_shift_normal / _normal_finish) against the fp64 restatement (tests/observe_shift_ref.py) under the project's bound
|got - want| <= C T + 2^-24 |want|, C = 1e-5 (tests/kernel_bounds.py), T the restatement's sums of absolute values built from the UNCENTRED
terms, the second term the one final rounding to fp32; no element is left out.  The cases are the 126 of tests/observe_cases.py (shapes up
to (1,33,8,32) and (2,5,17,63), every scale, partial tiles, the 33-view chunk boundary, far / NaN / whole / almost-whole shifts: the
smallest shapes that reach every branch).  Checked per case: d_shifts of `observe` at g and of the consistency loss from the device's own
residual, beta and coefficient; all eight entries of `normal` in plain and in Welsch mode (delta 0.5, beta_prev the plain mean bias), sum p
exact in plain mode; the residual plane and, tile by tile, the three plain sums (n, sum e, sum e^2: in plain mode the workspace's first
three entries, in both modes the optional plain workspace) bit-equal to hrn_consistency_residual's, sum p and beta to hrn_consistency_finish's;
the update against the fp64 formula applied to the DEVICE's own normal within 2 fp32 ulps of max(|d|, |step|); exact zeros and kept bits
for views that do not count, are fixed, far, NaN or alpha-0; sentinels behind every output.  Further: two runs bit-equal, a sample alone
equals itself in its batch, three appended alpha-0 views (one NaN shift) change no bit, either gradient half alone gives the bits of
both, the ops pass opcheck, shift_grad=False runs the old ops only, and refine_every=0 gives `reconstruct`'s bits."""
import functools

import numpy as np
import pytest
import torch

import kernel_bounds as KB
import kt
import observe_cases as OC
import observe_ref as O
import observe_shift_ref as R
import util
from hrnet_hip import binding

pytestmark = pytest.mark.gpu

PLAN = OC.plan()
DELTA = 0.5                   # the Welsch scale of these tests: the cases' residuals are of order 0.5, so the weights spread over (0, 1)
_dev = lambda a: None if a is None else util.dev(a)
I32, F64, U8 = torch.int32, torch.float64, torch.uint8
_bits = lambda p, q: torch.equal(p.contiguous().reshape(-1).view(U8), q.contiguous().reshape(-1).view(U8))


def _rc(rc, *guarded):
    torch.cuda.synchronize()
    assert rc == 0, binding.load_library().hrn_last_error()
    assert all(g.guard_ok() for g in guarded), "a write outside an output"


def _workspace(B, V, H, W):
    nbytes = kt.lib().hrn_observe_shift_workspace_bytes(B, V, H, W)
    assert nbytes == 8 * binding.SHIFT_NORMAL_SUMS * B * V * -(-H // OC.TH) * -(-W // OC.TW)
    return KB.Guarded((nbytes // 8,), F64), nbytes


def _t(a):
    return None if a is None else (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).float().cuda().contiguous()


def _grad(x, g, scale, masked=True, beta=None, coef=None, gain=None):
    """hrn_observe_shift_grad + _grad_finish -> d_shifts (Guarded)"""
    B, V, H, W = g.shape
    lib = kt.lib()
    ws, nbytes = _workspace(B, V, H, W)
    out = KB.Guarded((B, V, 2))
    hr, gd, shifts, bt, cf, gn = _dev(x["hr"]), _t(g), _dev(x["shifts"]), _t(beta), _t(coef), _t(gain)
    masks, alphas = (_dev(x["masks"]), _dev(x["alphas"])) if masked else (None, None)
    _rc(lib.hrn_observe_shift_grad(kt._p(hr), kt._p(gd), kt._p(masks), kt._p(alphas), kt._p(shifts), kt._p(bt), ws.ptr, nbytes, B, V, H, W, scale,
                                   kt._stream()), ws)
    _rc(lib.hrn_observe_shift_grad_finish(ws.ptr, nbytes, kt._p(cf), kt._p(gn), out.ptr, B, V, H, W, kt._stream()), ws, out)
    return out


def _normal(x, scale, brightness, beta_prev=None, fixed=None, damping=1e-3, max_step=0.5, update=True):
    """hrn_shift_normal + _normal_finish -> dict of Guarded: normal, residual, plain (the three plain sums a tile), sums (the workspace),
    shifts_out (None without `update`)"""
    B, V, H, W = x["lrs"].shape
    lib = kt.lib()
    ws, nbytes = _workspace(B, V, H, W)
    pbytes = lib.hrn_observe_workspace_bytes(B, V, H, W)
    g = dict(normal=KB.Guarded((B, V, 8), F64), residual=KB.Guarded((B, V, H, W)), plain=KB.Guarded((pbytes // 24, 3), F64), sums=ws,
             shifts_out=KB.Guarded((B, V, 2)) if update else None)
    hr, lrs, masks, alphas, shifts, bp = _dev(x["hr"]), _dev(x["lrs"]), _dev(x["masks"]), _dev(x["alphas"]), _dev(x["shifts"]), _t(beta_prev)
    fx = None if fixed is None else torch.from_numpy(np.ascontiguousarray(fixed, np.uint8)).cuda()
    _rc(lib.hrn_shift_normal(kt._p(hr), kt._p(lrs), kt._p(masks), kt._p(alphas), kt._p(shifts), kt._p(bp), DELTA, g["residual"].ptr, g["plain"].ptr,
                             pbytes, ws.ptr, nbytes, B, V, H, W, scale, kt._stream()), ws, g["residual"], g["plain"])
    _rc(lib.hrn_shift_normal_finish(ws.ptr, nbytes, kt._p(alphas), kt._p(shifts), kt._p(fx), g["normal"].ptr,
                                    g["shifts_out"].ptr if update else None, B, V, H, W, scale, int(brightness), damping, max_step, kt._stream()),
        ws, *(v for v in g.values() if v is not None))
    return g


def _residual(x, scale, brightness):
    """hrn_consistency_residual + _finish, the existing pair -> dict of CPU tensors: residual, beta, count, coef_loss, partials (tiles,3)"""
    B, V, H, W = x["lrs"].shape
    state = binding.ConsistencyState(B, V, H, W, "cuda")
    loss = torch.empty((B,), device="cuda")
    binding.consistency_residual(_dev(x["hr"]), _dev(x["lrs"]), _dev(x["masks"]), _dev(x["alphas"]), _dev(x["shifts"]), scale, 1.0, brightness,
                                 state, loss)
    torch.cuda.synchronize()
    return dict(residual=state.residual.cpu(), beta=state.beta.cpu(), count=state.count.cpu(), coef_loss=state.coef_loss.cpu(),
                partials=state.workspace.cpu().reshape(-1, 3))


def _close(tag, got, want, T, layout):
    got, want, T = got.double(), torch.from_numpy(np.asarray(want, np.float64)), torch.from_numpy(np.asarray(T, np.float64))
    assert bool(torch.isfinite(got).all()), f"{tag}: a non-finite value"
    return KB._assert_close(tag, "f32", got, want, T + 2.0 ** -24 * want.abs() / KB.C, layout=layout)


@functools.lru_cache(maxsize=None)
def _reference(c):
    """the restatement's results of a case, computed once: d_obs, d_loss (times gl), normal plain / Welsch, each with its T, and the
    beta_prev of the Welsch mode (the restatement's plain mean bias as fp32)"""
    shape, scale, kind, mkind, akind, brightness = c
    x, ref = OC.inputs(c), OC.reference(c)
    out = {}
    out["d_obs"], out["T_d_obs"] = R.d_shifts_observe(x["hr"], x["g"], x["shifts"], scale)
    out["d_loss"], out["T_d_loss"] = R.d_shifts_loss(x["hr"], x["lrs"], x["masks"], x["alphas"], x["shifts"], scale, brightness, x["gl"], s=ref)
    out["n_plain"], out["T_n_plain"] = R.normal(x["hr"], x["lrs"], x["masks"], x["alphas"], x["shifts"], scale, brightness, s=ref)
    out["beta_prev"] = ref["beta"].astype(np.float32)
    out["n_welsch"], out["T_n_welsch"] = R.normal(x["hr"], x["lrs"], x["masks"], x["alphas"], x["shifts"], scale, brightness, out["beta_prev"],
                                                  DELTA, s=ref)
    return out


def _check_update(tag, nrm, shifts_out, x, scale, fixed, damping=1e-3, max_step=0.5):
    """shifts_out against the fp64 formula on the device's own normal: 2 fp32 ulps of max(|d|, |step|); kept views keep their bits"""
    shifts = x["shifts"]
    keep = R.view_kept(x["alphas"], shifts, scale, fixed)
    want, steps, moved = R.update(nrm.numpy(), shifts, keep, damping, max_step)
    got = shifts_out.numpy()
    still = ~moved
    assert np.array_equal(got[still].view(np.uint32), shifts[still].view(np.uint32)), f"{tag}: a kept view's bits moved"
    if moved.any():
        scale_ = np.maximum(np.abs(shifts[moved].astype(np.float64)), np.abs(steps[moved]))
        err = np.abs(got[moved].astype(np.float64) - (shifts[moved].astype(np.float64) + steps[moved]))
        ulp = np.spacing(scale_.astype(np.float32)).astype(np.float64)
        print(f"{tag}: update of {int(moved.sum())} views, max error {float((err / ulp).max()):.2f} ulp")
        assert np.all(err <= 2.0 * ulp), tag
    return moved


@pytest.mark.parametrize("c", PLAN, ids=OC.case_id)
def test_every_output_against_the_restatement(c):
    shape, scale, kind, mkind, akind, brightness = c
    B, V, H, W = shape
    x, ref, want = OC.inputs(c), OC.reference(c), _reference(c)
    tag = OC.case_id(c)
    # observe's backward to the shifts: g where valid, nothing else
    d_obs = _grad(x, x["g"], scale, masked=False)
    _close(f"d_shifts observe {tag}", d_obs.get(), want["d_obs"], want["T_d_obs"], "b v a")
    assert bool((d_obs.get()[torch.from_numpy(want["T_d_obs"] == 0)] == 0).all())
    # the loss' gradient to the shifts, from the device's own residual, beta and coefficient
    dev = _residual(x, scale, brightness)
    d_loss = _grad(x, dev["residual"], scale, beta=dev["beta"], coef=dev["coef_loss"], gain=x["gl"])
    _close(f"d_shifts loss {tag}", d_loss.get(), want["d_loss"], want["T_d_loss"], "b v a")
    assert bool((d_loss.get()[torch.from_numpy(want["T_d_loss"] == 0)] == 0).all())
    dead = torch.from_numpy(R.view_kept(x["alphas"], x["shifts"], scale))          # does not count, or out of reach
    assert not d_loss.get()[dead].any(), "a view that does not count has a gradient"
    # the normal equations, plain: the residual plane and the plain sums are the existing kernels'
    fixed = R.fixed_mask(0, B, V)
    g = _normal(x, scale, brightness, fixed=fixed)
    n = g["normal"].get()
    assert _bits(g["residual"].get(), dev["residual"]), "the residual plane is not hrn_consistency_residual's"
    sums = g["sums"].get().reshape(-1, binding.SHIFT_NORMAL_SUMS)
    assert _bits(sums[:, :3].contiguous(), dev["partials"]), "a tile's n, sum e, sum e^2 are not hrn_consistency_residual's"
    assert _bits(g["plain"].get(), dev["partials"]), "the plain workspace is not hrn_consistency_residual's"
    assert torch.equal(n[..., 0], dev["count"].double()) and _bits(n[..., 6].float(), dev["beta"])
    _close(f"normal plain {tag}", n, want["n_plain"], want["T_n_plain"], "b v k")
    assert not n[dead].any()
    moved = _check_update(f"plain {tag}", n, g["shifts_out"].get(), x, scale, fixed)
    assert not moved[:, 0].any()
    # Welsch mode
    g = _normal(x, scale, brightness, beta_prev=want["beta_prev"], fixed=fixed, damping=0.1, max_step=0.05)
    n = g["normal"].get()
    assert _bits(g["residual"].get(), dev["residual"]) and _bits(g["plain"].get(), dev["partials"]), "Welsch mode: the plain sums moved"
    _close(f"normal welsch {tag}", n, want["n_welsch"], want["T_n_welsch"], "b v k")
    assert not n[dead].any()
    _check_update(f"welsch {tag}", n, g["shifts_out"].get(), x, scale, fixed, 0.1, 0.05)


def test_every_view_fixed_keeps_every_bit_and_shifts_out_is_optional():
    c = next(c for c in PLAN if c[0] == OC.SHAPES[4] and c[1] == 3 and c[2] == "nan")
    x = OC.inputs(c)
    B, V = c[0][:2]
    g = _normal(x, 3, True, fixed=np.ones((B, V), bool))
    assert np.array_equal(g["shifts_out"].get().numpy().view(np.uint32), x["shifts"].view(np.uint32))
    free = _normal(x, 3, True, fixed=None)
    assert not np.array_equal(free["shifts_out"].get().numpy().view(np.uint32), x["shifts"].view(np.uint32))
    only = _normal(x, 3, True, update=False)
    assert _bits(only["normal"].get(), g["normal"].get()) and _bits(free["normal"].get(), g["normal"].get())


BATCHED = [c for c in PLAN if c[0][0] == 2 and c[0] not in OC.DEGENERATE and c[2] in ("random", "nan", "whole-eps")]


def _all_bits(x, scale, brightness, bp):
    dev = _residual(x, scale, brightness)
    out = dict(d_obs=_grad(x, x["g"], scale, masked=False).get(),
               d_loss=_grad(x, dev["residual"], scale, beta=dev["beta"], coef=dev["coef_loss"], gain=x["gl"]).get())
    for name, b in (("plain", None), ("welsch", bp)):
        g = _normal(x, scale, brightness, beta_prev=b, fixed=None)
        out.update({f"{name}_{k}": g[k].get() for k in ("normal", "residual", "shifts_out")})      # (the tile sums are laid out by tile)
    return out


@pytest.mark.parametrize("c", BATCHED[::2], ids=OC.case_id)
def test_runs_are_bit_equal_and_a_sample_does_not_depend_on_its_batch_or_on_appended_views(c):
    shape, scale, kind, mkind, akind, brightness = c
    B, V, H, W = shape
    x = OC.inputs(c)
    bp = _reference(c)["beta_prev"]
    a, again = _all_bits(x, scale, brightness, bp), _all_bits(x, scale, brightness, bp)
    assert all(_bits(a[k], again[k]) for k in a)
    for b in range(B):
        one = {k: (None if v is None else v[b:b + 1]) for k, v in x.items()}
        o = _all_bits(one, scale, brightness, bp[b:b + 1])
        assert all(_bits(o[k][0], a[k][b]) for k in a), b
    # three more views with alpha 0 (random data, clear masks, shifts of every kind, one NaN): no bit of the first V views' results moves,
    # the appended views have no gradient and keep their shifts' bits
    rng = np.random.Generator(np.random.PCG64(77))
    more = dict(x)
    more["lrs"] = np.concatenate([x["lrs"], rng.uniform(0, 1, (B, 3, H, W)).astype(np.float32)], 1)
    more["g"] = np.concatenate([x["g"], rng.uniform(-1, 1, (B, 3, H, W)).astype(np.float32)], 1)
    more["masks"] = None if x["masks"] is None else np.concatenate([x["masks"], np.ones((B, 3, H, W), np.float32)], 1)
    more["alphas"] = np.concatenate([np.ones((B, V), np.float32) if x["alphas"] is None else x["alphas"], np.zeros((B, 3), np.float32)], 1)
    extra = rng.uniform(-2, 2, (B, 3, 2)).astype(np.float32)
    extra[:, 1, 0] = np.nan
    more["shifts"] = np.concatenate([x["shifts"], extra], 1)
    m = _all_bits(more, scale, brightness, np.concatenate([bp, np.zeros((B, 3), np.float32)], 1))
    for k in a:
        if k == "d_obs":
            continue                                     # observe has no alphas: its appended views are ordinary views
        assert _bits(m[k][:, :V], a[k]), k
        if "shifts_out" in k:
            assert _bits(m[k][:, V:], torch.from_numpy(extra)), k
        else:
            assert not m[k][:, V:].any(), k
    assert _bits(m["d_obs"][:, :V], a["d_obs"])


def _case_tensors(scale=3, kind="random"):
    c = next(c for c in PLAN if c[0] == OC.SHAPES[4] and c[1] == scale and c[2] == kind)
    x = OC.inputs(c)
    return c, x, tuple(_dev(x[k]) for k in ("hr", "lrs", "masks", "alphas", "shifts", "g", "gl"))


def test_ops_pass_opcheck_and_their_gradients_are_the_restatements():
    from hrnet_hip import observation
    ops = torch.ops.hrnet_hip
    checks = ("test_schema", "test_faketensor", "test_autograd_registration")
    c, x, (hr, lrs, masks, alphas, shifts, g, gl) = _case_tensors()
    shape, scale, kind, mkind, akind, brightness = c
    want = _reference(c)
    req = lambda t: t.clone().requires_grad_(True)
    loss, residual, beta, count, coef = ops.consistency_loss_train(hr, lrs, masks, alphas, shifts, scale, brightness)
    fixed = torch.zeros(shape[:2], dtype=U8, device="cuda")
    fixed[:, 0] = 1
    torch.library.opcheck(ops.observe_sg.default, (req(hr), req(shifts), scale), test_utils=checks)
    torch.library.opcheck(ops.consistency_loss_sg.default, (req(hr), lrs, masks, alphas, req(shifts), scale, brightness), test_utils=checks)
    torch.library.opcheck(ops.consistency_loss_sg.default, (hr, lrs, None, None, req(shifts), scale, True), test_utils=checks)
    torch.library.opcheck(ops.observe_shift_backward.default, (hr, residual, masks, alphas, shifts, beta, coef, gl, scale), test_utils=checks)
    torch.library.opcheck(ops.observe_shift_backward.default, (hr, g, None, None, shifts, None, None, None, scale), test_utils=checks)
    torch.library.opcheck(ops.shift_normal.default, (hr, lrs, masks, alphas, shifts, None, scale, brightness, 0.1), test_utils=checks)
    torch.library.opcheck(ops.shift_normal.default, (hr, lrs, None, None, shifts, beta, scale, True, 0.1), test_utils=checks)
    torch.library.opcheck(ops.refine_shifts.default, (hr, lrs, masks, alphas, shifts, fixed, scale, 2, 1e-3, 0.5, brightness, False, 0.1),
                          test_utils=checks)
    torch.library.opcheck(ops.refine_shifts.default, (hr, lrs, None, None, shifts, None, scale, 0, 1e-3, 0.5, True, True, 0.1), test_utils=checks)
    torch.library.opcheck(ops.reconstruct_joint.default, (hr, lrs, masks, alphas, shifts, fixed, scale, 3, 1, 1, 1e-3, 0.5, 1.0, brightness, True,
                                                          0.1, 4e-4, 2, 0.7, 0.02), test_utils=checks)
    # forward bits are the existing ops'; the gradients are the restatement's; either half alone gives the bits of both together
    def loss_grads(frame_grad, shift_grad):
        f, s = hr.clone().requires_grad_(frame_grad), shifts.clone().requires_grad_(shift_grad)
        L = observation.consistency_loss(f, lrs, s, masks, alphas, scale, brightness, shift_grad=True)
        assert torch.equal(L, loss)
        (L * gl).sum().backward()
        return f.grad, s.grad

    both, fonly, sonly = loss_grads(True, True), loss_grads(True, False), loss_grads(False, True)
    assert fonly[1] is None and sonly[0] is None and _bits(fonly[0], both[0]) and _bits(sonly[1], both[1])
    _close("op d_shifts loss", both[1].cpu(), want["d_loss"], want["T_d_loss"], "b v a")
    f0 = req(hr)
    (observation.consistency_loss(f0, lrs, shifts, masks, alphas, scale, brightness) * gl).sum().backward()
    assert _bits(f0.grad, both[0])

    def observe_grads(frame_grad, shift_grad):
        f, s = hr.clone().requires_grad_(frame_grad), shifts.clone().requires_grad_(shift_grad)
        views, valid = observation.observe(f, s, scale, shift_grad=True)
        assert not valid.requires_grad
        views.backward(g)
        return f.grad, s.grad, views.detach()

    both, fonly, sonly = observe_grads(True, True), observe_grads(True, False), observe_grads(False, True)
    assert fonly[1] is None and sonly[0] is None and _bits(fonly[0], both[0]) and _bits(sonly[1], both[1])
    assert _bits(both[2], observation.observe(hr, shifts, scale)[0])
    _close("op d_shifts observe", both[1].cpu(), want["d_obs"], want["T_d_obs"], "b v a")
    # shift_normal and refine_shifts are the C entry points
    n = observation.shift_normal(hr, lrs, shifts, masks, alphas, scale, brightness)
    dev = _normal(x, scale, brightness, fixed=R.fixed_mask(0, *shape[:2]))
    assert _bits(n.cpu(), dev["normal"].get())
    one, trace = observation.refine_shifts(hr, lrs, shifts, masks, alphas, scale, iters=1, brightness=brightness, return_trace=True)
    assert _bits(one.cpu(), dev["shifts_out"].get()) and _bits(trace[0].cpu(), dev["normal"].get()) and not one.requires_grad
    zero = observation.refine_shifts(hr, lrs, shifts, masks, alphas, scale, iters=0)
    assert _bits(zero, shifts) and zero.data_ptr() != shifts.data_ptr()


def test_only_the_halves_that_are_needed_are_launched_and_the_default_path_is_the_old_ops():
    from hrnet_hip import observation
    c, x, (hr, lrs, masks, alphas, shifts, g, gl) = _case_tensors()
    scale, brightness = c[1], c[5]

    def families(shift_grad, frame_grad, shifts_req):
        f, s = hr.clone().requires_grad_(frame_grad), shifts.clone().requires_grad_(shifts_req)
        binding.profile_enable(True)
        L = observation.consistency_loss(f, lrs, s, masks, alphas, scale, brightness, shift_grad=shift_grad)
        L.sum().backward()
        views, _ = observation.observe(f, s, scale, shift_grad=shift_grad)
        views.backward(g)
        torch.cuda.synchronize()
        rec = binding.profile_read()
        binding.profile_enable(False)
        assert (s.grad is not None) == (shift_grad and shifts_req)
        return {name: r["launches"] for name, r in rec.items()}

    old = {"consistency_residual": 1, "consistency_finish": 1, "observe": 1, "observe_adjoint": 2}
    new = {"observe_shift_grad": 2, "observe_shift_grad_finish": 2}
    assert families(False, True, True) == old
    assert families(True, True, False) == old
    assert families(True, True, True) == {**old, **new}
    assert families(True, False, True) == {"consistency_residual": 1, "consistency_finish": 1, "observe": 1, **new}


@pytest.mark.parametrize("robust", [None, "welsch"])
def test_refine_every_zero_is_reconstruct_and_fixing_every_view_keeps_the_shifts(robust):
    from hrnet_hip import observation
    c, x, (hr, lrs, masks, alphas, shifts, g, gl) = _case_tensors(kind="nan")
    scale, brightness = c[1], c[5]
    kw = dict(iters=4, brightness=brightness, robust=robust, delta=DELTA, lam=4e-4)
    want = observation.reconstruct(hr, lrs, shifts, masks, alphas, scale, **kw)
    sr, out = observation.reconstruct_joint(hr, lrs, shifts, masks, alphas, scale, refine_every=0, **kw)
    assert _bits(sr, want) and _bits(out, shifts) and out.data_ptr() != shifts.data_ptr()
    every = torch.ones(c[0][:2], dtype=torch.bool, device="cuda")
    sr, out = observation.reconstruct_joint(hr, lrs, shifts, masks, alphas, scale, fixed=every, **kw)
    assert _bits(sr, want) and _bits(out, shifts)
    sr, out = observation.reconstruct_joint(hr[:, None], lrs, shifts, masks, alphas, scale, **kw)
    assert tuple(sr.shape) == (c[0][0], 1) + tuple(hr.shape[1:]) and _bits(out[:, 0], shifts[:, 0]) and not _bits(out, shifts)
    assert bool(torch.isfinite(sr).all())


def test_register_and_refine_joint_and_the_baseline_table_run_the_joint_iteration():
    """the two wrappers: register_and_refine(joint=True) is its own search and start followed by reconstruct_joint, and
    validate.baseline_table(method="joint") scores that call"""
    import shift_add_scene as SS
    from hrnet_hip import observation, registration, shiftadd, validate
    sc = SS.make(n_lr=32, scale=3, views=5, band=0.25, limit=1.0, noise=0.005, clouds=1, margin=3.0, seed=2)
    lrs, masks = util.dev(sc["lrs"]), util.dev(sc["masks"])
    search = dict(points_per_dim=5, levels=6, radius=2.0)
    sr, shifts = observation.register_and_refine(lrs, masks, None, scale=3, iters=4, joint=True, **search)
    sr0, _, found = shiftadd.register_and_add(lrs, masks, None, scale=3, **search)
    want_sr, want_shifts = observation.reconstruct_joint(sr0, lrs, found, masks, None, 3, 4, step=1.0, robust=None, lam=0.0)
    assert _bits(sr, want_sr) and _bits(shifts, want_shifts) and _bits(shifts[:, 0], found[:, 0]) and not _bits(shifts, found)
    plain, same = observation.register_and_refine(lrs, masks, None, scale=3, iters=4, **search)
    assert _bits(same, found) and not _bits(plain, sr)
    hrs, maps = util.dev(sc["hr"][None].astype(np.float32)), torch.ones((1, 96, 96), device="cuda")
    batch = [(lrs, torch.ones((1, 5), device="cuda"), hrs, maps, ["scene"], masks)]
    joint = validate.baseline_table(batch, method="joint", iters=4, **search)
    again = validate.baseline_table(batch, method="back_projection", iters=4, joint=True, **search)
    back = validate.baseline_table(batch, method="back_projection", iters=4, **search)
    assert set(joint) == {"scene"} and joint == again and joint != back and np.isfinite(joint["scene"])


def test_frames_beyond_2_31_elements():
    """57 samples of two 2048 x 2048 views at x3: hr holds 57 x 6144^2 = 2.15e9 elements (past 2^31) in 8.6e9 bytes (past 2^32), 1.87M
    tiles walked by a grid of 2^16 workgroups.  d_shifts of both views of sample 0 and of sample 56 against the restatement formed in fp64
    on the device (its matrices are tests/observe_ref.py's and tests/observe_shift_ref.py's); every other sample's must be finite."""
    n, V, side, scale = 57, 2, 2048, 3
    KB._need(22)
    pool = KB._Pool()
    try:
        SH = scale * side
        per = SH * SH
        assert n * per > 1 << 31 and 4 * n * per > 1 << 32
        hr = pool.big(n, (SH, SH), KB.F32, fill="rand", seed=13, scale=0.5)
        rng = np.random.Generator(np.random.PCG64(57))
        shifts_np = rng.uniform(-1.5, 1.5, (n, V, 2)).astype(np.float32)
        shifts = pool.keep(util.dev(shifts_np))
        g = pool.keep(torch.rand((n, V, side, side), device="cuda", generator=torch.Generator(device="cuda").manual_seed(3)) - 0.5)
        nbytes = kt.lib().hrn_observe_shift_workspace_bytes(n, V, side, side)
        ws = pool.keep(torch.empty((nbytes // 8,), dtype=F64, device="cuda"))
        out = KB.Guarded((n, V, 2))
        before = hr.checksum()
        rc = kt.lib().hrn_observe_shift_grad(hr.ptr, kt._p(g), None, None, kt._p(shifts), None, kt._p(ws), nbytes, n, V, side, side, scale, kt._stream())
        torch.cuda.synchronize()
        assert rc == 0, binding.load_library().hrn_last_error()
        _rc(kt.lib().hrn_observe_shift_grad_finish(kt._p(ws), nbytes, None, None, out.ptr, n, V, side, side, kt._stream()), out)
        assert hr.guards_intact() and hr.checksum() == before
        got = out.get().double()
        assert bool(torch.isfinite(got).all()) and bool((got != 0).all())
        for k in (0, n - 1):
            f = hr.raw[2 * k * per:2 * (k + 1) * per].view(torch.float32).view(SH, SH).double()
            for v in range(V):
                dy, dx = shifts_np[k, v]
                Ay, Ax = (torch.from_numpy(O.axis_matrix(side, scale, d)).cuda() for d in (dy, dx))
                Oy, Ox = (torch.from_numpy(R.slope_matrix(side, scale, d)).cuda() for d in (dy, dx))
                gd = g[k, v].double()
                want = torch.stack([(gd * (Oy @ f @ Ax.T)).sum(), (gd * (Ay @ f @ Ox.T)).sum()]).cpu()
                T = torch.stack([(gd.abs() * (Oy.abs() @ f.abs() @ Ax.abs().T)).sum(), (gd.abs() * (Ay.abs() @ f.abs() @ Ox.abs().T)).sum()]).cpu()
                _close(f"d_shifts, sample {k} view {v}", got[k, v], want.numpy(), T.numpy(), "a")
                del Ay, Ax, Oy, Ox, gd
            del f
    finally:
        pool.free()
