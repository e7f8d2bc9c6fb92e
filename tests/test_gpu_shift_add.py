"""GPU (-m gpu): hrn_shift_add and hrn_shift_add_backward (csrc/shift_add.hip) against the fp64 restatement (tests/shift_add_ref.py) under
the project's bound |got - want| <= C T, C = 1e-5 (tests/kernel_bounds.py), T the restatement's sum of absolute terms (for `weight`,
T = D): the 126 cases of tests/shift_add_cases.py - six shapes around the kernels' tile, every scale, sigma and prior, whole, half,
almost-whole, random, far and NaN shifts, four kinds of masks, three of alphas.  The pixels whose restatement D + prior lies in
[2^-21, 2^-19] (the fallback's threshold) are left out; tests/test_shift_add_host.py holds them to 0.1 % of a case.  Further: exact zeros of
D, the fallback, sentinels behind every output, the in-place base, reproducibility, independence of the batch and of appended alpha-0
views, constants, the adjoint identity, the dispatcher ops with their autograd formula, and an output past 2^31 elements."""
import numpy as np
import pytest
import torch

import kernel_bounds as KB
import kt
import shift_add_cases as SC
import shift_add_ref as R
import util
from hrnet_hip import binding

pytestmark = pytest.mark.gpu

PLAN = SC.plan()
_dev = lambda a: None if a is None else util.dev(a)


def test_the_cases_use_the_kernels_tile():
    assert binding.SHIFT_ADD_TILE == (SC.TH, SC.TW)


def _forward(x, scale, sigma, prior, base="apart", weight=True):
    """hrn_shift_add into sentinel-guarded outputs.  base: "apart" (its own tensor), "inplace" (out starts as base and is handed over as
    base too) or None -> (out, weight or None), both Guarded"""
    B, V, H, W = x["views"].shape
    shp = (B, scale * H, scale * W)
    views, masks, alphas, shifts = _dev(x["views"]), _dev(x["masks"]), _dev(x["alphas"]), _dev(x["shifts"])
    out = KB.Guarded(shp, v=torch.from_numpy(x["base"]) if base == "inplace" else None)
    wt = KB.Guarded(shp) if weight else None
    b = _dev(x["base"]) if base == "apart" else None
    rc = kt.lib().hrn_shift_add(kt._p(views), kt._p(masks), kt._p(alphas), kt._p(shifts), out.ptr if base == "inplace" else kt._p(b), out.ptr,
                                wt.ptr if weight else None, B, V, H, W, scale, sigma, prior, kt._stream())
    torch.cuda.synchronize()
    assert rc == 0, binding.load_library().hrn_last_error()
    assert out.guard_ok() and (wt is None or wt.guard_ok()), "a write outside an output"
    return out, wt


def _backward(x, weight, scale, sigma, prior, views=True, base=True):
    """hrn_shift_add_backward at x["g"] with the fp32 `weight` -> (d_views, d_base), Guarded or None"""
    B, V, H, W = x["views"].shape
    g, w, masks, alphas, shifts = _dev(x["g"]), _dev(weight), _dev(x["masks"]), _dev(x["alphas"]), _dev(x["shifts"])
    dv = KB.Guarded((B, V, H, W)) if views else None
    db = KB.Guarded(tuple(g.shape)) if base else None
    rc = kt.lib().hrn_shift_add_backward(kt._p(g), kt._p(w), kt._p(masks), kt._p(alphas), kt._p(shifts), dv.ptr if views else None,
                                         db.ptr if base else None, B, V, H, W, scale, sigma, prior, kt._stream())
    torch.cuda.synchronize()
    assert rc == 0, binding.load_library().hrn_last_error()
    assert (dv is None or dv.guard_ok()) and (db is None or db.guard_ok()), "a write outside a gradient"
    return dv, db


def _close(tag, got, want, T, keep=None, layout="b y x"):
    got, want, T = got.double(), torch.from_numpy(np.asarray(want, np.float64)), torch.from_numpy(np.asarray(T, np.float64))
    assert bool(torch.isfinite(got).all()), f"{tag}: a non-finite value"
    if keep is not None:
        got = torch.where(torch.from_numpy(keep), got, want)
    return KB._assert_close(tag, "f32", got, want, T, layout=layout)


@pytest.mark.parametrize("c", PLAN, ids=SC.case_id)
def test_forward_against_the_restatement(c):
    shape, scale, kind, sigma, prior, mkind, akind = c
    x, ref = SC.inputs(c), SC.reference(c)
    tag = SC.case_id(c)
    out, wt = _forward(x, scale, sigma, prior)
    _close(f"out {tag}", out.get(), ref["out"], ref["T"], ref["keep"])
    _close(f"weight {tag}", wt.get(), ref["D"], ref["D"], ref["keep"])
    # no sample reaches: D is the restatement's zero exactly; under the threshold (by more than a factor of two) the result is the base
    zero = torch.from_numpy(ref["D"] == 0)
    assert bool((wt.get()[zero] == 0).all())
    fallback = torch.from_numpy(ref["den"] < 2.0 ** -21)
    assert torch.equal(out.get()[fallback], torch.from_numpy(x["base"])[fallback])
    if akind == "sample-zero":
        assert bool(fallback[-1].all()) if prior == 0 else bool(zero[-1].all())
    # the in-place base, and the result without its second output: the same bits
    inplace, _ = _forward(x, scale, sigma, prior, base="inplace", weight=False)
    assert torch.equal(inplace.bits(), out.bits())
    if prior == 0:                                                   # base NULL: 0 where nothing reaches, the same bits elsewhere
        ref0 = SC.reference(c, False)
        bare, wt0 = _forward(x, scale, sigma, prior, base=None)
        _close(f"out, no base {tag}", bare.get(), ref0["out"], ref0["T"], ref0["keep"])
        assert torch.equal(wt0.bits(), wt.bits()) and bool((bare.get()[fallback] == 0).all())
        reached = torch.from_numpy(ref["den"] > 2.0 ** -19)
        assert torch.equal(bare.get()[reached], out.get()[reached])


@pytest.mark.parametrize("c", PLAN, ids=SC.case_id)
def test_backward_against_the_restatement(c):
    shape, scale, kind, sigma, prior, mkind, akind = c
    x, ref = SC.inputs(c), SC.reference_adjoint(c)
    tag = SC.case_id(c)
    dv, db = _backward(x, ref["weight"], scale, sigma, prior)
    _close(f"d_views {tag}", dv.get(), ref["d_views"], ref["T_views"], layout="b v y x")
    _close(f"d_base {tag}", db.get(), ref["d_base"], ref["T_base"])
    # a view that does not count and a masked pixel get an exact zero
    assert bool((dv.get()[torch.from_numpy(ref["T_views"] == 0)] == 0).all())
    # each half alone: the same bits
    dv1, none = _backward(x, ref["weight"], scale, sigma, prior, base=False)
    none2, db1 = _backward(x, ref["weight"], scale, sigma, prior, views=False)
    assert none is None and none2 is None and torch.equal(dv1.bits(), dv.bits()) and torch.equal(db1.bits(), db.bits())


@pytest.mark.parametrize("c", PLAN[3::5], ids=SC.case_id)
def test_adjoint_identity_of_the_device_results(c):
    """out is linear in (views, base) with D held: <out, g> = <views, d_views> + <base, d_base>, the device's results summed in fp64"""
    shape, scale, kind, sigma, prior, mkind, akind = c
    x, ref = SC.inputs(c), SC.reference(c)
    out, wt = _forward(x, scale, sigma, prior)
    dv, db = _backward(x, wt.get().numpy(), scale, sigma, prior)             # the device's own D: both sides take the same fallbacks
    adj = SC.reference_adjoint(c)
    g, views, base = x["g"].astype(np.float64), x["views"].astype(np.float64), x["base"].astype(np.float64)
    lhs = float((out.get().double().numpy() * g).sum())
    rhs = float((views * dv.get().double().numpy()).sum() + (base * db.get().double().numpy()).sum())
    bound = KB.C * (float((ref["T"] * np.abs(g)).sum()) + float((np.abs(views) * adj["T_views"]).sum()) + float((np.abs(base) * adj["T_base"]).sum()))
    print(f"{SC.case_id(c)}: <out, g> - <views, d_views> - <base, d_base> = {lhs - rhs:.3e}, bound {bound:.3e}")
    assert abs(lhs - rhs) <= bound


BATCHED = [c for c in PLAN if c[0][0] == 2 and c[2] in ("random", "nan", "whole-eps")]


@pytest.mark.parametrize("c", BATCHED[::2], ids=SC.case_id)
def test_runs_are_bit_equal_and_a_sample_does_not_depend_on_its_batch_or_on_appended_views(c):
    shape, scale, kind, sigma, prior, mkind, akind = c
    B, V, H, W = shape
    x = SC.inputs(c)
    out, wt = _forward(x, scale, sigma, prior)
    again, wt2 = _forward(x, scale, sigma, prior)
    assert torch.equal(out.bits(), again.bits()) and torch.equal(wt.bits(), wt2.bits())
    dv, db = _backward(x, wt.get().numpy(), scale, sigma, prior)
    dv2, db2 = _backward(x, wt.get().numpy(), scale, sigma, prior)
    assert torch.equal(dv.bits(), dv2.bits()) and torch.equal(db.bits(), db2.bits())
    for b in range(B):
        one = {k: (None if v is None else v[b:b + 1]) for k, v in x.items()}
        o1, w1 = _forward(one, scale, sigma, prior)
        assert torch.equal(o1.get()[0], out.get()[b]) and torch.equal(w1.get()[0], wt.get()[b]), b
        dv1, db1 = _backward(one, wt.get().numpy()[b:b + 1], scale, sigma, prior)
        assert torch.equal(dv1.get()[0], dv.get()[b]) and torch.equal(db1.get()[0], db.get()[b]), b
    # three more views with alpha 0 (random data, clear masks, shifts of every kind, one NaN): no bit of the results moves
    rng = np.random.Generator(np.random.PCG64(77))
    more = dict(x)
    more["views"] = np.concatenate([x["views"], rng.uniform(0, 1, (B, 3, H, W)).astype(np.float32)], 1)
    more["masks"] = None if x["masks"] is None else np.concatenate([x["masks"], np.ones((B, 3, H, W), np.float32)], 1)
    more["alphas"] = np.concatenate([np.ones((B, V), np.float32) if x["alphas"] is None else x["alphas"], np.zeros((B, 3), np.float32)], 1)
    extra = rng.uniform(-2, 2, (B, 3, 2)).astype(np.float32)
    extra[:, 1, 0] = np.nan
    more["shifts"] = np.concatenate([x["shifts"], extra], 1)
    o3, w3 = _forward(more, scale, sigma, prior)
    assert torch.equal(o3.bits(), out.bits()) and torch.equal(w3.bits(), wt.bits())
    dv3, db3 = _backward(more, wt.get().numpy(), scale, sigma, prior)
    assert torch.equal(dv3.get()[:, :V], dv.get()) and bool((dv3.get()[:, V:] == 0).all()) and torch.equal(db3.bits(), db.bits())


@pytest.mark.parametrize("scale", SC.SCALES)
def test_constant_views_give_the_constant_wherever_a_sample_reaches(scale):
    rng = np.random.Generator(np.random.PCG64(20 + scale))
    B, V, H, W = 2, 5, 2 * SC.TH + 1, 2 * SC.TW - 1
    for sigma in SC.SIGMAS:
        x = dict(views=np.full((B, V, H, W), 0.625, np.float32), masks=(rng.uniform(0, 1, (B, V, H, W)) >= 0.6).astype(np.float32), alphas=None,
                 shifts=rng.uniform(-2.5, 2.5, (B, V, 2)).astype(np.float32), base=np.zeros((B, scale * H, scale * W), np.float32))
        out, wt = _forward(x, scale, sigma, 0.0, base=None)
        o, w = out.get().double(), wt.get().double()
        reached = w >= 2.0 ** -19
        assert bool(reached.any()) and float((o[reached] - 0.625).abs().max()) <= KB.C * 0.625
        assert bool((o[w < 2.0 ** -21] == 0).all())


def test_ops_pass_opcheck_and_their_gradients_are_the_restatements():
    ops = torch.ops.hrnet_hip
    checks = ("test_schema", "test_faketensor", "test_autograd_registration")
    c = (SC.SHAPES[4], 3, "random", 0.25, 0.05, "random", "some-zero")
    shape, scale, kind, sigma, prior, mkind, akind = c
    B, V, H, W = shape
    x = SC.inputs(c)
    views, masks, alphas, shifts, base, g = (_dev(x[k]) for k in ("views", "masks", "alphas", "shifts", "base", "g"))
    torch.library.opcheck(ops.shift_add.default, (views, masks, alphas, shifts, base, scale, sigma, prior), test_utils=checks)
    torch.library.opcheck(ops.shift_add.default, (views.clone().requires_grad_(True), None, None, shifts, None, 2, 0.5, 0.0), test_utils=checks)
    torch.library.opcheck(ops.shift_add.default, (views.clone().requires_grad_(True), masks, alphas, shifts, base.clone().requires_grad_(True),
                                                  scale, sigma, prior), test_utils=checks)
    out, wt = ops.shift_add(views, masks, alphas, shifts, base, scale, sigma, prior)
    for nv, nb in ((True, True), (True, False), (False, True)):
        torch.library.opcheck(ops.shift_add_backward.default, (g, wt, masks, alphas, shifts, V, H, W, scale, sigma, prior, nv, nb), test_utils=checks)
    # the ops are the C entry points
    o_c, w_c = _forward(x, scale, sigma, prior)
    assert torch.equal(out.cpu(), o_c.get()) and torch.equal(wt.cpu(), w_c.get())
    dv_c, db_c = _backward(x, w_c.get().numpy(), scale, sigma, prior)
    dv, db = ops.shift_add_backward(g, wt, masks, alphas, shifts, V, H, W, scale, sigma, prior, True, True)
    assert torch.equal(dv.cpu(), dv_c.get()) and torch.equal(db.cpu(), db_c.get())
    dv_only, empty = ops.shift_add_backward(g, wt, masks, alphas, shifts, V, H, W, scale, sigma, prior, True, False)
    assert torch.equal(dv_only, dv) and empty.numel() == 0
    # autograd through hrnet_hip.shiftadd: d_lrs and d_base are the restatement's adjoint at the device's own weight; each only when asked
    from hrnet_hip import shiftadd
    adj = R.adjoint(x["g"], w_c.get().numpy(), x["masks"], x["alphas"], x["shifts"], V, H, W, scale, sigma, prior)
    vr, br = views.clone().requires_grad_(True), base.clone().requires_grad_(True)
    sr, weight = shiftadd.shift_and_add(vr, shifts, masks, alphas, scale, sigma, prior, base=br, return_weight=True)
    assert torch.equal(sr, out) and torch.equal(weight, wt) and not weight.requires_grad
    sr.backward(g)
    _close("op d_lrs", vr.grad.cpu(), adj[0], adj[1], layout="b v y x")
    _close("op d_base", br.grad.cpu(), adj[2], adj[3])
    assert torch.equal(vr.grad, dv) and torch.equal(br.grad, db)
    vr2 = views.clone().requires_grad_(True)
    shiftadd.shift_and_add(vr2, shifts, masks, alphas, scale, sigma, prior, base=base).backward(g)
    assert torch.equal(vr2.grad, dv) and base.grad is None and shifts.grad is None
    br2 = base.clone().requires_grad_(True)
    shiftadd.shift_and_add(views, shifts, masks, alphas, scale, sigma, prior, base=br2).backward(g)
    assert torch.equal(br2.grad, db) and views.grad is None
    # base="bicubic" is upsample.baseline taken as data; None needs prior 0
    from hrnet_hip import upsample
    auto = shiftadd.shift_and_add(views, shifts, masks, alphas, scale, sigma, prior)
    bic = upsample.baseline(views, alphas, masks, scale)[:, 0]
    assert torch.equal(auto, ops.shift_add(views, masks, alphas, shifts, bic, scale, sigma, prior)[0])
    bare = shiftadd.shift_and_add(views, shifts, masks, alphas, scale, sigma, 0, base=None)
    assert torch.equal(bare, ops.shift_add(views, masks, alphas, shifts, None, scale, sigma, 0.0)[0])


def test_output_beyond_2_31_elements():
    """57 samples of one 2048 x 2048 view at x3 with `weight` NULL: 57 x 6144^2 = 2.15e9 output elements (past 2^31) in 8.6e9 bytes (past
    2^32), 934k tiles walked by a grid of 2^16 workgroups.  Checked on sampled rows - the first and last, the rows beside the tile seams,
    and random ones - of sample 0, the last sample and the samples every boundary falls into, against the restatement formed in fp64 on
    the device (its matrices are tests/shift_add_ref.py's)."""
    n, side, scale, sigma = 57, 2048, 3, 0.25
    KB._need(12)
    pool = KB._Pool()
    try:
        per = (scale * side) ** 2
        assert n * per > 1 << 31 and 4 * n * per > 1 << 32
        views = pool.big(n, (side, side), KB.F32, fill="rand", seed=13, scale=0.5)
        out = pool.big(n, (scale * side, scale * side), KB.F32, fill="sent")
        rng = np.random.Generator(np.random.PCG64(57))
        shifts_np = rng.uniform(-1.5, 1.5, (n, 1, 2)).astype(np.float32)
        shifts = pool.keep(util.dev(shifts_np))
        before = views.checksum()
        rc = kt.lib().hrn_shift_add(views.ptr, None, None, kt._p(shifts), None, out.ptr, None, n, 1, side, side, scale, sigma, 0.0, kt._stream())
        torch.cuda.synchronize()
        assert rc == 0, binding.load_library().hrn_last_error()
        assert out.guards_intact() and views.guards_intact() and views.checksum() == before
        planes = KB.boundary_images(n, per, 4)
        assert planes[0] == 0 and planes[-1] == n - 1 and len(planes) >= 4
        SH = scale * side
        rows = sorted({0, 1, SH - 2, SH - 1, scale * SC.TH - 1, scale * SC.TH, SH // 2 - 1, SH // 2} | set(int(r) for r in rng.integers(0, SH, 24)))
        for k in planes:
            Wy = torch.from_numpy(R.axis_matrix(side, scale, shifts_np[k, 0, 0], sigma, rows=rows)).cuda()
            Wx = pool.keep(torch.from_numpy(R.axis_matrix(side, scale, shifts_np[k, 0, 1], sigma)).cuda())
            f = views.raw[2 * k * side * side:2 * (k + 1) * side * side].view(torch.float32).view(side, side).double()
            N, D, A = Wy @ f @ Wx.T, Wy @ torch.ones_like(f) @ Wx.T, Wy @ f.abs() @ Wx.T
            # a shifted view leaves a band along two borders that no sample reaches: 0 there (base NULL), and the pixels at the
            # threshold are left out, as in every other case
            ok, keep = D >= 2.0 ** -20, (D < 2.0 ** -21) | (D > 2.0 ** -19)
            safe = torch.where(ok, D, torch.ones_like(D))
            want, T = torch.where(ok, N / safe, torch.zeros_like(N)), torch.where(ok, A / safe, torch.zeros_like(A))
            # (the border rows are among the sampled ones: whole rows of them may be unreached, or lie at the threshold at some phases)
            assert float(keep.double().mean()) >= 0.9 and float((ok & keep).double().mean()) >= 0.75
            got = out.raw[2 * k * per:2 * (k + 1) * per].view(torch.float32).view(SH, SH)[rows].double()
            ratio = float(((got - want).abs() / (KB.C * T + 1e-300))[keep].max())
            print(f"sample {k}: max error / bound {ratio:.3e}; C needed {ratio * KB.C:.2e}")
            assert ratio <= 1.0, k
            del f, N, D, A, want, T, got, Wy, ok, keep, safe
    finally:
        pool.free()
