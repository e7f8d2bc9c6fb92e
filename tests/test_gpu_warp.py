"""GPU: the backward of the six-tap sampler (hrn_mncc_apply_backward, the ops hrnet_hip::warp / warp_backward and
hrnet_hip.registration.warp) against the fp64 restatement (tests/warp_ref.py).

Shapes: 24 x 40 (one partial tile), 33 x 47, and 130 x 203 in a batch of two (seams at 64 and 128 on both axes, a last tile of 2 rows and
11 columns).  Frames and masks are registration_ref.scene's, d_out is standard normal.  Every shape meets every shift of SHIFTS: its views
cycle through them over as many sets as that takes.  (30, 0) leaves nothing valid on the 24-row frame, (300, 0) nothing anywhere;
(2, 0) and (0, 0) sit on whole pixels, where the sampler is C^1 but not C^2; (0.9999999, -1e-7) sits next to them on either side.

The bounds are kernel_bounds' |got - want| <= rounding + C T with its one constant C = 1e-5 and T the same sums over absolute values
(warp_ref.magnitudes); d_shifts is rounded to fp32 once, hence its 2^-24 |want|.  "C needed" is printed per case; the largest on an
MI355X: 2.33e-7 for d_views (2x2x130x203-set1), 4.16e-9 for d_shifts (1x2x24x40-set2).  The controls apply four mistakes to the
RESTATEMENT and require the same bound to reject each on at least one case (they are rejected on 9, 9, 9 and 8 of the 9)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import kernel_bounds as KB
import registration_ref as R
import warp_ref as WR

pytestmark = pytest.mark.gpu

SHAPES = [(1, 2, 24, 40), (1, 3, 33, 47), (2, 2, 130, 203)]
IDS = ["x".join(map(str, s)) for s in SHAPES]
SHIFTS = WR.SHIFTS
SENTINEL = 0x7F7F7F7F


def _sets(B, V):
    return -(-len(SHIFTS) // (B * V))


CASES = [(s, k) for s in SHAPES for k in range(_sets(s[0], s[1]))]
CASE_IDS = [f"{'x'.join(map(str, s))}-set{k}" for s, k in CASES]


def _cuda(*arrays):
    return tuple(None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays)


def _nothing_valid(shift, H, W):
    return not R.inside((H, W), shift).any()


@functools.lru_cache(maxsize=None)
def case(shape, k):
    """One set of shifts on one shape, with what the device's forward says is valid and the fp64 restatement of both gradients:
    a dict of numpy arrays, computed once and shared (read only)."""
    B, V, H, W = shape
    shifts = np.array([SHIFTS[(k * B * V + i) % len(SHIFTS)] for i in range(B * V)], np.float32).reshape(B, V, 2)
    scenes = [R.scene(H, W, R.random_shifts(V, 0.9, seed=7 * b + k), seed=100 * b + H * W + k) for b in range(B)]
    views, masks = np.stack([s[2] for s in scenes]), np.stack([s[3] for s in scenes])
    d_out = np.random.default_rng(H * W + k).standard_normal((B, V, H, W)).astype(np.float32)
    from hrnet_hip import binding
    out, valid = binding.mncc_apply_scene(*_cuda(views, masks, shifts))
    valid = valid.cpu().numpy()
    c = dict(shape=shape, shifts=shifts, views=views, masks=masks, d_out=d_out, valid=valid, out=out.cpu().numpy(),
             dv=np.zeros((B, V, H, W)), dv_mag=np.zeros((B, V, H, W)), ds=np.zeros((B, V, 2)), ds_mag=np.zeros((B, V, 2)))
    for b in range(B):
        for v in range(V):
            a = (views[b, v], d_out[b, v], valid[b, v], shifts[b, v])
            c["dv"][b, v] = WR.d_views(*a[1:])
            c["ds"][b, v] = WR.d_shifts(*a)
            c["dv_mag"][b, v], c["ds_mag"][b, v] = WR.magnitudes(*a)
    return c


def _views_of(c):
    B, V = c["shape"][:2]
    return [(b, v, tuple(float(x) for x in c["shifts"][b, v])) for b in range(B) for v in range(V)]


@functools.lru_cache(maxsize=None)
def device(shape, k):
    """(d_views, d_shifts) of the C entry point into buffers prefilled with a sentinel, as numpy float32"""
    from hrnet_hip import binding
    c = case(shape, k)
    B, V, H, W = shape
    lib = binding.load_library()
    views, shifts, valid, d_out = _cuda(c["views"], c["shifts"], c["valid"], c["d_out"])
    dv = torch.full((B, V, H, W), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
    ds = torch.full((B, V, 2), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
    nbytes = lib.hrn_mncc_apply_backward_workspace_bytes(B, V, H, W)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = lib.hrn_mncc_apply_backward(p(views), p(shifts), p(valid), p(d_out), B, V, H, W, p(dv), p(ds), p(ws), nbytes, ctypes.c_void_p(0))
    assert rc == 0, lib.hrn_last_error()
    torch.cuda.synchronize()
    return dv.cpu().numpy(), ds.cpu().numpy()


def test_the_cases_cover_every_shift_on_every_shape():
    for shape in SHAPES:
        seen = set()
        for k in range(_sets(*shape[:2])):
            seen |= {s for _, _, s in _views_of(case(shape, k))}
        assert seen == {tuple(float(np.float32(x)) for x in s) for s in SHIFTS}
    assert _nothing_valid((30.0, 0.0), 24, 40) and all(_nothing_valid((300.0, 0.0), *s[2:]) for s in SHAPES)


# ----------------------------------------------------------------------------- 1. the forward
@pytest.mark.parametrize("shape,k", CASES, ids=CASE_IDS)
def test_warp_forward_is_shift_scene(shape, k):
    from hrnet_hip import registration
    c = case(shape, k)
    views, masks, shifts = _cuda(c["views"], c["masks"], c["shifts"])
    for m in (masks, None):
        want_out, want_valid = registration.shift_scene(views, m, shifts)
        got_out, got_valid = registration.warp(views, shifts, m)
        assert torch.equal(got_out, want_out) and torch.equal(got_valid, want_valid)
        got_out, got_valid = registration.warp(views.clone().requires_grad_(True), shifts.clone().requires_grad_(True), m)
        assert torch.equal(got_out, want_out) and torch.equal(got_valid, want_valid)
        assert got_out.requires_grad and not got_valid.requires_grad
    # (B,H,W) frames with (B,2) shifts are the same planes
    want_out, want_valid = registration.shift_scene(views, masks, shifts)
    o3, v3 = registration.warp(views[:, 0], shifts[:, 0], masks[:, 0])
    assert torch.equal(o3, want_out[:, 0]) and torch.equal(v3, want_valid[:, 0])
    assert np.array_equal(want_out.cpu().numpy(), c["out"]) and np.array_equal(want_valid.cpu().numpy(), c["valid"])


# ----------------------------------------------------------------------------- 2. d_views per element
@pytest.mark.parametrize("shape,k", CASES, ids=CASE_IDS)
def test_d_views_per_element(shape, k):
    c = case(shape, k)
    got, _ = device(shape, k)
    assert not (got.view(np.int32) == SENTINEL).any(), "an element of d_views was not written"
    assert np.all(np.isfinite(got))
    g, want, mag = (torch.from_numpy(np.asarray(a, np.float64)) for a in (got, c["dv"], c["dv_mag"]))
    KB._assert_close(f"d_views {CASE_IDS[CASES.index((shape, k))]}", "f32", g, want, mag, layout="b v y x")
    zero = c["dv_mag"] == 0.0
    assert np.all(got[zero] == 0.0), "a structural zero of d_views is not exactly 0"
    for b, v, s in _views_of(c):
        if _nothing_valid(s, *shape[2:]):
            assert not got[b, v].any() and not c["dv"][b, v].any()
        else:
            assert np.abs(got[b, v]).max() > 0.1 and zero[b, v].mean() < 0.9


# ----------------------------------------------------------------------------- 3. d_shifts
@pytest.mark.parametrize("shape,k", CASES, ids=CASE_IDS)
def test_d_shifts(shape, k):
    c = case(shape, k)
    _, got = device(shape, k)
    assert not (got.view(np.int32) == SENTINEL).any() and np.all(np.isfinite(got))
    err = np.abs(got.astype(np.float64) - c["ds"])
    bound = 2.0 ** -24 * np.abs(c["ds"]) + KB.C * c["ds_mag"]
    need = float(((err - 2.0 ** -24 * np.abs(c["ds"])).clip(min=0) / (c["ds_mag"] + 1e-300)).max())
    print(f"d_shifts {CASE_IDS[CASES.index((shape, k))]}: max error / bound {float((err / (bound + 1e-300)).max()):.3e}; C needed {need:.2e}; "
          f"got {got.reshape(-1, 2).tolist()} want {c['ds'].reshape(-1, 2).tolist()}")
    assert np.all(err <= bound)
    for b, v, s in _views_of(c):
        if _nothing_valid(s, *shape[2:]):
            assert got[b, v, 0] == 0.0 and got[b, v, 1] == 0.0
        else:
            assert np.abs(c["ds"][b, v]).max() > 0.0 and np.abs(got[b, v]).max() > 0.0


# ----------------------------------------------------------------------------- 4. controls: the bound rejects the four mistakes
def _rejected(wrong_views=None, wrong_shifts=None):
    """on how many cases the device's result fails the bound against a restatement with a mistake in it"""
    n = 0
    for shape, k in CASES:
        c = case(shape, k)
        dv, ds = device(shape, k)
        B, V = shape[:2]
        bad = False
        for b in range(B):
            for v in range(V):
                a = (c["views"][b, v], c["d_out"][b, v], c["valid"][b, v], c["shifts"][b, v])
                if wrong_views:
                    bad |= bool(np.any(np.abs(dv[b, v] - wrong_views(*a[1:])) > KB.C * c["dv_mag"][b, v]))
                if wrong_shifts:
                    w = wrong_shifts(*a)
                    bad |= bool(np.any(np.abs(ds[b, v] - w) > 2.0 ** -24 * np.abs(w) + KB.C * c["ds_mag"][b, v]))
        n += bad
    return n


def test_controls():
    n = {"taps not reversed": _rejected(wrong_views=lambda g, m, s: WR.d_views(g, m, s, reverse=False)),
         "whole part -n": _rejected(wrong_views=lambda g, m, s: WR.d_views(g, m, s, whole=0)),
         "k in place of k'": _rejected(wrong_shifts=lambda T, g, m, s: WR.d_shifts(T, g, m, s, slope=R.taps)),
         "normalisation dropped": _rejected(wrong_shifts=lambda T, g, m, s: WR.d_shifts(T, g, m, s, slope=lambda f: WR.dtaps(f, False)))}
    print("cases on which the bound rejects the mistake, of", len(CASES), ":", n)
    assert all(v >= 1 for v in n.values()), n


# ----------------------------------------------------------------------------- 5. reproducibility
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_bits_are_reproducible_and_independent_of_the_batch(shape):
    from hrnet_hip import binding
    c = case(shape, 0)
    B, V = shape[:2]
    views, shifts, valid, d_out = _cuda(c["views"], c["shifts"], c["valid"], c["d_out"])
    dv, ds = binding.mncc_apply_backward(views, shifts, valid, d_out)
    want_dv, want_ds = device(shape, 0)
    assert np.array_equal(dv.cpu().numpy().view(np.int32), want_dv.view(np.int32))
    assert np.array_equal(ds.cpu().numpy().view(np.int32), want_ds.view(np.int32))
    dv2, ds2 = binding.mncc_apply_backward(views, shifts, valid, d_out)
    assert torch.equal(dv2.view(torch.int32), dv.view(torch.int32)) and torch.equal(ds2.view(torch.int32), ds.view(torch.int32))
    only_v, none = binding.mncc_apply_backward(views, shifts, valid, d_out, True, False)
    assert none is None and torch.equal(only_v.view(torch.int32), dv.view(torch.int32))
    none, only_s = binding.mncc_apply_backward(views, shifts, valid, d_out, False, True)
    assert none is None and torch.equal(only_s.view(torch.int32), ds.view(torch.int32))
    for b in range(B):
        for v in range(V):
            one = tuple(t[b:b + 1, v:v + 1].contiguous() for t in (views, shifts, valid, d_out))
            dv1, ds1 = binding.mncc_apply_backward(*one)
            assert torch.equal(dv1[0, 0].view(torch.int32), dv[b, v].view(torch.int32))
            assert torch.equal(ds1[0, 0].view(torch.int32), ds[b, v].view(torch.int32))


def test_only_the_needed_half_is_launched():
    from hrnet_hip import binding, registration
    c = case(SHAPES[1], 0)
    views, masks, shifts = _cuda(c["views"], c["masks"], c["shifts"])

    def families(frames_grad, shifts_grad):
        f, s = views.clone().requires_grad_(frames_grad), shifts.clone().requires_grad_(shifts_grad)
        out, valid = registration.warp(f, s, masks)
        binding.profile_enable(True)
        (out * valid).sum().backward()
        torch.cuda.synchronize()
        rec = binding.profile_read()
        binding.profile_enable(False)
        assert (f.grad is not None) == frames_grad and (s.grad is not None) == shifts_grad
        return {name: r["launches"] for name, r in rec.items() if name.startswith("mncc_apply_backward")}

    assert families(True, False) == {"mncc_apply_backward_views": 1}
    assert families(False, True) == {"mncc_apply_backward_shifts": 1}
    assert families(True, True) == {"mncc_apply_backward_views": 1, "mncc_apply_backward_shifts": 1}


# ----------------------------------------------------------------------------- 6. autograd end to end
def test_opcheck():
    ops = torch.ops.hrnet_hip
    c = case(SHAPES[1], 0)
    views, masks, shifts, valid, d_out = _cuda(c["views"], c["masks"], c["shifts"], c["valid"], c["d_out"])
    for args in ((views, masks, shifts), (views, None, shifts), (views.clone().requires_grad_(True), masks, shifts),
                 (views, masks, shifts.clone().requires_grad_(True)),
                 (views.clone().requires_grad_(True), None, shifts.clone().requires_grad_(True))):
        torch.library.opcheck(ops.warp.default, args)
    for need in ((True, True), (True, False), (False, True)):
        torch.library.opcheck(ops.warp_backward.default, (views, shifts, valid, d_out) + need)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_autograd_is_the_binding_call(shape):
    from hrnet_hip import binding, registration
    c = case(shape, 0)
    views, masks, shifts = _cuda(c["views"], c["masks"], c["shifts"])
    target = torch.from_numpy(c["out"]).cuda().roll(1, -1)
    f, s = views.clone().requires_grad_(True), shifts.clone().requires_grad_(True)
    warped, valid = registration.warp(f, s, masks)
    warped.retain_grad()
    loss = ((warped - target) ** 2 * valid).sum() / valid.sum()                 # a masked MSE composed in torch
    loss.backward()
    dv, ds = binding.mncc_apply_backward(views, shifts, valid, warped.grad)
    assert torch.equal(f.grad.view(torch.int32), dv.view(torch.int32)) and torch.equal(s.grad.view(torch.int32), ds.view(torch.int32))
    assert f.grad.abs().max() > 0 and s.grad.abs().max() > 0


# ----------------------------------------------------------------------------- 7. descent on the shifts
TRUE = [(0.37, -0.62), (-1.3, 0.7)]
GAIN = 0.1 / 0.11
OFFSET = 0.3 - 0.32 * GAIN


@pytest.mark.parametrize("H,W,seed", [(24, 40, 3), (70, 83, 5)])
def test_descent_on_the_shifts_recovers_them(H, W, seed):
    """Eight steps of s <- s - grad L / diag(J^T J) from truth + (0.3, -0.25), L = 1/2 sum c (a warp + b - ref)^2 with c = ref_mask valid:
    grad L from autograd on the device, the diagonal from the fp64 derivative images.  The fp64 restatement of this iteration ends within
    0.0044 px of the truth; 0.01 px covers fp32 resampling, not a wrong gradient - a wrong sign or scale diverges."""
    from hrnet_hip import registration
    ref, ref_mask, views, view_masks = R.scene(H, W, TRUE, seed)
    d_ref, d_rm, d_views, d_vm = _cuda(ref[None], ref_mask[None], views[None], view_masks[None])
    s = np.array(TRUE, np.float64) + np.array([0.3, -0.25])
    for step in range(8):
        ds = torch.tensor(s[None], dtype=torch.float32, device="cuda", requires_grad=True)
        warped, valid = registration.warp(d_views, ds, d_vm)
        c = d_rm[:, None] * valid
        (0.5 * (c * (GAIN * warped + OFFSET - d_ref[:, None]) ** 2).sum()).backward()
        grad, cn = ds.grad[0].double().cpu().numpy(), c[0].double().cpu().numpy()
        for v in range(len(TRUE)):
            _, dy, dx = WR.sample_d(views[v], np.float32(s[v]))
            diag = np.array([(cn[v] * (GAIN * dy) ** 2).sum(), (cn[v] * (GAIN * dx) ** 2).sum()])
            s[v] = np.float32(s[v]) - grad[v] / diag
        print(f"{H}x{W} step {step}: shifts {s.tolist()} error {np.abs(s - np.array(TRUE)).max():.5f} px")
    assert np.abs(s - np.array(TRUE)).max() <= 0.01
