"""GPU: hrn_subpixel_loss_train / hrn_subpixel_loss_backward and hrnet_hip.losses.subpixel_loss against the fp64
restatement tests/subpixel_ref.py, on the scenes of tests/test_subpixel_loss_host.py: B = 1 (24, 40) - one partial tile; B = 2 (70, 83) -
seams at 64, the last tile 6 rows by 19 columns; B = 1 (130, 203) - seams at 64 and 128, the last tile 2 by 11; each with the five true
shifts and both metrics, P = 7, 4 levels, radius 3, border 3.  The second sample of B = 2 is the scene of seed + 10 at the next shift.

Bounds.  The device forms t = S(sr - mean, s) in fp32; against fp64 a pixel is off by at most delta_p = C T_p, T_p = sum |k| |sr| over its
footprint, C = kernel_bounds.C = 1e-5.  Through the square that is |cMSE_device - cMSE_fp64| <= 2 mean(|e| delta) + mean(delta^2)
(subpixel_ref.cmse_bound, which adds the fp64 rounding of the six sums); through -10 log10 it is kernel_bounds.cpsnr_bound's form; the bias
is off by at most mean(delta).  The ABI returns a level's best point, not its P^2 values, so a level is checked as follows: wherever the
restatement's two lowest values of the level are further apart than twice the larger of their bounds the device must have taken the
restatement's point, and its cMSE there must be within the bound; where they are closer the device may take either, the sample's later
levels are then compared at the device's own points, and at most one of the 15 cases may do so.  d_srs is held per element to
|got - want| <= C T with subpixel_ref.grad_magnitude's T; the buffer is prefilled with a sentinel between guards, every element must be
written and the elements no counted pixel's footprint reaches must be exactly 0.

Controls: the restatement with one part of the definition left out (subpixel_ref.CONTROLS) must be REJECTED by the same comparisons on
most of the 15 cases.

The "C needed" of every comparison is printed; the largest are recorded in DESIGN.md section 7q."""
import ctypes

import numpy as np
import pytest
import torch

import kernel_bounds as KB
import shift_loss_ref
import subpixel_ref as SP

pytestmark = pytest.mark.gpu

C = KB.C
SENTINEL = float(np.frombuffer(np.uint32(0x7F7F7F7F).tobytes(), np.float32)[0])
GUARD = 1024
METRICS = {"cMSE": 1, "cPSNR": 2}
BATCH = {(24, 40): 1, (70, 83): 2, (130, 203): 1}
CASES = [(si, ki) for si in range(len(SP.SHAPES)) for ki in range(len(SP.SHIFTS))]
IDS = [f"{SP.SHAPES[si][0][0]}x{SP.SHAPES[si][0][1]}-{SP.SHIFTS[ki][0]:g},{SP.SHIFTS[ki][1]:g}" for si, ki in CASES]
D_OUT = {1: [0.7], 2: [0.7, -1.3]}
_scenes, _refs, _runs = {}, {}, {}


def scenes(si, ki):
    """the B samples of a case: [(sr, hr, hr_map)], numpy float32"""
    if (si, ki) not in _scenes:
        shape, seed = SP.SHAPES[si]
        _scenes[si, ki] = [SP.scene(*shape, SP.SHIFTS[(ki + b) % len(SP.SHIFTS)], seed + 10 * b) for b in range(BATCH[shape])]
    return _scenes[si, ki]


def reference(si, ki):
    """the restatement's search of every sample of a case, once"""
    if (si, ki) not in _refs:
        _refs[si, ki] = [SP.search(*x) for x in scenes(si, ki)]
    return _refs[si, ki]


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def batch(xs):
    return tuple(dev(np.stack([x[i] for x in xs])) for i in range(3))


def forward(si, ki, metric):
    """the device forward of a case, once: -> (out, stats, trace) as numpy"""
    from hrnet_hip import binding
    if (si, ki, metric) not in _runs:
        got = binding.subpixel_loss_train(*batch(scenes(si, ki)), metric, SP.BORDER, SP.P, SP.LEVELS, SP.RADIUS)
        _runs[si, ki, metric] = tuple(t.cpu().numpy() for t in got)
    return _runs[si, ki, metric]


def raw_backward(srs, hrs, maps, stats, d_out, metric, border=SP.BORDER):
    """hrn_subpixel_loss_backward into a sentinel-prefilled buffer between guards -> d_srs (B,H,W) numpy; the guards must be untouched"""
    from hrnet_hip import binding
    lib = binding.load_library()
    B, H, W = srs.shape
    buf = torch.full((B * H * W + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=srs.device)
    d_srs = buf[GUARD:GUARD + B * H * W]
    ws = torch.empty(lib.hrn_subpixel_loss_workspace_bytes(B, H, W, 3), dtype=torch.uint8, device=srs.device)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = lib.hrn_subpixel_loss_backward(p(srs), p(hrs), p(maps), p(stats), p(d_out), B, H, W, border, METRICS[metric], p(d_srs), p(ws),
                                        ws.numel(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.hrn_last_error()
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert (out[:GUARD] == SENTINEL).all() and (out[-GUARD:] == SENTINEL).all(), "a guard was written"
    return out[GUARD:-GUARD].reshape(B, H, W)


def needed(err, T):
    """the smallest C that passes |err| <= C T"""
    ok = T > 0
    return float((np.abs(err)[ok] / T[ok]).max()) if ok.any() else 0.0


def check_levels(x, ref, trace):
    """one sample's levels against the restatement -> (s* agrees with the restatement's, whether every level fell under the rule, the
    largest C needed).  Asserts the bound wherever the rule applies."""
    follows, under_rule, worst = True, True, 0.0
    for k in range(SP.LEVELS):
        point = (np.float32(trace[k, 0]), np.float32(trace[k, 1]))
        if follows:
            s, dys, dxs = ref["scores"][k], ref["coords"][k, 0], ref["coords"][k, 1]
            order = np.argsort(s, axis=None, kind="stable")[:2]
            (i0, j0), (i1, j1) = (np.unravel_index(o, s.shape) for o in order)
            b0, b1 = SP.cmse_bound(*x, SP.BORDER, (dys[i0], dxs[j0]), C), SP.cmse_bound(*x, SP.BORDER, (dys[i1], dxs[j1]), C)
            decided = s[i1, j1] - s[i0, j0] > 2.0 * max(b0, b1)
            same = point == (dys[i0], dxs[j0])
            if decided:
                assert same, f"level {k}: the device took {point}, the restatement {(dys[i0], dxs[j0])} with a gap of {s[i1, j1] - s[i0, j0]:.3e}"
            else:
                under_rule = False
            follows = same
        want, n, _ = SP.cmse(*x, SP.BORDER, point)
        bound = SP.cmse_bound(*x, SP.BORDER, point, C)
        err = abs(float(trace[k, 2]) - want) - 6e-8 * want                    # trace is fp32
        worst = max(worst, max(err, 0.0) / (bound / C))
        assert err <= bound, f"level {k} at {point}: cMSE {trace[k, 2]:.9g}, want {want:.9g}, bound {bound:.3g}"
    return follows, under_rule, worst


def check_result(x, at, metric, out, st, control={}):
    """out and stats of one sample at the device's point `at` against the restatement (under `control`) -> None, or what failed"""
    want, n, b = SP.cmse(*x, SP.BORDER, at, **{k: v for k, v in control.items() if k in ("no_bias", "no_crop", "no_footprint")})
    if st[0] != n:
        return f"n* {st[0]} != {n}"
    bound = SP.cmse_bound(*x, SP.BORDER, at, C)
    if abs(st[2] - want) > bound:
        return f"cMSE* {st[2]:.9g}, want {want:.9g}, bound {bound:.3g}"
    if abs(st[1] - b) > C * SP.magnitude(x[0], at)[SP.residual(*x, SP.BORDER, at)[0]].mean():
        return f"b* {st[1]:.9g}, want {b:.9g}"
    if metric == "cPSNR":
        value = SP.loss_of(want, "cPSNR")
        tol = float(KB.cpsnr_bound(torch.tensor(want), torch.tensor(bound))) + 6e-8 * abs(value)
    else:
        value, tol = want, bound + 6e-8 * want
    if abs(float(out) - value) > tol:
        return f"out {float(out):.9g}, want {value:.9g}, bound {tol:.3g}"
    return None


def check_grad(x, at, metric, d_out, got, control={}):
    """d_srs of one sample against the restatement's gradient (under `control`) -> (None or what failed, the C needed)"""
    want = SP.grad(*x, SP.BORDER, at, metric, d_out, **control)
    T = SP.grad_magnitude(*x, SP.BORDER, at, metric, d_out, C)
    if not np.isfinite(got).all() or (got == SENTINEL).any():
        return "an element was not written", np.inf
    err = np.abs(got.astype(np.float64) - want)
    if (err > C * T).any():
        i = np.unravel_index(np.argmax(err - C * T), err.shape)
        return f"d_srs{i}: got {got[i]:.9g}, want {want[i]:.9g}, bound {C * T[i]:.3g}", needed(err, T)
    if not (got[T == 0] == 0).all():
        return "a structural zero is not exact", needed(err, T)
    return None, needed(err, T)


@pytest.mark.parametrize("metric", ["cPSNR", "cMSE"])
@pytest.mark.parametrize("si,ki", CASES, ids=IDS)
def test_forward_and_backward_against_fp64(si, ki, metric):
    xs, refs = scenes(si, ki), reference(si, ki)
    out, stats, trace = forward(si, ki, metric)
    srs, hrs, maps = batch(xs)
    d_out = D_OUT[len(xs)]
    d_srs = raw_backward(srs, hrs, maps, dev(stats), dev(np.array(d_out, np.float32)), metric)
    for b, (x, ref) in enumerate(zip(xs, refs)):
        follows, _, worst = check_levels(x, ref, trace[b])
        at = (np.float32(stats[b, 3]), np.float32(stats[b, 4]))
        assert at == (trace[b, -1, 0], trace[b, -1, 1])
        if follows:
            assert at == tuple(ref["shift"]) and stats[b, 0] == ref["n"]
        failed = check_result(x, at, metric, out[b], stats[b])
        assert failed is None, f"sample {b}: {failed}"
        m0 = SP.crop_mask(x[2], SP.BORDER)
        for got, want in ((stats[b, 5], x[0].astype(np.float64).mean()), (stats[b, 6], x[1].astype(np.float64)[m0].mean())):
            assert got == np.float32(got) and abs(got - want) <= 1.2e-7 * abs(want)
        centred = stats[b, 7] + (stats[b, 6] - stats[b, 5])
        assert abs(centred - stats[b, 1]) <= 1e-15
        failed, c_grad = check_grad(x, at, metric, d_out[b], d_srs[b])
        print(f"sample {b}: s* {at}, n* {int(stats[b, 0])}, cMSE* {stats[b, 2]:.4e}; C needed: levels {worst:.2e}, d_srs {c_grad:.2e}")
        assert failed is None, f"sample {b}: {failed}"


def test_at_most_one_case_leaves_the_rule():
    """The 15 cases are the issue's scenes, sample 0 of every batch.  Measured: one, 130x203 at (2.9, -2.9), whose last level has a gap
    of 3.13e-8 against twice a bound of 1.60e-8.  The second samples of the B = 2 batches are further scenes under the same checks; one
    of them (seed 12 at (0.37, -0.62): 2.20e-8 against twice 2.36e-8) is outside the rule too and is listed, not counted."""
    left, extra = [], []
    for (si, ki), name in zip(CASES, IDS):
        _, _, trace = forward(si, ki, "cPSNR")
        for b, (x, ref) in enumerate(zip(scenes(si, ki), reference(si, ki))):
            if not check_levels(x, ref, trace[b])[1]:
                (extra if b else left).append(f"{name}[{b}]")
    print("outside the rule:", left, "and of the second samples:", extra)
    assert len(left) <= 1


@pytest.mark.parametrize("control", SP.CONTROLS)
def test_controls_are_rejected(control):
    metric, rejected = "cPSNR", 0
    for si, ki in CASES:
        xs = scenes(si, ki)
        out, stats, _ = forward(si, ki, metric)
        srs, hrs, maps = batch(xs)
        d_out = D_OUT[len(xs)]
        d_srs = raw_backward(srs, hrs, maps, dev(stats), dev(np.array(d_out, np.float32)), metric)
        at = (np.float32(stats[0, 3]), np.float32(stats[0, 4]))
        kw = {control: True}
        rejected += check_result(xs[0], at, metric, out[0], stats[0], kw) is not None or check_grad(xs[0], at, metric, d_out[0], d_srs[0], kw)[0] is not None
    print(f"{control}: rejected on {rejected} of {len(CASES)} cases")
    assert rejected > len(CASES) // 2


def test_samples_without_a_counted_pixel():
    """a fully masked sample, and one whose clear pixels all lie inside the border frame: NaN and a zero gradient, the others untouched"""
    from hrnet_hip import binding
    (sr, hr, m), = scenes(1, 0)[:1]
    masked, framed = np.zeros_like(m), np.zeros_like(m)
    framed[:SP.BORDER], framed[:, -SP.BORDER:] = 1.0, 1.0
    srs, hrs, maps = dev(np.stack([sr, sr, sr])), dev(np.stack([hr, hr, hr])), dev(np.stack([masked, m, framed]))
    for metric in METRICS:
        out, stats, trace = binding.subpixel_loss_train(srs, hrs, maps, metric, SP.BORDER, SP.P, SP.LEVELS, SP.RADIUS)
        alone = forward(1, 0, metric)
        assert torch.isnan(out[[0, 2]]).all() and out[1].cpu().numpy().tobytes() == alone[0][0].tobytes()
        assert stats[1].cpu().numpy().tobytes() == alone[1][0].tobytes()
        st = stats.cpu().numpy()
        for b in (0, 2):
            assert st[b, 0] == 0 and st[b, 1] == 0 and np.isnan(st[b, 2]) and (st[b, 3:5] == 0).all() and st[b, 7] == 0
            assert np.isnan(trace[b, :, 2].cpu().numpy()).all()
        d = raw_backward(srs, hrs, maps, stats, dev(np.array([1.0, 1.0, 1.0], np.float32)), metric)
        assert (d[0] == 0).all() and (d[2] == 0).all() and np.abs(d[1]).max() > 0


def test_bits_do_not_depend_on_the_run_the_batch_or_the_grad_mode():
    from hrnet_hip import binding, losses
    xs = scenes(1, 2)
    srs, hrs, maps = batch(xs)
    first = binding.subpixel_loss_train(srs, hrs, maps, "cPSNR", SP.BORDER, SP.P, SP.LEVELS, SP.RADIUS)
    again = binding.subpixel_loss_train(srs, hrs, maps, "cPSNR", SP.BORDER, SP.P, SP.LEVELS, SP.RADIUS)
    d_out = dev(np.array(D_OUT[2], np.float32))
    g1, g2 = (raw_backward(srs, hrs, maps, first[1], d_out, "cPSNR") for _ in range(2))
    for a, b in zip(first, again):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    assert g1.tobytes() == g2.tobytes()
    for b in range(2):                                   # a sample alone gives the bits it had inside the batch
        alone = binding.subpixel_loss_train(srs[b:b + 1], hrs[b:b + 1], maps[b:b + 1], "cPSNR", SP.BORDER, SP.P, SP.LEVELS, SP.RADIUS)
        for a, w in zip(alone, first):
            assert a[0].cpu().numpy().tobytes() == w[b].cpu().numpy().tobytes()
        g = raw_backward(srs[b:b + 1].contiguous(), hrs[b:b + 1].contiguous(), maps[b:b + 1].contiguous(), alone[1], d_out[b:b + 1].contiguous(), "cPSNR")
        assert g[0].tobytes() == g1[b].tobytes()
    with torch.no_grad():                                # the wrapper: no-grad and grad forwards, the same bits
        plain, shift, tr = losses.subpixel_loss(srs[:, None], hrs, maps, return_shift=True, return_trace=True)
    x = srs.clone().requires_grad_(True)
    tracked = losses.subpixel_loss(x, hrs, maps)
    assert tracked.requires_grad and not plain.requires_grad
    assert plain.cpu().numpy().tobytes() == tracked.detach().cpu().numpy().tobytes() == first[0].cpu().numpy().tobytes()
    assert shift.dtype == torch.float32 and torch.equal(shift.double(), first[1][:, 3:5]) and torch.equal(tr, first[2])
    (tracked * d_out).sum().backward()
    assert x.grad.cpu().numpy().tobytes() == g1.tobytes()
    assert losses.subpixel_loss(x, hrs.clone().requires_grad_(True), maps).grad_fn is not None


def test_shift_is_the_negative_of_shift_loss_offsets():
    from hrnet_hip import binding, losses
    srs, hrs, maps = batch(scenes(1, 1))                 # sample 0: the true shift (2, 0)
    _, s = losses.subpixel_loss(srs, hrs, maps, return_shift=True)
    _, stats = binding.shift_loss_train(srs, hrs, maps, "cPSNR", SP.BORDER, False)
    offsets = shift_loss_ref.offsets(stats[:, 3].long(), SP.BORDER)
    assert offsets[0].tolist() == [-2, 0] and torch.round(s[0]).long().tolist() == [2, 0]     # sample 1 is 0.45 px from a tie of offsets


def test_opcheck():
    ops = torch.ops.hrnet_hip
    srs, hrs, maps = batch(scenes(0, 0))
    checks = ("test_schema", "test_faketensor", "test_autograd_registration")
    args = (srs, hrs, maps, "cPSNR", SP.BORDER, SP.P, SP.LEVELS, SP.RADIUS)
    for first in (srs, srs.clone().requires_grad_(True)):
        torch.library.opcheck(ops.subpixel_loss_train.default, (first,) + args[1:], test_utils=checks)
    out, stats, _ = ops.subpixel_loss_train(*args)
    torch.library.opcheck(ops.subpixel_loss_backward.default, (srs, hrs, maps, stats, torch.ones_like(out), "cPSNR", SP.BORDER), test_utils=checks)


def test_six_adam_steps_lower_the_loss():
    """a free (1, 70, 83) image, started 0.4 px off its target, trained on the loss alone"""
    from hrnet_hip import losses
    sr, hr, m = SP.scene(70, 83, (0.4, -0.4), 5)
    x = dev(sr[None]).requires_grad_(True)
    hrs, maps = dev(hr[None]), dev(m[None])
    opt = torch.optim.Adam([x], lr=1e-4)
    values = []
    for _ in range(6):
        opt.zero_grad()
        loss = -losses.subpixel_loss(x, hrs, maps).mean()
        loss.backward()
        opt.step()
        values.append(float(loss.detach()))
    with torch.no_grad():
        values.append(float(-losses.subpixel_loss(x, hrs, maps).mean()))
    print("loss per step:", values)
    assert all(b < a for a, b in zip(values, values[1:]))
