"""GPU: cSSIM as a training loss (hrnet_hip.losses.cssim_loss over hrn_shift_cssim / hrn_cssim_loss_backward) against
the fp64 restatement of its gradient in the direct form (tests/cssim_grad_ref.py), which tests/test_cssim_loss_host.py holds to torch
fp64 autograd.

Cases (cssim_grad_ref.CASES, both windows): a frame whose map is one pixel; cssim_cases.scene_batch(2, 24, 24) and (1, 49, 71); the 40
conditioning scenes (level 0.9, 0.5, 0.05 at contrast 0.05 - clear, with a blob, the left third masked - and level 0.9 at contrast
0.005); a crop of one pixel more than one backward tile (16 x 44 crop pixels under the gaussian window, 16 x 52 under the uniform) along
both axes, and of two tiles + 1, so that an interior tile and both remainders exist; borders 0, 3 and 8; the bias off; clip on with
pixels clamped at both ends.  The backward tile's halo of 2 (T - 1) is wider than every frame but the two-tiles ones, so every tile here
has pixels outside the crop on some side.

Bound: cssim_loss_bounds.CSSIM_GRAD_TOL x the sample's max |gradient| - four times the largest error of the float32 CPU model of the
kernel's algebra over these cases, never the kernel's own error; the kernel's measured error is printed per case.  k* must equal the
restatement's, whose best offset leads by >= cssim_cases.PIN_GAP on every case (the CPU test asserts it)."""
import numpy as np
import pytest
import torch

import cssim_grad_ref as G
import util
from cssim_loss_bounds import CSSIM_GRAD_TOL

pytestmark = pytest.mark.gpu

CASE = {c[0]: c for c in G.CASES}
D_OUT = (1.0, -0.75, 0.0, 2.5)                          # per sample, cycled: a 0 and a negative value among them


def _loss_and_grad(x, border, window, d_out, **kw):
    """-> (loss (B,), shift (B,2), d_srs (B,H,W)) as numpy, the cotangent of the loss d_out"""
    from hrnet_hip import losses
    s, h, m = (util.dev(a) for a in x)
    s.requires_grad_(True)
    loss, shift = losses.cssim_loss(s, h, m, border_w=border, window=window, return_shift=True, **kw)
    (loss * util.dev(np.asarray(d_out, np.float32))).sum().backward()
    return loss.detach().cpu().numpy(), shift.cpu().numpy(), s.grad.cpu().numpy()


@pytest.mark.parametrize("case", G.CASES, ids=[c[0] for c in G.CASES])
def test_gradient_matches_the_restatement(case):
    cid, family, _, border, window, opt = case
    x = G.case_input(case)
    B = len(x[0])
    (scores, k, _, _), grads = G.case_ref(case)
    d_out = [D_OUT[(b + (0 if B > 1 else 1)) % len(D_OUT)] for b in range(B)]      # a lone sample takes the negative value
    loss, shift, got = _loss_and_grad(x, border, window, d_out, **opt)
    nb = 2 * border + 1
    for b in range(B):
        assert (shift[b, 0] + border) * nb + shift[b, 1] + border == k[b], (cid, b)
        assert abs(loss[b] - (1.0 - scores[b, k[b]])) <= 2e-6, (cid, b)
        want = -d_out[b] * grads[b]                                 # the loss is 1 - score
        if d_out[b] == 0:
            assert not got[b].any(), (cid, b)
            continue
        err = G.rel_err(got[b], want)
        print(f"cssim gradient {cid}[{b}] ({family}): max |gpu - fp64| = {err:.3e} of the max |gradient| {np.abs(want).max():.3e}")
        assert err <= CSSIM_GRAD_TOL, (cid, b, err)
        inner = got[b][border:got[b].shape[0] - border, border:got[b].shape[1] - border]
        assert np.count_nonzero(got[b]) == np.count_nonzero(inner)   # the border frame is exactly 0
        assert not got[b][want == 0].any()                           # masked (and clamped) pixels too


@pytest.mark.parametrize("window", ["gaussian", "uniform"])
def test_forward_identity(window):
    """with and without grad the loss is 1 - shift_cssim bit for bit, the shifts alike"""
    from hrnet_hip import binding, losses
    x = G.case_input(CASE[f"holes-24x24-{window}"])
    s, h, m = (util.dev(a) for a in x)
    for clip in (False, True):
        score, want_shift = losses.shift_cssim(s, h, m, window=window, clip=clip, return_shift=True)
        want = 1.0 - score
        plain, shift0 = losses.cssim_loss(s, h, m, window=window, clip=clip, return_shift=True)
        sg = s.clone().requires_grad_(True)
        live, shift1 = losses.cssim_loss(sg, h, m, window=window, clip=clip, return_shift=True)
        with torch.no_grad():
            quiet = losses.cssim_loss(sg, h, m, window=window, clip=clip)
        assert live.requires_grad and not plain.requires_grad and not quiet.requires_grad
        assert torch.equal(plain, want) and torch.equal(live.detach(), want) and torch.equal(quiet, want)
        assert torch.equal(shift0, want_shift) and torch.equal(shift1, want_shift) and shift1.dtype == torch.int64
        _, stats, _ = binding.shift_cssim(s, h, m, 3, window, clip)
        _, stats2 = torch.ops.hrnet_hip.shift_cssim_train(s, h, m, 3, window, clip, True, 1.0)
        assert torch.equal(stats, stats2)
    assert torch.equal(losses.cssim_loss(s, h, m), 1.0 - losses.shift_cssim(s, h, m, clip=False))          # clip defaults to False


def test_border_frame_and_clamped_pixels_are_exactly_zero():
    x = G.case_input(CASE["clip-gaussian"])
    _, _, got = _loss_and_grad(x, 3, "gaussian", [1.0, -2.0], clip=True)
    s = x[0]
    clamped = (s < 0) | (s > 1)
    assert clamped[:, 3:-3, 3:-3].any() and not got[clamped].any()
    frame = np.ones(s.shape, bool)
    frame[:, 3:-3, 3:-3] = False
    assert not got[frame].any() and got.any()


def test_a_sample_without_an_offset_gets_nan_and_a_zero_gradient():
    s, h, m = (a.copy() for a in G.case_input(CASE["holes-24x24-gaussian"]))
    x3 = tuple(np.concatenate([a, a[:1], a[:1]]) for a in (s, h, m))
    x3[2][1] = 0.0                                                  # sample 1: all masked; sample 3: a cotangent of 0
    loss, shift, got = _loss_and_grad(x3, 3, "gaussian", [1.0, 1.0, 1.0, 0.0])
    assert np.isnan(loss[1]) and shift[1].tolist() == [-4, 3] and not got[1].any()
    assert loss[3] == loss[0] and not got[3].any()
    lone, _, g0 = _loss_and_grad(tuple(a[:1] for a in x3), 3, "gaussian", [1.0])
    assert loss[0] == lone[0] == loss[2] and np.array_equal(got[0], g0[0]) and np.array_equal(got[2], g0[0])
    assert np.isfinite(got).all() and got[0].any()


def test_two_runs_are_bit_identical_and_a_sample_does_not_see_its_batch():
    case = CASE["two-tiles+1-gaussian-holes"]
    x1 = G.case_input(case)
    x = tuple(np.concatenate([a, b]) for a, b in zip(x1, G.case_input(CASE["two-tiles+1-gaussian-clear"])))
    a = _loss_and_grad(x, 3, "gaussian", [1.0, -0.75])
    b = _loss_and_grad(x, 3, "gaussian", [1.0, -0.75])
    for p, q in zip(a, b):
        assert np.array_equal(p, q)
    alone = _loss_and_grad(x1, 3, "gaussian", [1.0])
    assert alone[0][0] == a[0][0] and np.array_equal(alone[2][0], a[2][0])


def test_targets_get_no_gradient_and_the_wrapper_takes_a_channel_axis_and_strided_input():
    from hrnet_hip import losses
    x = G.case_input(CASE["holes-24x24-uniform"])
    s, h, m = (util.dev(a) for a in x)
    s.requires_grad_(True); h.requires_grad_(True); m.requires_grad_(True)
    losses.cssim_loss(s, h, m, window="uniform").sum().backward()
    assert h.grad is None and m.grad is None and s.grad is not None
    want = s.grad.clone()
    s4 = s.detach()[:, None].clone().requires_grad_(True)
    losses.cssim_loss(s4, h, m, window="uniform").sum().backward()
    assert torch.equal(s4.grad[:, 0], want)
    st = s.detach().transpose(1, 2).contiguous().transpose(1, 2).requires_grad_(True)
    assert not st.is_contiguous()
    losses.cssim_loss(st, h, m, window="uniform").sum().backward()
    assert torch.equal(st.grad, want)


def test_opcheck():
    s, h, m = (util.dev(a) for a in G.case_input(CASE["holes-24x24-gaussian"]))
    s.requires_grad_(True)
    torch.library.opcheck(torch.ops.hrnet_hip.shift_cssim_train.default, (s, h, m, 3, "gaussian", False, True, 1.0),
                          test_utils=("test_schema", "test_faketensor", "test_autograd_registration"))
    _, stats = torch.ops.hrnet_hip.shift_cssim_train(s.detach(), h, m, 3, "gaussian", False, True, 1.0)
    d_out = util.dev(np.array([1.0, -0.5], np.float32))
    torch.library.opcheck(torch.ops.hrnet_hip.cssim_loss_backward.default, (s.detach(), h, m, stats, d_out, 3, "gaussian", False, True, 1.0),
                          test_utils=("test_schema", "test_faketensor"))


def test_one_training_step_reaches_the_parameters():
    """a 4-view 16 x 16 HRNet (x3, 48 x 48 targets): the loss's gradient arrives at every trainable parameter, finite and not all zero"""
    from hrnet_hip import losses
    model = util._fresh_model(precision="fp32")
    rng = np.random.Generator(np.random.PCG64(91))
    lrs, alphas = util.dev(rng.random((2, 4, 16, 16), dtype=np.float32)), util.dev(np.ones((2, 4), np.float32))
    hrs, maps = util.dev(rng.random((2, 48, 48), dtype=np.float32)), util.dev((rng.random((2, 48, 48)) > 0.1).astype(np.float32))
    loss = losses.cssim_loss(model(lrs, alphas), hrs, maps).mean()
    loss.backward()
    assert torch.isfinite(loss)
    grads = [p.grad for p in model.parameters() if p.requires_grad]
    assert grads and all(g is not None and torch.isfinite(g).all() for g in grads) and any(g.abs().max() > 0 for g in grads)
