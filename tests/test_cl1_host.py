"""CPU: the restatement of the shift-searched L1 / Charbonnier loss (tests/cl1_ref.py) against itself - the closed
form of the gradient against autograd, the invariances of the definition - and the conditions on the input sets that
tests/test_gpu_cl1_loss.py relies on, asserted here so that the GPU file need exclude no sample; the Python surface's argument checks
and the two tools' command lines."""
import os
import sys

import numpy as np
import pytest
import torch

import cl1_cases as C
import cl1_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D_OUT = torch.tensor([1.0, -0.5, 2.0], dtype=torch.float64)


def _autograd(x, border, clip, eps):
    s = x[0].double().requires_grad_(True)
    out, k, cl, stats = R.cl1_loss(s, x[1], x[2], border, clip, eps)
    (out * D_OUT).sum().backward()
    return out.detach(), k, cl, stats, s.grad


@pytest.mark.parametrize("eps", [0.0, 1e-3])
@pytest.mark.parametrize("kind", ["rand", "clip", "plant", "weight"])
def test_closed_form_is_autograd(kind, eps):
    for shape, border in (((20, 20), 0), ((37, 53), 3), ((53, 37), 1)):
        x, clip = C.case(kind, shape, border)
        _, k, _, _, want = _autograd(x, border, clip, eps)
        got = R.closed_form_grad(*x, k, D_OUT, border, clip, eps)
        e = float((got - want).abs().max() / want.abs().max())
        print(f"{kind} {shape} border {border} eps {eps}: closed form vs autograd {e:.1e} of the max-norm")
        assert e <= 1e-12
        if border:
            frame = torch.ones_like(want, dtype=torch.bool)
            frame[:, border:-border, border:-border] = False
            assert (want[frame] == 0).all()
        if clip:
            assert (want[(x[0] < 0) | (x[0] > 1)] == 0).all()


def test_stats_are_those_of_the_selected_offset():
    x, _ = C.case("rand", (37, 53), 3)
    for eps in C.EPS:
        out, k, cl, stats = R.cl1_loss(*x, 3, False, eps)
        _, ns, bs, sg = R.all_cl1(*x, 3, False, eps)
        for b in range(C.B):
            assert stats[b].tolist() == [float(ns[b, k[b]]), float(bs[b, k[b]]), float(cl[b, k[b]]), float(k[b]), float(sg[b, k[b]])]
            assert float(out[b]) == float(cl[b].min())


@pytest.mark.parametrize("eps", [0.0, 1e-3])
def test_a_constant_added_to_srs_changes_neither_value_nor_offset(eps):
    """the brightness bias absorbs it (no clip: a clamp does not commute with the shift)"""
    x, _ = C.case("rand", (37, 53), 3)
    out, k, _, _ = R.cl1_loss(*x, 3, False, eps)
    out2, k2, _, _ = R.cl1_loss(x[0].double() + 0.37, x[1], x[2], 3, False, eps)
    assert torch.equal(k, k2) and float(((out2 - out).abs() / out).max()) <= 1e-12


def test_charbonnier_tends_to_l1():
    """|e| <= sqrt(e^2 + eps^2) <= |e| + eps per pixel, so per offset, so for the minimum over the offsets"""
    x, _ = C.case("rand", (37, 53), 3)
    l1 = R.cl1_loss(*x, 3, False, 0.0)[0]
    last = None
    for eps in (1e-2, 1e-4, 1e-6):
        d = R.cl1_loss(*x, 3, False, eps)[0] - l1
        assert (d > 0).all() and (d <= eps).all() and (last is None or (d < last).all())
        last = d


@pytest.mark.parametrize("eps", [0.0, 1e-3])
def test_planted_offset_is_selected(eps):
    for shape in C.SHAPES:
        for border in C.BORDERS:
            x, plant = C.planted(*shape, border, 51 + border)
            nb = 2 * border + 1
            assert R.cl1_loss(*x, border, False, eps)[1].tolist() == [u * nb + v for u, v in plant]


def test_no_clear_pixel_is_nan_and_a_nan_is_never_selected_over_a_number():
    s, h, m = C.random(20, 20, 5)
    m[1] = 0
    out, k, _, stats = R.cl1_loss(s, h, m, 1)
    assert torch.isnan(out[1]) and k[1] == -1 and stats[1, [0, 1, 4]].tolist() == [0.0, 0.0, 0.0] and torch.isfinite(out[[0, 2]]).all()
    cl = torch.tensor([[float("nan"), 2.0, 1.0, 1.0], [float("nan"), float("nan"), 3.0, 3.0]], dtype=torch.float64)
    ns = torch.tensor([[1.0, 1.0, 1.0, 1.0], [1.0, 0.0, 0.0, 1.0]], dtype=torch.float64)
    assert R.select(cl, ns).tolist() == [2, 3]


# ----------------------------------------------------------------------------- what the GPU file relies on
@pytest.mark.parametrize("kind,shape,border", C.CASES, ids=[f"{k}-{s[0]}x{s[1]}-b{b}" for k, s, b in C.CASES])
def test_input_conditions_of_the_gpu_tests(kind, shape, border):
    """Every input set the GPU file compares: the two lowest cL1 differ by more than 1e-6 relative (the device's 1e-5-accurate values
    still select the restatement's offset only if its fp64 sums do; they are far more accurate than the gap), and at eps = 0 no
    weighted pixel's |e| at k* is below 1e-9 (the device forms e in fp64 from an fp64 bias that differs from the restatement's by
    rounding, ~1e-16: every sign agrees)."""
    x, clip = C.case(kind, shape, border)
    for eps in C.EPS:
        _, k, cl, _ = R.cl1_loss(*x, border, clip, eps)
        gap = float(R.top_two_gap(cl).min())
        print(f"{kind} {shape} border {border} eps {eps}: top-two gap {gap:.2e}")
        assert (k >= 0).all() and gap > 1e-6
        if eps == 0:
            least = R.min_abs_e(*x, k, border, clip)
            print(f"{kind} {shape} border {border}: min |e| {least:.2e}")
            assert least > 1e-9


# ----------------------------------------------------------------------------- the Python surface, without a device
def test_ops_are_registered_and_the_wrapper_checks_its_arguments():
    from hrnet_hip import binding, losses
    ops = torch.ops.hrnet_hip
    assert hasattr(ops, "cl1_loss_train") and hasattr(ops, "cl1_loss_backward")
    assert hasattr(binding, "cl1_loss_train") and hasattr(binding, "cl1_loss_backward")
    s, h, m = C.random(20, 20, 1)
    with pytest.raises(TypeError, match="ROCm device"):
        losses.cl1_loss(s, h, m)
    with pytest.raises(TypeError, match="torch.Tensor"):
        losses.cl1_loss(s.numpy(), h, m)
    with pytest.raises(ValueError, match="equal"):
        losses.cl1_loss(s, h[:, :19], m)
    for border in (-1, 9, 10):
        with pytest.raises(ValueError, match="border_w"):
            losses.cl1_loss(s, h, m, border_w=border)
    for eps in (-1e-3, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="eps"):
            losses.cl1_loss(s, h, m, eps=eps)


def test_fake_kernels_give_the_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from hrnet_hip import binding  # noqa: F401  (registers the ops)
    with FakeTensorMode():
        s = torch.empty((3, 20, 24), device="cuda")
        out, stats = torch.ops.hrnet_hip.cl1_loss_train(s, s, s, 3, False, 0.0)
        assert tuple(out.shape) == (3,) and out.dtype == torch.float32 and tuple(stats.shape) == (3, 5) and stats.dtype == torch.float64
        g = torch.ops.hrnet_hip.cl1_loss_backward(s, s, s, stats, out, 3, False, 0.0)
        assert tuple(g.shape) == (3, 20, 24) and g.dtype == torch.float32


def test_tools_know_the_loss():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import shift_loss_bench
    import train_step_bench
    o = vars(train_step_bench.options("32 32 64 10 --precision bf16 --loss shift,l1 --repeats 3".split()))
    assert o["loss"] == ["shift", "l1"] and o["repeats"] == 3 and "l1" in train_step_bench.SEARCHED
    assert vars(train_step_bench.options("8 4 16 2 --loss l1".split()))["loss"] == ["l1"]        # no ShiftNet: its window does not apply
    assert {"cl1_fwd", "cl1_bwd", "shift_loss_fwd", "shift_loss_bwd", "shift_cpsnr"} <= set(shift_loss_bench.FAMILIES)
    # the composition the bench times is the definition (fp32 against the fp64 restatement)
    x, _ = C.case("clip", (37, 53), 3)
    for eps in C.EPS:
        want = R.cl1_loss(*x, 3, True, eps)[0]
        got = shift_loss_bench.torch_cl1(*x, 3, eps).double()
        assert float(((got - want).abs() / want).max()) <= 1e-5
