"""CPU: the fp64 restatement of the robust, regularised reconstruction (tests/robust_ref.py) is what DESIGN.md section 7u defines - the
bilateral-TV gradient against central differences, its sum, constant planes, frames smaller than the window, the Hessian bound of the
step-size rule, the Welsch step's limits - the Python surface refuses bad arguments, and the quality table's three orderings hold."""
import numpy as np
import pytest
import torch

import observe_ref as O
import robust_ref as RB
import robust_scenes as Q
import shift_add_scene as SS

rng = lambda seed: np.random.Generator(np.random.PCG64(seed))


def _brute(x, P, alpha, eps):
    """R and g by loops over ordered pairs (p, q = p - d): the definition word by word, weights unrounded"""
    H, W = x.shape
    R, g = 0.0, np.zeros_like(x)
    for l, m in RB.displacements(P):
        wd = alpha ** (abs(l) + abs(m))
        for y in range(H):
            for xx in range(W):
                qy, qx = y - l, xx - m
                if 0 <= qy < H and 0 <= qx < W:
                    t = x[y, xx] - x[qy, qx]
                    R += wd * (np.sqrt(t * t + eps * eps) - eps)
                    d = t / np.sqrt(t * t + eps * eps)
                    g[y, xx] += wd * d
                    g[qy, qx] -= wd * d
    return R, g


@pytest.mark.parametrize("P", [1, 2, 3])
def test_gradient_is_the_derivative_of_the_value_and_sums_to_zero(P):
    x = rng(P).uniform(0, 1, (7, 9))
    alpha, eps, h = 0.5, 0.25, 1e-5                       # alpha, eps exact in fp32: the rounded weights are the unrounded ones
    g, T = RB.btv_grad(x, P, alpha, eps)
    num = np.zeros_like(x)
    for i in range(x.size):
        d = np.zeros(x.size)
        d[i] = h
        d = d.reshape(x.shape)
        num.flat[i] = (RB.btv_value(x + d, P, alpha, eps)[0] - RB.btv_value(x - d, P, alpha, eps)[0]) / (2 * h)
    assert np.abs(g - num).max() <= 1e-8 * max(1.0, np.abs(g).max())
    assert abs(g.sum()) <= 1e-12 * np.abs(g).sum()
    R, gb = _brute(x, P, alpha, eps)
    assert np.isclose(RB.btv_value(x, P, alpha, eps)[0], R, rtol=1e-13) and np.allclose(g, gb, rtol=1e-12, atol=1e-14)
    assert (T > 0).all()


@pytest.mark.parametrize("P", [1, 2, 3])
def test_constant_planes_and_frames_smaller_than_the_window(P):
    c = np.full((6, 5), 0.37)
    assert RB.btv_value(c, P, 0.7, 0.02)[0] == 0 and not RB.btv_grad(c, P, 0.7, 0.02)[0].any()
    for shape in [(1, 1), (1, 7), (2, 2), (5, 3)]:
        x = rng(11).uniform(0, 1, shape)
        R, g = _brute(x, P, 0.5, 0.25)
        assert np.isclose(RB.btv_value(x, P, 0.5, 0.25)[0], R, rtol=1e-13, atol=0) and np.allclose(RB.btv_grad(x, P, 0.5, 0.25)[0], g, rtol=1e-12, atol=1e-14)
    one = RB.btv_grad(np.array([[0.4]]), P, 0.7, 0.02)
    assert one[0][0, 0] == 0 and one[1][0, 0] == 0 and RB.btv_value(np.array([[0.4]]), P, 0.7, 0.02) == (0, 0)
    # equal neighbours: the plane is two constant halves, g is exactly 0 away from the seam
    x = np.zeros((8, 12))
    x[:, 6:] = 1.0
    g = RB.btv_grad(x, P, 0.7, 0.02)[0]
    assert not g[:, :6 - P].any() and not g[:, 6 + P:].any() and g[:, 5].all()


@pytest.mark.parametrize("P", [1, 2, 3])
def test_hessian_of_the_prior_is_below_the_step_size_rules_bound(P):
    """power iteration on the Hessian of R (a central difference of g) at random planes, smooth ones included (the Hessian is largest
    where differences are small against eps): its largest eigenvalue is at most 4 W / eps"""
    alpha, eps = 0.7, 0.02
    bound = 4.0 * RB.weight_sum(P, alpha) / eps
    worst = 0.0
    for seed, amp in ((0, 1.0), (1, 1e-3), (2, 0.0)):
        r = rng(seed)
        x = 0.5 + amp * r.uniform(-0.5, 0.5, (12, 13))
        v = r.standard_normal(x.shape)
        lam = 0.0
        for _ in range(80):
            v /= np.sqrt((v * v).sum())
            h = 1e-7
            Hv = (RB.btv_grad(x + h * v, P, alpha, eps)[0] - RB.btv_grad(x - h * v, P, alpha, eps)[0]) / (2 * h)
            lam = float((v * Hv).sum())
            v = Hv
        worst = max(worst, lam)
        assert lam <= bound * (1 + 1e-6), (seed, lam, bound)
    print(f"P={P}: largest eigenvalue found {worst:.1f}, bound 4 W / eps = {bound:.1f}")
    assert worst >= 0.4 * bound                          # the bound is not idle: the constant plane reaches 69 / 56 / 53 % of it


def test_weight_sum_and_step_rule_numbers():
    assert abs(RB.weight_sum(2, 0.7) - 10.42) < 0.005
    assert abs(RB.step_bound(1.0, 4e-4, 2, 0.7, 0.02) - 1.85) < 0.005


def _small(noise=0.01, seed=3):
    sc = SS.make(n_lr=16, scale=3, views=4, band=0.25, limit=1.0, noise=noise, clouds=1, margin=2.0, seed=seed)
    x0 = rng(5).uniform(0.2, 0.8, (1, 48, 48))
    return sc, x0


def test_options_off_are_back_projection_and_a_huge_delta_is_the_plain_step():
    sc, x0 = _small()
    a, trace, _ = RB.reconstruct(x0, sc["lrs"], sc["masks"], None, sc["shifts"], 3, 4, robust=False, lam=0.0)
    b, losses = O.back_project(x0, sc["lrs"], sc["masks"], None, sc["shifts"], 3, 4)
    assert np.array_equal(a, b) and np.array_equal(trace[:, :, 0], losses) and np.array_equal(trace[:, :, 1], losses) and not trace[:, :, 2].any()
    zero, t0, _ = RB.reconstruct(x0, sc["lrs"], sc["masks"], None, sc["shifts"], 3, 0)
    assert np.array_equal(zero, x0) and t0.shape == (0, 1, 3)
    for brightness in (True, False):
        plain, _, _ = RB.data_step(x0, sc["lrs"], sc["masks"], None, sc["shifts"], 3, 1.0, brightness)
        soft, _, info = RB.data_step(x0, sc["lrs"], sc["masks"], None, sc["shifts"], 3, 1.0, brightness, robust=True, delta=1e6)
        assert np.abs(soft - plain).max() <= 1e-9 and np.abs(info["rt"]["inlier"] - 1.0).max() <= 1e-9
        assert np.abs(info["rt"]["loss"] - info["s"]["L"]).max() <= 1e-9


def test_a_view_of_outliers_contributes_exactly_nothing():
    sc, x0 = _small()
    lrs = sc["lrs"].copy()
    lrs[0, 2] += 100.0                                   # without the brightness bias: e = -100, (e / delta)^2 = 1e6, exp underflows to 0
    x1, _, info = RB.data_step(x0, lrs, sc["masks"], None, sc["shifts"], 3, 1.0, False, robust=True, delta=0.1)
    rt, s = info["rt"], info["s"]
    assert s["n"][0, 2] > 0 and rt["sw"][0, 2] == 0 and rt["beta"][0, 2] == 0 and rt["inlier"][0, 2] == 0 and not rt["r"][0, 2].any()
    rest = O.adjoint(np.where(np.arange(4)[None, :, None, None] == 2, 0.0, rt["r"]), sc["shifts"], 3)[0]
    assert np.array_equal(x0 - (9.0 / 4.0) * rest, x1)   # V_b still counts the view: it has counted pixels


def test_python_surface_checks_its_arguments():
    from hrnet_hip import binding, observation
    lrs, shifts, sr0 = torch.zeros(2, 3, 8, 8), torch.zeros(2, 3, 2), torch.zeros(2, 24, 24)
    bad = [(ValueError, dict(robust="huber")), (ValueError, dict(robust=True)), (ValueError, dict(delta=0.0)), (ValueError, dict(delta=-1.0)),
           (ValueError, dict(delta=float("nan"))), (ValueError, dict(delta=float("inf"))), (TypeError, dict(delta="small")),
           (ValueError, dict(lam=-1e-4)), (ValueError, dict(lam=float("nan"))), (TypeError, dict(lam=None)), (ValueError, dict(P=0)),
           (ValueError, dict(P=4)), (ValueError, dict(P=2.0)), (ValueError, dict(P=True)), (ValueError, dict(alpha=0.0)), (ValueError, dict(alpha=1.5)),
           (ValueError, dict(alpha=float("nan"))), (ValueError, dict(eps=0.0)), (ValueError, dict(eps=-0.02)), (ValueError, dict(eps=float("inf"))),
           (ValueError, dict(step=2.0)), (ValueError, dict(iters=-1)), (TypeError, dict(brightness=1)), (TypeError, dict(return_trace=1)),
           (ValueError, dict(lam=0.01)),                                    # the prototype's divergence: step (1.02 + 4 lam W / eps) = 21.9
           (ValueError, dict(sr0=torch.zeros(2, 25, 24))), (ValueError, dict(scale=2)), (TypeError, dict(lrs=lrs.numpy())),
           (TypeError, dict())]                                            # everything right, but on the CPU: no fallback
    for exc, kw in bad:
        args = dict(sr0=sr0, lrs=lrs, shifts=shifts)
        args.update(kw)
        with pytest.raises(exc):
            observation.reconstruct(**args)
    # the step-size rule at 1.99 passes (and the call then stops at the CPU tensors), at 2.01 raises with the numbers
    W = RB.weight_sum(2, 0.7)
    assert abs(binding.btv_weight_sum(2, 0.7) - W) < 1e-12
    lam_at = lambda bound, step: (bound / step - RB.DATA_EIGENVALUE) * 0.02 / (4.0 * W)
    for step in (1.0, 0.5, 1.5):
        assert abs(binding.step_bound(step, lam_at(1.99, step), 2, 0.7, 0.02) - 1.99) < 1e-9
        observation.check_reconstruct(step, "welsch", 0.1, lam_at(1.99, step), 2, 0.7, 0.02)
        with pytest.raises(TypeError, match="ROCm device only"):
            observation.reconstruct(sr0, lrs, shifts, step=step, lam=lam_at(1.99, step))
        with pytest.raises(ValueError, match=r"below 2.*2\.01"):
            observation.reconstruct(sr0, lrs, shifts, step=step, lam=lam_at(2.01, step))
    observation.check_reconstruct(1.9, None, 0.1, 0.0, 2, 0.7, 0.02)           # without the prior the rule is check_step's alone
    for exc, kw in [(TypeError, dict(srs=None)), (ValueError, dict(srs=torch.zeros(24, 24))), (ValueError, dict(srs=torch.zeros(2, 2, 24, 24))),
                    (TypeError, dict(srs=sr0.long())), (ValueError, dict(P=0)), (ValueError, dict(alpha=2.0)), (ValueError, dict(eps=0.0)),
                    (TypeError, dict())]:
        args = dict(srs=sr0)
        args.update(kw)
        with pytest.raises(exc):
            observation.btv_loss(**args)
    frames = torch.zeros(1, 2, 16, 16)
    with pytest.raises(ValueError, match="robust"):
        observation.register_and_refine(frames, robust="tukey")
    with pytest.raises(ValueError, match="below 2"):
        observation.register_and_refine(frames, lam=0.01)
    with pytest.raises(TypeError):                                          # the search refuses CPU tensors
        observation.register_and_refine(frames, robust="welsch", lam=4e-4)


def test_baseline_table_takes_the_robust_method():
    from hrnet_hip import validate
    x = torch.zeros(2, 3, 16, 16)
    batch = (x, torch.ones(2, 3), torch.zeros(2, 48, 48), torch.ones(2, 48, 48), ["a", "b"], torch.ones_like(x))
    with pytest.raises(ValueError, match="robust"):
        validate.baseline_table([batch], method="lanczos")
    with pytest.raises(ValueError, match="delta"):
        validate.baseline_table([batch], method="robust", delta=0.0)
    with pytest.raises(TypeError, match="ROCm device only"):
        validate.baseline_table([batch], method="robust", iters=3)


def test_quality_table_orderings():
    """the restatement on the three scenes (DESIGN.md section 7u holds the table); the prototype's margins were 6.0 / 3.0 / 7.5 dB"""
    for sc in Q.SCENES:
        cells = [f"{m} {Q.restated(*sc, m, 10)[1]:.2f} / {Q.restated(*sc, m, 30)[1]:.2f}" for m in Q.METHODS]
        print(f"noise {sc[0]}, {sc[1]} unmasked: start {Q.psnr(Q.scene(*sc)['start'], Q.scene(*sc)):.2f} dB | " + " | ".join(cells))
    for sc, method, iters, margin in Q.ORDERINGS:
        got, plain = Q.restated(*sc, method, iters)[1], Q.restated(*sc, "plain", iters)[1]
        print(f"{sc} {method} at {iters}: {got:.2f} dB against plain {plain:.2f} dB")
        assert got >= plain + margin
