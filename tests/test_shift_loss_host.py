"""CPU: the restatement of the shift-searched loss (tests/shift_loss_ref.py) against the reference's own numbers
(tests/golden/callers.npz) and the numpy oracle, its symmetry under transposition, and the host side of the new surface: exports,
argument checks of the C entry points (nothing is launched) and of hrnet_hip.losses.shift_loss."""
import ctypes
import os

import numpy as np
import pytest
import torch

import shift_loss_ref as R
import util
from oracle import hrnet_np as O


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def test_restatement_is_the_reference_shift_cpsnr():
    g = util.golden("callers")
    out, k, _ = R.shift_loss(_t(g["srs"]), _t(g["hrs"]), _t(g["maps"]), "cPSNR", 3, clip=True)
    assert util.rel_err(out.numpy(), g["shift_cpsnr"]) <= 1e-9
    assert k.min() >= 0 and k.max() < 49


def test_restatement_without_border_is_the_reference_cpsnr():
    g = util.golden("callers")
    out, k, _ = R.shift_loss(_t(g["srs"]), _t(g["hrs"]), _t(g["maps"]), "cPSNR", 0, clip=True)
    assert util.rel_err(out.numpy(), g["cpsnr"]) <= 1e-9
    assert (k == 0).all()


def _random(B, H, W, seed, lo=-0.2, hi=1.2):
    rng = np.random.Generator(np.random.PCG64(seed))
    srs = (lo + (hi - lo) * rng.random((B, H, W))).astype(np.float32)
    hrs = rng.random((B, H, W), dtype=np.float32)
    maps = (rng.random((B, H, W)) > 0.1).astype(np.float32)
    return srs, hrs, maps


@pytest.mark.parametrize("border", [0, 1, 3])
def test_restatement_is_the_oracle_on_random_squares(border):
    srs, hrs, maps = _random(3, 29, 29, 5)
    out, _, _ = R.shift_loss(_t(srs), _t(hrs), _t(maps), "cPSNR", border, clip=True)
    want = O.shift_cpsnr(np.clip(srs, 0, 1).astype(np.float64), hrs, maps, border)
    assert util.rel_err(out.numpy(), want) <= 1e-9
    cm, _, _ = R.shift_loss(_t(srs), _t(hrs), _t(maps), "cMSE", border, clip=True)
    assert util.rel_err(-10 * np.log10(cm.numpy()), want) <= 1e-9


def test_transposing_the_inputs_transposes_the_offset():
    srs, hrs, maps = _random(4, 23, 31, 6)
    out, k, _ = R.shift_loss(_t(srs), _t(hrs), _t(maps), "cPSNR", 2)
    tr = [_t(x.transpose(0, 2, 1)) for x in (srs, hrs, maps)]
    out_t, k_t, _ = R.shift_loss(*tr, "cPSNR", 2)
    assert util.rel_err(out_t.numpy(), out.numpy()) <= 1e-12
    assert torch.equal(R.offsets(k_t, 2), R.offsets(k, 2).flip(1))
    assert len({tuple(o) for o in R.offsets(k, 2).tolist()}) > 1          # the samples do not all pick one offset


def test_gradient_is_the_stated_formula_and_the_bias_term_vanishes():
    """autograd through the restatement (bias attached) == c m (s + bias - g) at the selected offset: the bias term contributes nothing"""
    srs, hrs, maps = _random(2, 17, 19, 7, 0.0, 1.0)
    s = _t(srs).double().requires_grad_(True)
    out, k, cm = R.shift_loss(s, _t(hrs), _t(maps), "cPSNR", 2)
    out.sum().backward()
    want = torch.zeros_like(s)
    for b in range(2):
        u, v = int(k[b]) // 5, int(k[b]) % 5
        g, m = _t(hrs)[b, u:u + 13, v:v + 15].double(), _t(maps)[b, u:u + 13, v:v + 15].double()
        sc = s.detach()[b, 2:15, 2:17]
        n = m.sum()
        bias = (m * (g - sc)).sum() / n
        want[b, 2:15, 2:17] = -20.0 / (np.log(10.0) * n * cm[b, k[b]]) * m * (sc + bias - g)
    assert float((s.grad - want).abs().max() / want.abs().max()) <= 1e-12


def test_no_clear_pixel_gives_nan_and_no_offset():
    srs, hrs, maps = _random(2, 12, 12, 8)
    maps[1] = 0
    out, k, _ = R.shift_loss(_t(srs), _t(hrs), _t(maps), "cMSE", 1)
    assert np.isfinite(float(out[0])) and np.isnan(float(out[1])) and int(k[1]) == -1


# ----------------------------------------------------------------------------- the new surface, host side
NAMES = ("hrn_shift_loss_workspace_bytes", "hrn_shift_loss_train", "hrn_shift_loss_backward")


@pytest.fixture(scope="module")
def lib():
    from hrnet_hip import binding, build
    if not os.path.exists(binding.LIB_PATH):
        build.build_library(verbose=False)
    return binding.load_library()


def test_exports_are_present(lib):
    from hrnet_hip import binding, build, losses
    header = open(os.path.join(os.path.dirname(util.GOLDEN), "..", "include", "hrnet_hip.h")).read()
    for n in NAMES:
        assert n in binding.SIGNATURES and hasattr(lib, n) and n + "(" in header, n
    assert "shift_loss.hip" in build.SOURCES
    assert callable(losses.shift_loss) and callable(binding.shift_loss_train) and callable(binding.shift_loss_backward)
    assert hasattr(torch.ops.hrnet_hip, "shift_loss_train") and hasattr(torch.ops.hrnet_hip, "shift_loss_backward")
    assert lib.hrn_version() == 1


def test_c_entry_points_refuse_bad_arguments_before_any_launch(lib):
    null, p = ctypes.c_void_p(0), ctypes.c_void_p(64)          # p: never dereferenced, every call below fails its checks first
    train = lambda B, H, W, border, metric, a=p: lib.hrn_shift_loss_train(a, p, p, B, H, W, border, metric, 0, p, p, p, 1 << 40, null)
    back = lambda B, H, W, border, metric, a=p: lib.hrn_shift_loss_backward(a, p, p, p, p, B, H, W, border, metric, 0, p, null)
    for f in (train, back):
        assert f(2, 16, 16, 3, 2, null) == -2 and b"null" in lib.hrn_last_error()
        assert f(2, 16, 16, 9, 2) == -2 and b"border" in lib.hrn_last_error()
        assert f(2, 16, 16, -1, 2) == -2
        assert f(2, 6, 16, 3, 2) == -2 and f(2, 16, 6, 3, 2) == -2 and b"shape" in lib.hrn_last_error()
        assert f(0, 16, 16, 3, 2) == -2
        assert f(2, 16, 16, 3, 0) == -2 and b"metric" in lib.hrn_last_error()
        assert f(65536, 16, 16, 3, 2) == -2 and b"grid" in lib.hrn_last_error()
    assert lib.hrn_shift_loss_train(p, p, p, 2, 16, 16, 3, 2, 0, p, p, p, 8, null) == -3
    ws = lib.hrn_shift_loss_workspace_bytes
    assert ws(2, 16, 16, 9) == 0 and ws(2, 6, 16, 3) == 0 and ws(0, 16, 16, 3) == 0
    # three fp64 sums per offset per tile; more rows or columns never need less
    assert ws(2, 16, 16, 3) >= 2 * 49 * 3 * 8 and ws(2, 16, 16, 3) % (49 * 3 * 8) == 0
    assert ws(1, 4608, 6144, 3) >= ws(1, 384, 384, 3) >= ws(1, 16, 16, 3)
    assert ws(4, 96, 96, 0) == 4 * ws(1, 96, 96, 0)


def test_python_argument_errors():
    from hrnet_hip import losses
    a = torch.zeros(2, 16, 16)
    with pytest.raises(ValueError, match="metric"):
        losses.shift_loss(a, a, a, metric="masked_MSE")
    with pytest.raises(ValueError, match="equal"):
        losses.shift_loss(a, a[:, :12], a)
    with pytest.raises(ValueError, match="equal"):
        losses.shift_loss(torch.zeros(2, 2, 16, 16), a, a)
    with pytest.raises(ValueError, match="border_w"):
        losses.shift_loss(torch.zeros(2, 16, 6), torch.zeros(2, 16, 6), torch.zeros(2, 16, 6), border_w=3)
    with pytest.raises(ValueError, match="border_w"):
        losses.shift_loss(torch.zeros(2, 40, 40), torch.zeros(2, 40, 40), torch.zeros(2, 40, 40), border_w=9)
    with pytest.raises(TypeError, match="no CPU fallback"):
        losses.shift_loss(a, a, a)
    with pytest.raises(TypeError, match="torch.Tensor"):
        losses.shift_loss(a.numpy(), a, a)
