"""HRNet.train_precision (config key "train_precision"): parsing without a GPU, and the C ABI's dtype check of the training entry
points - HRN_DTYPE_BF16 now passes it, so a bad argument behind it is what fails (still -2 before any launch)."""
import copy
import ctypes

import pytest

from hrnet_hip import binding
from oracle import weights


def _net(**extra):
    from DeepNetworks.HRNet import HRNet
    cfg = copy.deepcopy(weights.HRNET_CONFIG)
    cfg.update(extra)
    return HRNet(cfg)


def test_train_precision_defaults_to_none():
    m = _net()
    assert m.train_precision is None and m._train_dtype() is None


@pytest.mark.parametrize("name,dt", [("fp32", binding.F32), ("f32", binding.F32), ("float32", binding.F32), ("bf16", binding.BF16),
                                     ("BF16", binding.BF16), ("bfloat16", binding.BF16), ("bf16x3", binding.BF16X3)])
def test_train_precision_aliases(name, dt):
    m = _net(train_precision=name)
    assert m.train_precision == name and m._train_dtype() == dt
    assert m._dtype() == binding.F32                     # `precision` is untouched


def test_train_precision_unknown_value_raises():
    m = _net(train_precision="fp16")
    with pytest.raises(ValueError, match="train_precision"):
        m._train_dtype()
    m.train_precision = "bf16"
    assert m._train_dtype() == binding.BF16


@pytest.fixture(scope="module")
def lib():
    try:
        return binding.load_library()
    except (RuntimeError, OSError) as e:
        pytest.skip(f"libhrnet_hip.so not built: {e}")


def test_training_entry_points_accept_bf16(lib):
    p = ctypes.c_void_p
    P = binding.HrnetParams()
    P.num_layers = 2
    # a null argument behind the dtype check: the error names it, not the dtype
    rc = lib.hrn_hrnet_forward_train_s(p(1), binding.BF16, 2, 3, 1, None, p(1), 2, 4, 8, 8, p(1), p(1), 1 << 40, None)
    assert rc == -2 and b"null" in lib.hrn_last_error()
    rc = lib.hrn_hrnet_backward_in(p(1), binding.BF16, 3, ctypes.byref(P), 1, None, p(1), 2, 4, 8, 8, p(1), ctypes.byref(P), None, None,
                                   p(1), 1 << 40, None)
    assert rc == -2 and b"null" in lib.hrn_last_error()
    for dt in (3, 7):
        rc = lib.hrn_hrnet_forward_train_s(p(1), dt, 2, 3, 1, p(1), p(1), 2, 4, 8, 8, p(1), p(1), 1 << 40, None)
        assert rc == -2 and b"dtype" in lib.hrn_last_error()


def _call_in(lib, dt=0, scale=3, packed=1, params=True, grads=True, lrs=1, alphas=1, d_sr=1, tws=1, d_lrs=None, d_alphas=None):
    p = ctypes.c_void_p
    P = binding.HrnetParams()
    P.num_layers = 2
    return lib.hrn_hrnet_backward_in(p(packed), dt, scale, ctypes.byref(P) if params else None, 1, p(lrs), p(alphas), 2, 4, 8, 8,
                                     p(d_sr), ctypes.byref(P) if grads else None, p(d_lrs), p(d_alphas), p(tws), 1 << 40, None)


def test_backward_in_bad_scale_dtype_and_nulls_return_minus_2(lib):
    """hrn_hrnet_backward_in's argument checks with every training dtype valid (0, 1, 2): only other dtypes are refused as such."""
    assert _call_in(lib, scale=5) == -2 and b"scale" in lib.hrn_last_error()
    for dt in (-1, 3, 7):
        assert _call_in(lib, dt=dt) == -2 and b"dtype" in lib.hrn_last_error()
    for dt in (binding.F32, binding.BF16, binding.BF16X3):
        for kw in ({"packed": None}, {"params": False}, {"grads": False}, {"lrs": None}, {"alphas": None}, {"d_sr": None}, {"tws": None}):
            assert _call_in(lib, dt=dt, d_lrs=1, d_alphas=1, **kw) == -2 and b"null" in lib.hrn_last_error(), (dt, kw)


@pytest.mark.parametrize("dt", [binding.F32, binding.BF16, binding.BF16X3])
def test_misaligned_blob_or_workspace_returns_minus_2(lib, dt):
    """packed and train_ws must be 256-byte aligned in every dtype: refused on the host, before any launch."""
    p = ctypes.c_void_p
    P = binding.HrnetParams()
    P.num_layers = 2
    for pk, tws in ((1, 256), (256, 1), (256, 256 + 16)):
        rc = lib.hrn_hrnet_forward_train_s(p(pk), dt, 2, 3, 1, p(256), p(256), 2, 4, 8, 8, p(256), p(tws), 1 << 40, None)
        assert rc == -2 and b"aligned" in lib.hrn_last_error(), (pk, tws)
        assert _call_in(lib, dt=dt, packed=pk, tws=tws) == -2 and b"aligned" in lib.hrn_last_error(), (pk, tws)
