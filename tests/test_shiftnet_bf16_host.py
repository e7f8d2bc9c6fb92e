"""ShiftNet.train_precision (keyword, attribute, HRNET_HIP_SHIFTNET_TRAIN_PRECISION): parsing without a GPU, and the dtype-aware C ABI of
ShiftNet's training path (hrn_shiftnet_train_workspace_bytes_dt / hrn_shiftnet_forward_train_dt / hrn_shiftnet_backward_dt): sizes and the
argument checks that return before any launch."""
import ctypes

import pytest

from hrnet_hip import binding

ENV = "HRNET_HIP_SHIFTNET_TRAIN_PRECISION"


def _net(**kw):
    from DeepNetworks.ShiftNet import ShiftNet
    return ShiftNet(**kw)


def test_default_is_none(monkeypatch):
    monkeypatch.delenv(ENV, raising=False)
    m = _net()
    assert m.train_precision is None and m._train_dtype is None


@pytest.mark.parametrize("name,dt", [("fp32", binding.F32), ("f32", binding.F32), ("float32", binding.F32), ("bf16", binding.BF16),
                                     ("BF16", binding.BF16), ("bfloat16", binding.BF16)])
def test_keyword_attribute_and_environment_set_the_mode(monkeypatch, name, dt):
    monkeypatch.delenv(ENV, raising=False)
    m = _net(train_precision=name)
    assert m.train_precision == name and m._train_dtype == dt
    m = _net()
    m.train_precision = name
    assert m.train_precision == name and m._train_dtype == dt
    m.train_precision = None
    assert m._train_dtype is None
    monkeypatch.setenv(ENV, name)
    m = _net()
    assert m.train_precision == name and m._train_dtype == dt
    assert _net(train_precision="fp32")._train_dtype == binding.F32          # the keyword wins over the environment


def test_empty_environment_variable_means_default(monkeypatch):
    monkeypatch.setenv(ENV, "")
    assert _net().train_precision is None


@pytest.mark.parametrize("bad", ["fp16", "float16", "int8", 3])
def test_unknown_values_raise_value_error(monkeypatch, bad):
    monkeypatch.delenv(ENV, raising=False)
    with pytest.raises(ValueError, match="train_precision"):
        _net(train_precision=bad)
    m = _net()
    with pytest.raises(ValueError, match="train_precision"):
        m.train_precision = bad
    assert m.train_precision is None                      # a refused value leaves the mode as it was
    monkeypatch.setenv(ENV, str(bad))
    with pytest.raises(ValueError, match="train_precision"):
        _net()


def test_bf16x3_is_not_implemented(monkeypatch):
    monkeypatch.delenv(ENV, raising=False)
    with pytest.raises(NotImplementedError):
        _net(train_precision="bf16x3")
    m = _net(train_precision="bf16")
    with pytest.raises(NotImplementedError):
        m.train_precision = "BF16X3"
    assert m._train_dtype == binding.BF16


def test_state_dict_is_unchanged(monkeypatch):
    monkeypatch.delenv(ENV, raising=False)
    ref = _net().state_dict()
    got = _net(train_precision="bf16").state_dict()
    assert list(got) == list(ref)
    assert all(tuple(got[k].shape) == tuple(ref[k].shape) and got[k].dtype == ref[k].dtype for k in ref)


@pytest.fixture(scope="module")
def lib():
    try:
        return binding.load_library()
    except (RuntimeError, OSError) as e:
        pytest.skip(f"libhrnet_hip.so not built: {e}")


def test_library_exports_the_dtype_entry_points(lib):
    for name in ("hrn_shiftnet_train_workspace_bytes_dt", "hrn_shiftnet_forward_train_dt", "hrn_shiftnet_backward_dt"):
        assert hasattr(lib, name), name


@pytest.mark.parametrize("B", [1, 3, 32, 35])
def test_workspace_sizes(lib, B):
    old = lib.hrn_shiftnet_train_workspace_bytes(B)
    assert lib.hrn_shiftnet_train_workspace_bytes_dt(binding.F32, B) == old
    bf = lib.hrn_shiftnet_train_workspace_bytes_dt(binding.BF16, B)
    assert 0 < bf < old
    for dt in (binding.BF16X3, -1, 3):
        assert lib.hrn_shiftnet_train_workspace_bytes_dt(dt, B) == 0
    assert lib.hrn_shiftnet_train_workspace_bytes_dt(binding.BF16, 0) == 0


def _fwd(lib, dt, packed=256, params=True, x=256, theta=256, tws=256):
    P = binding.ShiftnetParams()
    return lib.hrn_shiftnet_forward_train_dt(ctypes.c_void_p(packed), dt, ctypes.byref(P) if params else None, ctypes.c_void_p(x), 2, 0.1,
                                             None, ctypes.c_void_p(theta), ctypes.c_void_p(tws), 1 << 40, None)


def _bwd(lib, dt, params=True, x=256, d_theta=256, grads=True, tws=256):
    P = binding.ShiftnetParams()
    return lib.hrn_shiftnet_backward_dt(ctypes.byref(P) if params else None, dt, ctypes.c_void_p(x), 2, None, ctypes.c_void_p(d_theta),
                                        ctypes.byref(P) if grads else None, None, ctypes.c_void_p(tws), 1 << 40, None)


def test_unsupported_dtype_returns_minus_2(lib):
    for dt in (binding.BF16X3, -1, 7):
        assert _fwd(lib, dt) == -2 and b"dtype" in lib.hrn_last_error()
        assert _bwd(lib, dt) == -2 and b"dtype" in lib.hrn_last_error()


@pytest.mark.parametrize("dt", [binding.F32, binding.BF16])
def test_null_arguments_return_minus_2(lib, dt):
    for kw in ({"packed": None}, {"params": False}, {"x": None}, {"theta": None}, {"tws": None}):
        assert _fwd(lib, dt, **kw) == -2 and b"null" in lib.hrn_last_error(), kw
    for kw in ({"params": False}, {"x": None}, {"d_theta": None}, {"grads": False}, {"tws": None}):
        assert _bwd(lib, dt, **kw) == -2 and b"null" in lib.hrn_last_error(), kw


def test_null_bf16_conv_weights_return_minus_2(lib):
    """bf16 packs the conv weights from params->conv_w: with BatchNorm tensors set but conv_w null, -2 before any launch."""
    P = binding.ShiftnetParams()
    for i in range(8):
        P.bn_g[i] = P.bn_b[i] = P.bn_rm[i] = P.bn_rv[i] = 256
    P.fc1_w = 256
    rc = lib.hrn_shiftnet_forward_train_dt(ctypes.c_void_p(256), binding.BF16, ctypes.byref(P), ctypes.c_void_p(256), 2, 0.1, None,
                                           ctypes.c_void_p(256), ctypes.c_void_p(256), 1 << 40, None)
    assert rc == -2 and b"conv_w" in lib.hrn_last_error()


def test_misaligned_bf16_blob_or_workspace_returns_minus_2(lib):
    for pk, tws in ((1, 256), (256, 1), (256, 256 + 16)):
        assert _fwd(lib, binding.BF16, packed=pk, tws=tws) == -2 and b"aligned" in lib.hrn_last_error(), (pk, tws)
    assert _bwd(lib, binding.BF16, tws=256 + 16) == -2 and b"aligned" in lib.hrn_last_error()


@pytest.mark.parametrize("dt", [binding.F32, binding.BF16])
def test_small_workspace_returns_minus_3(lib, dt):
    P = binding.ShiftnetParams()
    for i in range(8):
        P.conv_w[i] = P.bn_g[i] = P.bn_b[i] = P.bn_rm[i] = P.bn_rv[i] = 256
    P.fc1_w = 256
    need = lib.hrn_shiftnet_train_workspace_bytes_dt(dt, 2)
    rc = lib.hrn_shiftnet_forward_train_dt(ctypes.c_void_p(256), dt, ctypes.byref(P), ctypes.c_void_p(256), 2, 0.1, None, ctypes.c_void_p(256),
                                           ctypes.c_void_p(256), need - 1, None)
    assert rc == -3
    rc = lib.hrn_shiftnet_backward_dt(ctypes.byref(P), dt, ctypes.c_void_p(256), 2, None, ctypes.c_void_p(256), ctypes.byref(P), None,
                                      ctypes.c_void_p(256), need - 1, None)
    assert rc == -3
