"""CPU: the C ABI for frozen parameters - hrn_hrnet_backward_sel / hrn_shiftnet_backward_sel are declared, bound and exported, and their
argument checks (NULL arguments, dtype, scale, workspace size) return -2 / -3 before any launch, so no device is needed.  The launch
counters of the test hooks (hrn_kt_launch_count) stay at zero through all of it."""
import ctypes
import os
import re

import pytest

from hrnet_hip import binding
import kt
from kt import COUNTERS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hrn_hrnet_backward_sel", "hrn_shiftnet_backward_sel")


@pytest.fixture(scope="module")
def lib():
    try:
        return kt.lib()
    except (RuntimeError, OSError) as e:
        pytest.skip(f"libhrnet_hip.so not built: {e}")


def test_declared_bound_and_exported(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hrnet_hip.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in binding.SIGNATURES and hasattr(lib, name)
    # same arguments as the entry points they select from
    assert binding.SIGNATURES["hrn_hrnet_backward_sel"] == binding.SIGNATURES["hrn_hrnet_backward_in"]
    assert binding.SIGNATURES["hrn_shiftnet_backward_sel"] == binding.SIGNATURES["hrn_shiftnet_backward_dt"]
    # the launch counters are a test hook, not part of the public header
    assert "hrn_kt_launch_count" not in text and hasattr(lib, "hrn_kt_launch_count") and hasattr(lib, "hrn_kt_launch_count_reset")
    assert lib.hrn_kt_launch_count(b"no_such_kernel") == -1


def _hrnet(lib, dt=0, scale=3, packed=256, params=True, grads=True, lrs=256, alphas=256, d_sr=256, tws=256, tws_bytes=1 << 40,
           d_lrs=None, d_alphas=None):
    p = ctypes.c_void_p
    P = binding.HrnetParams()
    P.num_layers = 2
    G = binding.HrnetParams()             # every field NULL: nothing requested (the struct itself is still required)
    G.num_layers = 2
    return lib.hrn_hrnet_backward_sel(p(packed), dt, scale, ctypes.byref(P) if params else None, 1, p(lrs), p(alphas), 2, 4, 8, 8, p(d_sr),
                                      ctypes.byref(G) if grads else None, p(d_lrs), p(d_alphas), p(tws), tws_bytes, None)


def _shiftnet(lib, dt=0, params=True, grads=True, x=256, d_theta=256, tws=256, tws_bytes=1 << 40, B=2):
    p = ctypes.c_void_p
    P = binding.ShiftnetParams()
    G = binding.ShiftnetParams()
    return lib.hrn_shiftnet_backward_sel(ctypes.byref(P) if params else None, dt, p(x), B, None, p(d_theta),
                                         ctypes.byref(G) if grads else None, None, p(tws), tws_bytes, None)


def _counts(lib):
    return {c: lib.hrn_kt_launch_count(c.encode()) for c in COUNTERS}


def test_hrnet_backward_sel_rejects_before_any_launch(lib):
    lib.hrn_kt_launch_count_reset()
    assert _hrnet(lib, scale=5) == -2 and b"scale" in lib.hrn_last_error()
    assert _hrnet(lib, dt=7) == -2 and b"dtype" in lib.hrn_last_error()
    for kw in ({"packed": None}, {"params": False}, {"grads": False}, {"lrs": None}, {"alphas": None}, {"d_sr": None}, {"tws": None}):
        assert _hrnet(lib, d_lrs=256, d_alphas=256, **kw) == -2 and b"null" in lib.hrn_last_error(), kw
    assert _hrnet(lib, packed=257) == -2 and b"aligned" in lib.hrn_last_error()
    need = lib.hrn_hrnet_train_workspace_bytes(2, 2, 4, 8, 8)
    assert need > 0
    for dt in (0, 1, 2):
        assert _hrnet(lib, dt=dt, tws_bytes=need - 1) == -3 and b"too small" in lib.hrn_last_error()
    assert set(_counts(lib).values()) == {0}


def test_shiftnet_backward_sel_rejects_before_any_launch(lib):
    lib.hrn_kt_launch_count_reset()
    assert _shiftnet(lib, dt=2) == -2 and b"dtype" in lib.hrn_last_error()            # bf16x3 ShiftNet training stays refused
    for kw in ({"params": False}, {"grads": False}, {"x": None}, {"d_theta": None}, {"tws": None}):
        assert _shiftnet(lib, **kw) == -2 and b"null" in lib.hrn_last_error(), kw
    assert _shiftnet(lib, B=0) == -2
    for dt in (0, 1):
        need = lib.hrn_shiftnet_train_workspace_bytes_dt(dt, 2)
        assert _shiftnet(lib, dt=dt, tws_bytes=need - 1) == -3 and b"too small" in lib.hrn_last_error()
    assert set(_counts(lib).values()) == {0}


def test_workspace_sizes_are_unchanged(lib):
    """Nothing new goes into the workspaces: the sizes the selective entry points check are the ones of the full backward."""
    for B, V, H in ((2, 5, 16), (32, 32, 64)):
        assert lib.hrn_hrnet_train_workspace_bytes(2, B, V, H, H) > 0
    lib.hrn_kt_launch_count_reset()
    need = lib.hrn_hrnet_train_workspace_bytes(2, 2, 4, 8, 8)
    assert _hrnet(lib, tws_bytes=need - 1) == -3 and (b"(%d < %d)" % (need - 1, need)) in lib.hrn_last_error()
    need = lib.hrn_shiftnet_train_workspace_bytes(2)
    assert _shiftnet(lib, tws_bytes=need - 1) == -3 and (b"(%d < %d)" % (need - 1, need)) in lib.hrn_last_error()


def test_selective_ops_are_registered():
    import torch
    ops = torch.ops.hrnet_hip
    s = str(ops.hrnet_backward_sel.default._schema)
    assert "bool[] need_params, bool need_lrs, bool need_alphas" in s and "Tensor(a5!) tws" in s
    s = str(ops.shiftnet_backward_sel.default._schema)
    assert "bool need_input_grad, SymInt dtype, bool[] need_params" in s
    # the existing ops keep their schemas
    assert str(ops.hrnet_backward_in.default._schema).endswith("bool need_lrs, bool need_alphas) -> (Tensor[], Tensor, Tensor)")
    assert "need_params" not in str(ops.shiftnet_backward.default._schema)
