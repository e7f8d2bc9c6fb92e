"""hrn_hrnet_backward_in's argument checks: bad arguments fail with -2 before any launch, so no device is needed."""
import ctypes

import pytest

from hrnet_hip import binding


@pytest.fixture(scope="module")
def lib():
    try:
        return binding.load_library()
    except (RuntimeError, OSError) as e:
        pytest.skip(f"libhrnet_hip.so not built: {e}")


def _call(lib, dt=0, scale=3, packed=1, params=True, grads=True, lrs=1, alphas=1, d_sr=1, tws=1, d_lrs=None, d_alphas=None):
    p = ctypes.c_void_p
    P = binding.HrnetParams()
    P.num_layers = 2
    return lib.hrn_hrnet_backward_in(p(packed), dt, scale, ctypes.byref(P) if params else None, 1, p(lrs), p(alphas), 2, 4, 8, 8,
                                     p(d_sr), ctypes.byref(P) if grads else None, p(d_lrs), p(d_alphas), p(tws), 1 << 40, None)


def test_bad_scale_dtype_and_nulls_return_minus_2(lib):
    assert _call(lib, scale=5) == -2 and b"scale" in lib.hrn_last_error()
    assert _call(lib, dt=1) == -2 and b"dtype" in lib.hrn_last_error()
    assert _call(lib, dt=7) == -2 and b"dtype" in lib.hrn_last_error()
    for kw in ({"packed": None}, {"params": False}, {"grads": False}, {"lrs": None}, {"alphas": None}, {"d_sr": None}, {"tws": None}):
        assert _call(lib, d_lrs=1, d_alphas=1, **kw) == -2 and b"null" in lib.hrn_last_error(), kw


def test_backward_s_is_the_null_null_case(lib):
    """hrn_hrnet_backward_s shares the checks (it is hrn_hrnet_backward_in with both input-gradient pointers NULL)."""
    p = ctypes.c_void_p
    P = binding.HrnetParams()
    rc = lib.hrn_hrnet_backward_s(p(1), 0, 5, ctypes.byref(P), 1, p(1), p(1), 2, 4, 8, 8, p(1), ctypes.byref(P), p(1), 1 << 40, None)
    assert rc == -2 and b"scale" in lib.hrn_last_error()
