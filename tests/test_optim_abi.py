"""CPU: the guarded optimiser's C ABI (include/hrnet_hip.h: hrn_grad_sumsq*, hrn_optim_prepare, hrn_adam_step_ex).  The library loads
without a GPU, the new symbols are in the ctypes table, and every refusal returns -2 with a message that names the argument - before any
launch: every call here carries exactly one fault, and its pointers are host memory no kernel could use."""
import ctypes
import os

import pytest


@pytest.fixture(scope="module")
def lib():
    from hrnet_hip import binding, build
    if not os.path.exists(binding.LIB_PATH):
        build.build_library(verbose=False)
    return binding.load_library()


_keep = []


def _buf(nbytes=256, misalign=0):
    """a host pointer, 16-byte aligned (+ misalign)"""
    raw = ctypes.create_string_buffer(nbytes + 32)
    _keep.append(raw)
    return ctypes.c_void_p((ctypes.addressof(raw) + 15) // 16 * 16 + misalign)


NULL = ctypes.c_void_p(0)
NEW = ["hrn_grad_sumsq_workspace_bytes", "hrn_grad_sumsq", "hrn_optim_prepare", "hrn_adam_step_ex"]


def test_new_symbols_are_exported_and_in_the_ctypes_table(lib):
    from hrnet_hip import binding
    for name in NEW:
        assert name in binding.SIGNATURES and hasattr(lib, name), name
    assert binding.OPTIM_MAX_GROUPS == 8 and binding.OPTIM_CTL_BYTES == 48
    # the control block's layout as the header states it
    assert {k: off for k, (off, _) in binding.OPTIM_CTL_FIELDS.items()} == dict(applied=0, skipped=8, norm=16, coef=24, step_size=28,
                                                                                 inv_bc2_sqrt=32, lr=36, skip=40)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hrnet_hip.h")).read()
    assert "#define HRN_OPTIM_MAX_GROUPS 8" in header and "typedef struct hrn_optim_ctl" in header


def test_workspace_bytes_follow_the_grid(lib):
    f = lib.hrn_grad_sumsq_workspace_bytes
    assert f(0) == f(1) == f(4 * 256) == 16 and f(4 * 256 + 4) == 32          # one (sum, count) pair of doubles per block of 256 x 4 elements
    assert f(1024 * 256 * 4) == f(1024 * 256 * 4 + 7) == f(1 << 40) == 1024 * 16      # at most 1024 blocks: the grid strides beyond


def _refused(lib, rc, *words):
    msg = lib.hrn_last_error().decode()
    assert rc == -2, (rc, msg)
    for w in words:
        assert w in msg, (w, msg)


def test_grad_sumsq_refusals(lib):
    g, out, ws = _buf(), _buf(), _buf(1024 * 16)
    call = lib.hrn_grad_sumsq
    _refused(lib, call(NULL, 8, out, ws, 16, NULL), "hrn_grad_sumsq", "grads")
    _refused(lib, call(g, 8, NULL, ws, 16, NULL), "hrn_grad_sumsq", "out")
    _refused(lib, call(g, 8, out, NULL, 16, NULL), "hrn_grad_sumsq", "ws")
    _refused(lib, call(_buf(misalign=4), 8, out, ws, 16, NULL), "hrn_grad_sumsq", "16-byte aligned")
    _refused(lib, call(g, 8, out, ws, 15, NULL), "hrn_grad_sumsq", "ws_bytes", "15 < 16")
    _refused(lib, call(g, 4 * 256 + 4, out, ws, 16, NULL), "hrn_grad_sumsq", "ws_bytes", "16 < 32")
    _refused(lib, call(g, 0, out, ws, 0, NULL), "hrn_grad_sumsq", "ws_bytes")          # n == 0 still needs its 16 bytes and its out


def test_optim_prepare_refusals(lib):
    sums, ctl = _buf(), _buf(8 * 48)
    call = lib.hrn_optim_prepare
    _refused(lib, call(NULL, 1, 0, 1.0, 1e-3, 0.9, 0.999, ctl, NULL), "hrn_optim_prepare", "sums")
    _refused(lib, call(sums, 1, 0, 1.0, 1e-3, 0.9, 0.999, NULL, NULL), "hrn_optim_prepare", "ctl")
    for n_groups in (0, -1, 9):
        _refused(lib, call(sums, n_groups, 0, 1.0, 1e-3, 0.9, 0.999, ctl, NULL), "hrn_optim_prepare", "n_groups", "1..8")
    for n_groups, group in ((1, 1), (8, 8), (3, -1)):
        _refused(lib, call(sums, n_groups, group, 1.0, 1e-3, 0.9, 0.999, ctl, NULL), "hrn_optim_prepare", "group", f"0..{n_groups - 1}")
    for b in (1.0, -0.1, float("nan")):
        _refused(lib, call(sums, 1, 0, 1.0, 1e-3, b, 0.999, ctl, NULL), "hrn_optim_prepare", "beta1")
        _refused(lib, call(sums, 1, 0, 1.0, 1e-3, 0.9, b, ctl, NULL), "hrn_optim_prepare", "beta2")


def test_adam_step_ex_refusals(lib):
    p, g, m, v, ema, ctl = (_buf() for _ in range(6))
    call = lib.hrn_adam_step_ex
    tail = (8, 0.9, 0.999, 1e-8, 0.0, 0, 0.99)
    for k, name in enumerate(("params", "grads", "exp_avg", "exp_avg_sq")):
        ptrs = [p, g, m, v]
        ptrs[k] = NULL
        _refused(lib, call(*ptrs, ema, *tail, ctl, NULL), "hrn_adam_step_ex", name + " is null")
    _refused(lib, call(p, g, m, v, NULL, *tail, NULL, NULL), "hrn_adam_step_ex", "ctl")
    for b in (1.0, -0.1, float("nan")):
        _refused(lib, call(p, g, m, v, NULL, 8, b, 0.999, 1e-8, 0.0, 0, 0.0, ctl, NULL), "hrn_adam_step_ex", "beta1")
        _refused(lib, call(p, g, m, v, NULL, 8, 0.9, b, 1e-8, 0.0, 0, 0.0, ctl, NULL), "hrn_adam_step_ex", "beta2")
        _refused(lib, call(p, g, m, v, ema, 8, 0.9, 0.999, 1e-8, 0.0, 0, b, ctl, NULL), "hrn_adam_step_ex", "ema_decay")
    _refused(lib, call(p, g, m, v, _buf(misalign=8), *tail, ctl, NULL), "hrn_adam_step_ex", "16-byte aligned")
    # without an EMA buffer its decay is not looked at, and n == 0 is a no-op: neither launches anything
    assert call(p, g, m, v, NULL, 0, 0.9, 0.999, 1e-8, 0.0, 0, 7.0, ctl, NULL) == 0
