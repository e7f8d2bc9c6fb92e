"""CPU: the C entry points of the observation model's derivative in the shifts (csrc/observe_shift.hip) are declared, exported and bound
with the declared types, refuse bad arguments with -2 before any launch (no device is touched: the pointers below are never
dereferenced), and the workspace query states the bytes."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
c = ctypes
# this file's own table: what the header has to declare, argument by argument
TABLE = {
    "hrn_observe_shift_workspace_bytes": (c.c_size_t, [c.c_int] * 4),
    "hrn_observe_shift_grad": (c.c_int, [c.c_void_p] * 7 + [c.c_size_t] + [c.c_int] * 5 + [c.c_void_p]),
    "hrn_observe_shift_grad_finish": (c.c_int, [c.c_void_p, c.c_size_t] + [c.c_void_p] * 3 + [c.c_int] * 4 + [c.c_void_p]),
    "hrn_shift_normal": (c.c_int, [c.c_void_p] * 6 + [c.c_float] + [c.c_void_p] * 2 + [c.c_size_t, c.c_void_p, c.c_size_t] + [c.c_int] * 5
                         + [c.c_void_p]),
    "hrn_shift_normal_finish": (c.c_int, [c.c_void_p, c.c_size_t] + [c.c_void_p] * 5 + [c.c_int] * 6 + [c.c_float] * 2 + [c.c_void_p]),
}
NULL = c.c_void_p(0)
P_ = [c.c_void_p((k + 1) << 20) for k in range(10)]                       # ten buffers 1 MiB apart
B, V, H, W, SCALE = 1, 2, 4, 4, 3
BIG = 1 << 16


@pytest.fixture(scope="module")
def lib():
    from hrnet_hip import binding, build
    if not os.path.exists(binding.LIB_PATH):
        build.build_library(verbose=False)
    return binding.load_library()


def _grad(lib, **kw):
    a = dict(hr=P_[0], g=P_[1], masks=NULL, alphas=NULL, shifts=P_[2], beta=NULL, ws=P_[3], ws_bytes=BIG, B=B, V=V, H=H, W=W, scale=SCALE)
    a.update(kw)
    return lib.hrn_observe_shift_grad(a["hr"], a["g"], a["masks"], a["alphas"], a["shifts"], a["beta"], a["ws"], a["ws_bytes"], a["B"], a["V"],
                                      a["H"], a["W"], a["scale"], NULL)


def _grad_finish(lib, **kw):
    a = dict(ws=P_[3], ws_bytes=BIG, coef=NULL, gain=NULL, d_shifts=P_[4], B=B, V=V, H=H, W=W)
    a.update(kw)
    return lib.hrn_observe_shift_grad_finish(a["ws"], a["ws_bytes"], a["coef"], a["gain"], a["d_shifts"], a["B"], a["V"], a["H"], a["W"], NULL)


def _normal(lib, **kw):
    a = dict(hr=P_[0], lrs=P_[1], masks=NULL, alphas=NULL, shifts=P_[2], beta_prev=NULL, delta=0.1, residual=NULL, plain=NULL, plain_bytes=BIG, ws=P_[3],
             ws_bytes=BIG, B=B, V=V, H=H, W=W, scale=SCALE)
    a.update(kw)
    return lib.hrn_shift_normal(a["hr"], a["lrs"], a["masks"], a["alphas"], a["shifts"], a["beta_prev"], a["delta"], a["residual"], a["plain"],
                                a["plain_bytes"], a["ws"], a["ws_bytes"], a["B"], a["V"], a["H"], a["W"], a["scale"], NULL)


def _normal_finish(lib, **kw):
    a = dict(ws=P_[3], ws_bytes=BIG, alphas=NULL, shifts=P_[2], fixed=NULL, normal=P_[5], shifts_out=P_[6], B=B, V=V, H=H, W=W, scale=SCALE,
             damping=1e-3, max_step=0.5)
    a.update(kw)
    return lib.hrn_shift_normal_finish(a["ws"], a["ws_bytes"], a["alphas"], a["shifts"], a["fixed"], a["normal"], a["shifts_out"], a["B"], a["V"],
                                       a["H"], a["W"], a["scale"], 1, a["damping"], a["max_step"], NULL)


def test_declared_exported_and_bound_with_the_declared_types(lib):
    from hrnet_hip import binding, build
    header = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "hrnet_hip.h")).read(), flags=re.S)
    scalars = {"int": c.c_int, "float": c.c_float, "size_t": c.c_size_t}
    for name, sig in TABLE.items():
        m = re.search(r"^(\w+) " + name + r"\(([^)]*)\);", header, re.M)
        assert m, f"{name} is not declared"
        kind = lambda decl: c.c_void_p if "*" in decl else scalars[" ".join(decl.split()[:-1])]     # a parameter's last word is its name
        assert (scalars[m.group(1)], [kind(a) for a in m.group(2).split(",")]) == sig, name
        assert binding.SIGNATURES[name] == sig, name
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == sig, name
    assert "observe_shift.hip" in build.SOURCES


def test_constants_and_workspace_bytes(lib):
    from hrnet_hip import binding
    header = open(os.path.join(ROOT, "include", "hrnet_hip.h")).read()
    assert "#define HRN_SHIFT_NORMAL_SUMS 10" in header and binding.SHIFT_NORMAL_SUMS == 10 and binding.SHIFT_MIN_WEIGHT == 3.0
    th, tw = binding.OBSERVE_TILE
    tiles = lambda b, v, h, w: b * v * -(-h // th) * -(-w // tw)
    for shape in [(1, 1, 1, 1), (2, 5, 17, 63), (32, 32, 128, 128), (1, 1, 16384, 16384)]:
        assert lib.hrn_observe_shift_workspace_bytes(*shape) == 80 * tiles(*shape)            # ten fp64 sums per LR tile
    for shape in [(0, 1, 8, 8), (1, 0, 8, 8), (1, 1, 0, 8), (1, 1, 8, 16385), (-1, 1, 8, 8)]:
        assert lib.hrn_observe_shift_workspace_bytes(*shape) == 0


def test_bad_arguments_fail_before_any_launch(lib):
    required = ((_grad, ("hr", "g", "shifts", "ws")), (_grad_finish, ("ws", "d_shifts")), (_normal, ("hr", "lrs", "shifts", "ws")),
                (_normal_finish, ("ws", "shifts", "normal")))
    for fn, ptrs in required:
        for name in ptrs:
            assert fn(lib, **{name: NULL}) == -2 and b"null" in lib.hrn_last_error(), name
        for name in ("B", "V", "H", "W"):
            assert fn(lib, **{name: 0}) == -2 and b"empty" in lib.hrn_last_error(), name
            assert fn(lib, **{name: -3}) == -2, name
        assert fn(lib, H=16385) == -2 and b"16384" in lib.hrn_last_error()
        assert fn(lib, W=16385) == -2
    for fn in (_grad, _normal, _normal_finish):
        for scale in (1, 5, 0):
            assert fn(lib, scale=scale) == -2 and b"scale" in lib.hrn_last_error()
    # the workspace: too small, misaligned
    need = lib.hrn_observe_shift_workspace_bytes(B, V, H, W)
    assert need == 160
    for fn in (_grad, _grad_finish, _normal, _normal_finish):
        assert fn(lib, ws_bytes=need - 1) == -2 and b"workspace" in lib.hrn_last_error()
        assert fn(lib, ws=c.c_void_p((4 << 20) + 4)) == -2 and b"aligned" in lib.hrn_last_error()
    assert _normal_finish(lib, normal=c.c_void_p((6 << 20) + 4)) == -2 and b"aligned" in lib.hrn_last_error()
    # the options: delta only counts with beta_prev; damping and max_step only with shifts_out
    for delta in (0.0, -0.1, float("nan"), float("inf")):
        assert _normal(lib, beta_prev=P_[7], delta=delta) == -2 and b"delta" in lib.hrn_last_error(), delta
    for damping in (-1e-3, float("nan"), float("inf")):
        assert _normal_finish(lib, damping=damping) == -2 and b"damping" in lib.hrn_last_error(), damping
    for max_step in (0.0, -0.5, float("nan"), float("inf")):
        assert _normal_finish(lib, max_step=max_step) == -2 and b"max_step" in lib.hrn_last_error(), max_step
    # overlaps
    assert _grad(lib, ws=P_[0]) == -2 and b"alias" in lib.hrn_last_error()
    assert _grad(lib, ws=P_[2]) == -2 and b"alias" in lib.hrn_last_error()
    assert _grad(lib, beta=P_[3]) == -2 and b"alias" in lib.hrn_last_error()
    assert _grad_finish(lib, d_shifts=P_[3]) == -2 and b"alias" in lib.hrn_last_error()
    assert _grad_finish(lib, gain=P_[4]) == -2 and b"alias" in lib.hrn_last_error()
    assert _normal(lib, ws=P_[1]) == -2 and b"alias" in lib.hrn_last_error()
    assert _normal(lib, residual=P_[3]) == -2 and b"alias" in lib.hrn_last_error()
    assert _normal(lib, residual=P_[1]) == -2 and b"alias" in lib.hrn_last_error()
    # the optional workspace of the three plain sums: hrn_observe_workspace_bytes, aligned, apart from everything
    plain = lib.hrn_observe_workspace_bytes(B, V, H, W)
    assert plain == 48
    assert _normal(lib, plain=P_[8], plain_bytes=plain - 1) == -2 and b"plain_workspace" in lib.hrn_last_error()
    assert _normal(lib, plain=c.c_void_p((9 << 20) + 4)) == -2 and b"aligned" in lib.hrn_last_error()
    assert _normal(lib, plain=P_[3]) == -2 and b"alias" in lib.hrn_last_error()
    assert _normal(lib, plain=P_[1]) == -2 and b"alias" in lib.hrn_last_error()
    assert _normal(lib, plain=P_[8], residual=P_[8]) == -2 and b"alias" in lib.hrn_last_error()
    assert _normal_finish(lib, shifts_out=P_[2]) == -2 and b"shifts_out" in lib.hrn_last_error()          # may not be shifts itself
    assert _normal_finish(lib, shifts_out=c.c_void_p((3 << 20) + 8)) == -2 and b"alias" in lib.hrn_last_error()
    assert _normal_finish(lib, shifts_out=P_[5]) == -2 and b"alias" in lib.hrn_last_error()
    assert _normal_finish(lib, normal=P_[2]) == -2 and b"alias" in lib.hrn_last_error()
    assert _normal_finish(lib, fixed=P_[5]) == -2 and b"alias" in lib.hrn_last_error()
