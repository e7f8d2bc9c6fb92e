"""CPU: which kernel runs a conv3x3 launch, and which descriptors are refused - through hrn_kt_conv_route, the pure step of
hrn_launch_conv3x3 (conv3x3.h: hrn_conv3x3_route), which launches nothing: every pointer below is host memory and is only compared with
NULL.

The expected table is written out here from the rules and the instance lists of conv3x3.h, not derived from the library:
  bf16x3   v6x3's instances or an error (also with scale / relu, or on the forced general route)
  bf16     without scale / relu and not forced: r64 for 64 -> 64 (plain input; no, plain or alpha residual), else v6's instances, else the
           general kernel, which files every layer under the plain name
  f32, and bf16 with scale / relu or forced: the general kernel
and a fast family whose 32-bit arithmetic an image exceeds (H W 2 max(cin, cout) >= 2^31 bytes) gives way to the general kernel - for
bf16x3, which has none, to the error tests/test_large_offsets_host.py pins.  Without a device the library counts 256 CUs (prof.hip)."""
import ctypes
import itertools
import os

import pytest
import torch

import kernel_bounds
import kt
from kt import BF16, BF16X3, F32

DT_NAME = {F32: "f32", BF16: "bf16", BF16X3: "bf16x3"}
# (cin, cout, res_mode, in_pair) of every instantiated fast kernel
V6 = {(64, 128, 0, 0), (128, 128, 0, 1), (128, 128, 2, 1), (128, 128, 0, 0), (128, 128, 1, 0), (128, 128, 2, 0), (128, 64, 0, 0), (128, 64, 3, 0)}
V6X3 = V6 | {(64, 64, 0, 0), (64, 64, 1, 0)}
R64 = {(64, 64, 0, 0), (64, 64, 1, 0), (64, 64, 3, 0)}          # <false>, <true>, <true>
H, W, PAIR_H, V, PAIR_LAST = 9, 27, 2, 7, 3                      # a level of 5 views in a stack of 7 slots, as tests/kernel_refs.py


@pytest.fixture(scope="module")
def lib():
    from hrnet_hip import binding, build
    if not os.path.exists(binding.LIB_PATH):
        build.build_library(verbose=False)
    return kt.lib()


@pytest.fixture(autouse=True)
def cus(monkeypatch):
    n = kt._cus() if torch.cuda.is_available() else 256
    monkeypatch.setattr(kernel_bounds, "_cus", lambda: n)
    return n


_BUF = (ctypes.c_float * 64)()
PTR = ctypes.cast(_BUF, ctypes.c_void_p)


def descriptor(dt, cin, cout, res_mode=0, in_pair=0, slot=False, M=2 * PAIR_H, H=H, W=W, **over):
    """a well-formed descriptor of the layer, as the fields of ConvParams (+ dt, route, cin, cout); `over` overrides fields"""
    x3 = dt == BF16X3
    pair = bool(in_pair or res_mode == 2)
    slot = slot or res_mode == 3
    d = dict(dt=dt, route=0, cin=cin, cout=cout, M=M, H=H, W=W, wpk=PTR, bias=PTR, slope=None, out=PTR, scale=None, relu=0,
             in_pair=in_pair, stack=PTR if pair or res_mode == 3 else None, pair_h=PAIR_H if pair else 0, pair_last=PAIR_LAST,
             pair_vs=V if pair else 0, res_mode=res_mode, res=PTR if res_mode in (1, 3) else None, res_vs=V if res_mode == 3 else 0,
             alphas=PTR if res_mode == 3 else None, alpha_vs=V if res_mode == 3 else 0, out_h=PAIR_H if slot else 0,
             out_vs=V if slot else 0, in_lo=64 if x3 and not in_pair else 0, stack_lo=64 if x3 and pair else 0, out_lo=64 if x3 else 0,
             res_lo=64 if x3 and res_mode in (1, 3) else 0)
    d["in"] = None if in_pair else PTR
    assert not set(over) - set(d), over
    d.update(over)
    return d


def route(lib, d):
    """-> (rc, kernel family, profiler name, grid, error message)"""
    fam, name, grid = ctypes.c_char_p(), ctypes.c_char_p(), ctypes.c_long(-1)
    rc = lib.hrn_kt_conv_route(d["dt"], d["route"], d["cin"], d["cout"], d["in"], d["stack"], d["pair_h"], d["pair_last"], d["pair_vs"], d["wpk"],
                               d["bias"], d["slope"], d["res"], d["res_mode"], d["res_vs"], d["alphas"], d["alpha_vs"], d["out"], d["out_h"],
                               d["out_vs"], d["in_lo"], d["stack_lo"], d["out_lo"], d["res_lo"], d["M"], d["H"], d["W"], d["in_pair"], d["scale"],
                               d["relu"], ctypes.byref(fam), ctypes.byref(name), ctypes.byref(grid))
    if rc:
        return rc, None, None, None, lib.hrn_last_error()
    return rc, fam.value.decode(), name.value.decode(), grid.value, b""


def expected(dt, cin, cout, res_mode, in_pair, forced, epi):
    """-> (kernel family, profiler name), or None: an error"""
    layer = (cin, cout, res_mode, in_pair)
    size = f"{cin}x{cout}"
    res = "+res" if res_mode else ""
    if dt == BF16X3:
        return ("v6x3", f"conv3x3_bf16x3_{size}{res}") if layer in V6X3 and not forced and not epi else None
    if dt == BF16 and not forced and not epi:
        if layer in R64:
            return "r64", f"conv3x3_bf16_{size}{res}"
        if layer in V6:
            return "v6", f"conv3x3_bf16_{size}{res}"
    return "general", f"conv3x3_{DT_NAME[dt]}_{size}"


def expected_grid(family, dt, cin, cout, M, H, W):
    r = 1 if family == "general" else 0         # kernel_bounds' route 1: the general kernel's tiles and grid
    return kernel_bounds._grid(r, cout, M * kernel_bounds._tiles(dt, r, cin, cout, H, W), dt)


def test_the_examples_of_the_table():
    assert expected(BF16, 128, 128, 3, 0, False, None) == ("general", "conv3x3_bf16_128x128")
    assert expected(BF16, 128, 128, 1, 1, False, None) == ("general", "conv3x3_bf16_128x128")
    assert expected(BF16, 128, 64, 1, 0, False, None) == ("general", "conv3x3_bf16_128x64")
    assert expected(BF16, 64, 64, 3, 0, False, None) == ("r64", "conv3x3_bf16_64x64+res")
    assert expected(BF16X3, 128, 64, 1, 0, False, None) is None
    assert expected(BF16, 128, 128, 2, 1, False, None) == ("v6", "conv3x3_bf16_128x128+res")
    assert expected(BF16, 128, 128, 2, 1, False, "relu") == ("general", "conv3x3_bf16_128x128")
    assert expected(F32, 64, 128, 0, 0, False, None) == ("general", "conv3x3_f32_64x128")
    assert len(V6) == 8 and len(V6X3) == 10


@pytest.mark.parametrize("dt", [F32, BF16, BF16X3], ids=DT_NAME.get)
def test_route_table(lib, dt):
    """every (cin, cout), res_mode, in_pair, route and scale / relu at 9 x 27, M = 2 pair_h: the family, the profiler name and the grid"""
    seen = set()
    for cin, cout, res_mode, in_pair, forced, epi in itertools.product((64, 128), (64, 128), range(4), (0, 1), (False, True),
                                                                       (None, "scale", "relu")):
        d = descriptor(dt, cin, cout, res_mode, in_pair, route=int(forced), scale=PTR if epi == "scale" else None, relu=int(epi == "relu"))
        rc, fam, name, grid, err = route(lib, d)
        tag = (DT_NAME[dt], cin, cout, res_mode, in_pair, forced, epi)
        if (in_pair and cin != 128) or (res_mode == 2 and cout != 128):        # no such layer: outside the descriptor contract
            assert rc == -2 and (b"cin" in err if in_pair and cin != 128 else b"cout" in err), (tag, rc, err)
            continue
        want = expected(dt, cin, cout, res_mode, in_pair, forced, epi)
        if want is None:
            assert rc == -2 and b"bf16x3" in err, (tag, rc, err)
            continue
        assert rc == 0 and (fam, name) == want, (tag, rc, fam, name, err)
        assert grid == expected_grid(fam, dt, cin, cout, d["M"], H, W) and 0 < grid < 16, (tag, grid)
        seen.add(fam)
    assert seen == {F32: {"general"}, BF16: {"general", "r64", "v6"}, BF16X3: {"v6x3"}}[dt]


@pytest.mark.parametrize("dt,cin,cout,res_mode,in_pair,forced", [
    (BF16, 64, 64, 1, 0, False), (BF16, 128, 128, 2, 1, False), (BF16, 128, 64, 3, 0, False), (BF16, 64, 128, 0, 0, False),
    (BF16X3, 64, 64, 0, 0, False), (BF16X3, 128, 128, 0, 1, False), (BF16, 64, 64, 1, 0, True), (BF16, 128, 128, 3, 0, False),
    (F32, 64, 64, 0, 0, False), (F32, 128, 128, 2, 0, False)])
def test_grid_below_and_above_the_cu_count(lib, cus, dt, cin, cout, res_mode, in_pair, forced):
    """the persistent grid: every tile its own workgroup while there are fewer tiles than one round, then one round, a multiple of 8"""
    for M in (2 * PAIR_H, 6 * PAIR_H, 600 * PAIR_H):
        rc, fam, _, grid, err = route(lib, descriptor(dt, cin, cout, res_mode, in_pair, M=M, route=int(forced)))
        assert rc == 0, err
        total = M * kernel_bounds._tiles(dt, 1 if fam == "general" else 0, cin, cout, H, W)
        assert grid == expected_grid(fam, dt, cin, cout, M, H, W), (fam, M, grid)
        assert grid <= total and (grid == total or grid % 8 == 0)
        if M == 600 * PAIR_H:
            per_cu = 2 // (cout // 64) if fam == "general" else 1
            assert total > per_cu * cus and grid == (per_cu * cus) & ~7


# H W 2 max(cin, cout) one step below 2^31 and at it (the shapes of tests/test_gpu_large_offsets.py's FRAME_CONV)
LIMIT = [(BF16, "r64", 64, 64, 0, 4096), (BF16, "r64", 64, 64, 1, 4096), (BF16, "v6", 128, 64, 3, 2048), (BF16, "v6", 128, 64, 0, 2048),
         (BF16, "v6", 64, 128, 0, 2048), (BF16, "v6", 128, 128, 1, 2048), (BF16X3, "v6x3", 64, 64, 1, 4096), (BF16X3, "v6x3", 64, 128, 0, 2048),
         (BF16X3, "v6x3", 128, 64, 3, 2048), (BF16X3, "v6x3", 128, 128, 0, 2048)]


@pytest.mark.parametrize("dt,family,cin,cout,res_mode,rows", LIMIT, ids=[f"{DT_NAME[a]}-{c}x{d}-res{e}" for a, _, c, d, e, _ in LIMIT])
def test_size_boundary(lib, dt, family, cin, cout, res_mode, rows):
    assert rows * 4096 * 2 * max(cin, cout) == 1 << 31
    size, res = f"{cin}x{cout}", "+res" if res_mode else ""
    slot_h = dict(out_h=1) if res_mode == 3 else {}
    for hh, ww in ((rows - 1, 4096), (rows, 4095)):
        rc, fam, name, _, err = route(lib, descriptor(dt, cin, cout, res_mode, M=1, H=hh, W=ww, **slot_h))
        assert rc == 0 and (fam, name) == (family, f"conv3x3_{DT_NAME[dt]}_{size}{res}"), (hh, ww, rc, fam, name, err)
    rc, fam, name, _, err = route(lib, descriptor(dt, cin, cout, res_mode, M=1, H=rows, W=4096, **slot_h))
    if dt == BF16X3:
        assert rc == -2 and f"conv3x3 bf16x3: image too large for 32-bit in-image offsets (H={rows} W=4096)".encode() in err, (rc, err)
    else:
        assert rc == 0 and (fam, name) == ("general", f"conv3x3_bf16_{size}"), (rc, fam, name, err)


def test_tile_total_boundary(lib):
    """the other 32-bit limit, the tile total below 2^30: 2^30 one-pixel images are 2^30 tiles"""
    for dt in (BF16, BF16X3):
        rc, fam, _, _, err = route(lib, descriptor(dt, 64, 64, M=(1 << 30) - 1, H=1, W=1))
        assert rc == 0 and fam == ("r64" if dt == BF16 else "v6x3"), (rc, fam, err)
        rc, fam, _, _, err = route(lib, descriptor(dt, 64, 64, M=1 << 30, H=1, W=1))
        assert (rc == 0 and fam == "general") if dt == BF16 else (rc == -2 and b"image too large" in err), (rc, fam, err)


# ---- the descriptor contract: (base layer, the one field set wrong, what the message must name)
PLAIN, PAIRIN, PAIRRES, RES1, ALPHA, SLOT = ((64, 64, 0, 0, False), (128, 128, 0, 1, False), (128, 128, 2, 0, False), (64, 64, 1, 0, False),
                                             (128, 64, 3, 0, False), (128, 64, 0, 0, True))
BASES = [PLAIN, PAIRIN, PAIRRES, RES1, ALPHA, SLOT]
VIOLATIONS = [
    (PLAIN, dict(M=0), b"M=0"), (PLAIN, dict(H=0), b"H=0"), (PLAIN, dict(W=-1), b"W=-1"),
    (PLAIN, dict(wpk=None), b"wpk"), (PLAIN, dict(bias=None), b"bias"), (PLAIN, dict(out=None), b"out"), (PLAIN, {"in": None}, b"null in"),
    (PLAIN, dict(res_mode=4), b"res_mode"), (PLAIN, dict(res_mode=-1), b"res_mode"),
    (PLAIN, dict(in_pair=1, stack=PTR, pair_h=PAIR_H, pair_vs=V, stack_lo=64), b"in_pair needs cin=128"),
    (PLAIN, dict(cin=32), b"cin=32"), (PLAIN, dict(cout=256), b"cout=256"), (PLAIN, dict(dt=3), b"dt=3"),
    (PAIRIN, dict(stack=None), b"stack"), (PAIRIN, dict(pair_h=0), b"pair_h"), (PAIRIN, dict(M=2 * PAIR_H + 1), b"pair_h"),
    (PAIRIN, dict(pair_last=PAIR_H - 2), b"pair_last"), (PAIRIN, dict(pair_last=V), b"pair_vs"), (PAIRIN, dict(pair_vs=PAIR_LAST), b"pair_vs"),
    (PAIRRES, dict(stack=None), b"stack"), (PAIRRES, dict(pair_h=0), b"pair_h"), (PAIRRES, dict(M=2 * PAIR_H + 1), b"pair_h"),
    (PAIRRES, dict(pair_last=PAIR_H - 2), b"pair_last"), (PAIRRES, dict(pair_last=V), b"pair_vs"),
    (PAIRRES, dict(cout=64), b"res_mode 2 needs cout=128"),
    (RES1, dict(res=None), b"res_mode 1 needs res"),
    (ALPHA, dict(res=None), b"res_mode 3 needs res"), (ALPHA, dict(out_h=0), b"out_h"), (ALPHA, dict(res_vs=PAIR_H - 1), b"res_vs"),
    (ALPHA, dict(pair_last=PAIR_H - 2), b"pair_last"), (ALPHA, dict(pair_last=V), b"alpha_vs"), (ALPHA, dict(alpha_vs=PAIR_LAST), b"alpha_vs"),
    (ALPHA, dict(M=2 * PAIR_H + 1), b"out_h"), (ALPHA, dict(out_vs=PAIR_H - 1), b"out_vs"),
    (SLOT, dict(M=2 * PAIR_H + 1), b"out_h"), (SLOT, dict(out_vs=PAIR_H - 1), b"out_vs"),
]
X3_VIOLATIONS = [
    (PLAIN, dict(out_lo=0), b"out_lo"), (PLAIN, dict(in_lo=0), b"in_lo"), (PAIRIN, dict(stack_lo=0), b"stack_lo"),
    (PLAIN, dict(scale=PTR), b"scale"), (PLAIN, dict(relu=1), b"relu"), (PLAIN, dict(route=1), b"no general kernel"),
]


def _base(dt, base, over):
    cin, cout, res_mode, in_pair, slot = base
    d = descriptor(dt, cin, cout, res_mode, in_pair, slot)
    assert not set(over) - set(d), over
    d.update(over)
    return d


@pytest.mark.parametrize("dt", [F32, BF16, BF16X3], ids=DT_NAME.get)
def test_descriptor_contract(lib, dt):
    """each base descriptor is accepted; with ONE clause of the contract violated it is -2 and the message names the field"""
    for base in BASES:
        rc, _, _, _, err = route(lib, _base(dt, base, {}))
        assert rc == 0, (base, err)
    for base, wrong, names in VIOLATIONS + (X3_VIOLATIONS if dt == BF16X3 else []):
        rc, fam, _, _, err = route(lib, _base(dt, base, wrong))
        assert rc == -2 and names in err and err.startswith(b"conv3x3"), (DT_NAME[dt], base, wrong, rc, fam, err)
    # null alphas: res_mode 3 reads no alpha, and pair_last is free
    rc, _, _, _, err = route(lib, _base(dt, ALPHA, dict(alphas=None, alpha_vs=0, pair_last=-5)))
    assert rc == 0, err
