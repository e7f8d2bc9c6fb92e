"""CPU: hrn_masked_composite and the three hrn_hrnet_*_ref entry points are declared, exported and bound with the declared types; they
refuse bad arguments with a negative code before any launch (no device is touched: the pointers below are never dereferenced); and
hrnet_hip.composite.masked_composite / HRNet.forward(ref=...) refuse theirs in Python."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hrn_masked_composite", "hrn_hrnet_forward_ref", "hrn_hrnet_forward_train_ref", "hrn_hrnet_backward_ref")
NULL = ctypes.c_void_p(0)


@pytest.fixture(scope="module")
def lib():
    from hrnet_hip import binding, build
    if not os.path.exists(binding.LIB_PATH):
        build.build_library(verbose=False)
    return binding.load_library()


def test_header_exports_and_signatures_agree(lib):
    from hrnet_hip import binding
    text = open(os.path.join(ROOT, "include", "hrnet_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    for name in NEW:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared in include/hrnet_hip.h"
        assert name in binding.SIGNATURES and hasattr(lib, name), name
        res, args = binding.SIGNATURES[name]
        params = [a.strip() for a in m.group(1).split(",")]
        assert res is ctypes.c_int and len(params) == len(args), name
        for decl, ct in zip(params, args):          # (tests/test_abi.py compares every type of every entry point; here: pointers and ints)
            want = (ctypes.POINTER(binding.HrnetParams) if "hrn_hrnet_params" in decl else ctypes.c_void_p) if "*" in decl else \
                (ctypes.c_size_t if decl.startswith("size_t") else ctypes.c_int)
            assert ct is want, (name, decl, ct)
    # the _ref forms are the forms they extend plus the frame (and its gradient)
    n = lambda s: len(binding.SIGNATURES[s][1])
    assert n("hrn_hrnet_forward_ref") == n("hrn_hrnet_forward_s") + 1
    assert n("hrn_hrnet_forward_train_ref") == n("hrn_hrnet_forward_train_s") + 1
    assert n("hrn_hrnet_backward_ref") == n("hrn_hrnet_backward_sel") + 2


def _composite(lib, p, **kw):
    a = dict(views=p, masks=p, alphas=p, B=2, V=5, H=8, W=9, n_ref=9, ref=p, count=p, filled=p)
    a.update(kw)
    return lib.hrn_masked_composite(a["views"], a["masks"], a["alphas"], a["B"], a["V"], a["H"], a["W"], a["n_ref"], a["ref"], a["count"],
                                    a["filled"], NULL)


def test_composite_bad_arguments_fail_before_any_launch(lib):
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    for name in ("views", "ref"):
        assert _composite(lib, p, **{name: NULL}) == -2 and b"null" in lib.hrn_last_error()
    for n_ref in (0, -1, 33, 1 << 20):
        assert _composite(lib, p, n_ref=n_ref) == -2 and b"n_ref" in lib.hrn_last_error()
    for name in ("B", "V", "H", "W"):
        for bad in (0, -3):
            assert _composite(lib, p, **{name: bad}) == -2 and b"empty" in lib.hrn_last_error()
    assert _composite(lib, p, B=1 << 20, H=1 << 12, W=1 << 12) == -2 and b"one launch" in lib.hrn_last_error()
    # the limit itself: one workgroup per (sample, tile of 256 pixels), tiles B = 2^31 exactly, with whole tiles and with a ragged last one
    for B, H, W in ((1 << 27, 64, 64), (1 << 27, 63, 61), (1 << 30, 33, 10)):
        assert -(-H * W // 256) * B == 1 << 31
        assert _composite(lib, p, B=B, H=H, W=W) == -2 and f"{B} samples of {H} x {W} exceed one launch".encode() in lib.hrn_last_error()


def test_ref_entry_points_refuse_a_null_frame_and_what_their_base_forms_refuse(lib):
    from hrnet_hip import binding
    buf = ctypes.create_string_buffer(512)
    p = ctypes.cast(buf, ctypes.c_void_p)
    P = binding.HrnetParams()
    P.num_layers = 2
    fwd = lambda ref=p, dt=0, B=1, lrs=p: lib.hrn_hrnet_forward_ref(p, dt, 2, 3, 1, lrs, p, ref, B, 2, 8, 8, p, p, 0, NULL)
    trn = lambda ref=p, dt=0, B=1, lrs=p: lib.hrn_hrnet_forward_train_ref(p, dt, 2, 3, 1, lrs, p, ref, B, 2, 8, 8, p, p, 0, NULL)
    bwd = lambda ref=p, dt=0, B=1, lrs=p: lib.hrn_hrnet_backward_ref(p, dt, 3, ctypes.byref(P), 1, lrs, p, ref, B, 2, 8, 8, p, ctypes.byref(P),
                                                                     p, p, p, p, 0, NULL)
    for call in (fwd, trn, bwd):
        assert call(ref=NULL) == -2 and b"ref" in lib.hrn_last_error()
        assert call(dt=7) == -2 and b"dtype" in lib.hrn_last_error()
        assert call(B=0) == -2
        assert call(lrs=NULL) == -2 and b"null" in lib.hrn_last_error()
    # with every pointer set the next refusal is the workspace's size (or, in training, the blob's alignment): still no launch
    assert fwd() == -3 and b"workspace" in lib.hrn_last_error()
    assert trn() in (-2, -3) and bwd() in (-2, -3)


def test_composite_py_argument_errors():
    from hrnet_hip import composite
    x = torch.zeros(2, 3, 8, 8)
    with pytest.raises(TypeError, match="lrs must be a torch.Tensor"):
        composite.masked_composite([[1.0]])
    with pytest.raises(TypeError, match="lr_masks must be"):
        composite.masked_composite(x, lr_masks=1)
    with pytest.raises(TypeError, match="alphas must be"):
        composite.masked_composite(x, alphas=[1, 1, 1])
    with pytest.raises(TypeError, match="n_ref must be an integer"):
        composite.masked_composite(x, n_ref=9.0)
    with pytest.raises(ValueError, match=r"\(B,V,H,W\)"):
        composite.masked_composite(x[0])
    with pytest.raises(ValueError, match="lr_masks must have the shape"):
        composite.masked_composite(x, lr_masks=x[:, :2])
    with pytest.raises(ValueError, match="alphas must be"):
        composite.masked_composite(x, alphas=torch.ones(2, 4))
    for bad in (0, 33, -1):
        with pytest.raises(ValueError, match="n_ref must be in 1..32"):
            composite.masked_composite(x, n_ref=bad)
    with pytest.raises(TypeError, match="ROCm device only"):          # the device comes last: every error above was raised on CPU tensors
        composite.masked_composite(x, x, torch.ones(2, 3))
    assert "LOWER median" in composite.masked_composite.__doc__ and "(c - 1) // 2" in composite.masked_composite.__doc__


def test_forward_ref_argument_errors():
    from DeepNetworks.HRNet import HRNet
    from oracle import weights
    m = HRNet({k: dict(v) for k, v in weights.HRNET_CONFIG.items()})
    lrs, alphas = torch.zeros(2, 3, 8, 8), torch.ones(2, 3)
    for call in (m.forward, m.forward_ensemble, m.forward_tiled):
        with pytest.raises(TypeError, match="ref must be a torch.Tensor"):
            call(lrs, alphas, ref=[0.0])
        with pytest.raises(TypeError, match="floating-point"):
            call(lrs, alphas, ref=torch.zeros(2, 8, 8, dtype=torch.int32))
        for shape in ((2, 8, 9), (1, 8, 8), (2, 1, 8, 8)):
            with pytest.raises(ValueError, match=r"ref must be \(B,H,W\)"):
                call(lrs, alphas, ref=torch.zeros(shape))
        with pytest.raises(RuntimeError, match="must be on the views' device"):
            call(lrs, alphas, ref=torch.zeros(2, 8, 8, device="meta"))


def test_composite_bench_command_line_and_byte_floors():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import composite_bench
    o = composite_bench.PARSER.parse_args([])
    assert (o.B, o.V, o.S, o.n_ref, o.precision, o.rounds, o.reps) == (32, 32, 128, [9, 32], ["bf16", "bf16x3"], 7, 10)
    o = composite_bench.PARSER.parse_args("4 12 64 --n-ref 16 --precision fp32 --rounds 3".split())
    assert (o.B, o.V, o.S, o.n_ref, o.precision, o.rounds) == (4, 12, 64, [16], ["fp32"], 3)
    with pytest.raises(SystemExit):
        composite_bench.PARSER.parse_args(["4", "12"])
    px = 32 * 128 * 128
    # 4 B * HW * (n views + n masks + ref + count); with `filled` 4 B * HW * (2 V + V + 2)
    assert composite_bench.floor_us(32, 32, 128, 9, False) == pytest.approx(4 * 20 * px / 6.3e12 * 1e6)
    assert composite_bench.floor_us(32, 32, 128, 32, False) == pytest.approx(4 * 66 * px / 6.3e12 * 1e6)
    assert composite_bench.floor_us(32, 32, 128, 9, True) == composite_bench.floor_us(32, 32, 128, 32, True) == pytest.approx(4 * 98 * px / 6.3e12 * 1e6)
