"""CPU: the bicubic upsampler's definition and plumbing.  The fp64 restatement (tests/upsample_ref.py) against torch's CPU bicubic, forward
and adjoint; the rows of its matrices; <up f, g> = <f, up^T g>; the host weight table of hrnet_hip/upsample.py; header, export and
binding of the two entry points and their argument checks (no device is touched: the pointers are never dereferenced); HRNet's
`global_residual` key; the Python argument errors; the norm.csv round trip; the bench tool's byte floors."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import upsample_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1), (2, 5), (5, 7), (16, 19)]
SCALES = [2, 3, 4]
NULL = ctypes.c_void_p(0)


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_restatement_equals_torch_bicubic_forward_and_adjoint(shape, scale):
    rng = np.random.Generator(np.random.PCG64(scale * 100 + shape[0]))
    f = rng.uniform(-1, 1, (2,) + shape)
    g = rng.uniform(-1, 1, (2, scale * shape[0], scale * shape[1]))
    x = torch.from_numpy(f)[None].requires_grad_(True)
    y = torch.nn.functional.interpolate(x, scale_factor=scale, mode="bicubic", align_corners=False)
    (y * torch.from_numpy(g)[None]).sum().backward()
    e_f = np.abs(R.forward(f, scale, -0.75, rounded=False) - y.detach().numpy()[0]).max()
    e_b = np.abs(R.adjoint(g, scale, -0.75, rounded=False) - x.grad.numpy()[0]).max()
    print(f"{shape} x{scale}: forward {e_f:.2e}, adjoint {e_b:.2e}")
    assert e_f <= 1e-12 and e_b <= 1e-12


@pytest.mark.parametrize("a", [-0.75, -0.5])
def test_every_row_sums_to_one(a):
    for scale in SCALES:
        for n in (1, 2, 3, 5, 16, 19):
            assert np.abs(R.axis_matrix(n, scale, a, rounded=False).sum(1) - 1).max() <= 1e-14
        _, w = R.phase_weights(scale, a, rounded=False)
        assert np.abs(w.sum(1) - 1).max() <= 1e-14


@pytest.mark.parametrize("scale", SCALES)
def test_adjoint_identity(scale):
    rng = np.random.Generator(np.random.PCG64(7 + scale))
    for H, W in SHAPES:
        f, g = rng.uniform(-1, 1, (H, W)), rng.uniform(-1, 1, (scale * H, scale * W))
        lhs, rhs = float((R.forward(f, scale) * g).sum()), float((f * R.adjoint(g, scale)).sum())
        assert abs(lhs - rhs) <= 1e-12 * float((R.t_forward(f, scale) * np.abs(g)).sum())


@pytest.mark.parametrize("a", [-0.75, -0.5, -1.0, 0.375])       # fp32 values: `a` crosses the C ABI as a float
def test_host_weight_table_is_the_restatement_rounded_to_fp32(a):
    from hrnet_hip import upsample
    for scale in SCALES:
        shift, w = upsample.phase_weights(scale, a)
        i, want = R.phase_weights(scale, a, rounded=False)
        assert w.dtype == np.float32 and w.shape == (scale, 4) and np.array_equal(shift, i)
        assert np.array_equal(w, want.astype(np.float32))
        assert np.array_equal(w.astype(np.float64), R.phase_weights(scale, a, rounded=True)[1])
        assert list(shift) == [-1 if 2 * p + 1 < scale else 0 for p in range(scale)]       # the kernels' phase_shift
    with pytest.raises(ValueError, match="2, 3 or 4"):
        upsample.phase_weights(5)
    with pytest.raises(ValueError, match="finite"):
        upsample.phase_weights(3, float("nan"))


@pytest.fixture(scope="module")
def lib():
    from hrnet_hip import binding, build
    if not os.path.exists(binding.LIB_PATH):
        build.build_library(verbose=False)
    return binding.load_library()


def test_header_exports_signatures_and_sources_agree(lib):
    from hrnet_hip import binding, build
    assert "upsample.hip" in build.SOURCES
    raw = open(os.path.join(ROOT, "include", "hrnet_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", raw, flags=re.S)
    kinds = {"int64_t": ctypes.c_int64, "int": ctypes.c_int, "float": ctypes.c_float}
    for name in ("hrn_upsample", "hrn_upsample_backward"):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared in include/hrnet_hip.h"
        assert name in binding.SIGNATURES and hasattr(lib, name), name
        res, args = binding.SIGNATURES[name]
        params = [p.strip() for p in m.group(1).split(",")]
        assert res is ctypes.c_int and len(params) == len(args), name
        for decl, ct in zip(params, args):
            assert ct is (ctypes.c_void_p if "*" in decl else kinds[decl.split()[0]]), (name, decl, ct)
    tile = tuple(int(re.search(r"#define\s+HRN_UPSAMPLE_TILE_" + k + r"\s+(\d+)", text).group(1)) for k in "HW")
    assert tile == binding.UPSAMPLE_TILE
    assert "INDICES CLAMPED" in raw and "w1(x) = ((a + 2) x - (a + 3)) x^2 + 1" in raw


def test_bad_arguments_fail_before_any_launch(lib):
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.cast(buf, ctypes.c_void_p)
    far = ctypes.c_void_p(p.value + (1 << 30))                  # never dereferenced
    def fwd(frames=p, base=NULL, out=far, n=1, H=4, W=5, scale=3, a=-0.75):
        return lib.hrn_upsample(frames, base, out, n, H, W, scale, a, NULL)
    def bwd(d_out=far, d_frames=p, n=1, H=4, W=5, scale=3, a=-0.75):
        return lib.hrn_upsample_backward(d_out, d_frames, n, H, W, scale, a, NULL)
    assert fwd(frames=NULL) == -2 and b"null" in lib.hrn_last_error()
    assert fwd(out=NULL) == -2 and b"null" in lib.hrn_last_error()
    assert bwd(d_out=NULL) == -2 and bwd(d_frames=NULL) == -2 and b"null" in lib.hrn_last_error()
    for call in (fwd, bwd):
        for scale in (0, 1, 5, -3):
            assert call(scale=scale) == -2 and b"scale" in lib.hrn_last_error()
        for a in (float("nan"), float("inf"), -float("inf")):
            assert call(a=a) == -2 and b"finite" in lib.hrn_last_error()
        for kw in ({"n": 0}, {"n": -1}, {"H": 0}, {"W": -2}):
            assert call(**kw) == -2 and b"empty" in lib.hrn_last_error()
        assert call(H=16385) == -2 and call(W=1 << 20) == -2 and b"16384" in lib.hrn_last_error()
        assert call(n=1 << 40, H=16384, W=16384) == -2 and b"address space" in lib.hrn_last_error()
    # aliasing: frames inside out; a base that overlaps out without being out; d_frames inside d_out
    assert fwd(out=p) == -2 and b"alias" in lib.hrn_last_error()
    assert fwd(frames=ctypes.c_void_p(far.value + 4 * 9 * 20 - 4)) == -2 and b"alias" in lib.hrn_last_error()
    assert fwd(base=ctypes.c_void_p(far.value + 16)) == -2 and b"base" in lib.hrn_last_error()
    assert bwd(d_out=p) == -2 and b"alias" in lib.hrn_last_error()


def test_global_residual_key_is_parsed():
    import copy
    from DeepNetworks.HRNet import HRNet
    from oracle import weights
    cfg = copy.deepcopy(weights.HRNET_CONFIG)
    m = HRNet(cfg)
    assert m.global_residual is None and m._residual_on() is False
    keys = list(m.state_dict())
    for value, on in ((True, True), (False, False), (None, False)):
        m = HRNet(dict(copy.deepcopy(cfg), global_residual=value))
        assert m.global_residual is value and m._residual_on() is on
        assert list(m.state_dict()) == keys                     # no new parameters
    for bad in ("yes", 1, 0.5, "bicubic"):
        m = HRNet(dict(copy.deepcopy(cfg), global_residual=bad))
        with pytest.raises(ValueError, match="global_residual must be None, False or True"):
            m(torch.zeros(1, 2, 8, 8), torch.ones(1, 2))
    m = HRNet(dict(copy.deepcopy(cfg), global_residual=True)).train()
    with pytest.raises(NotImplementedError, match="ref="):
        m(torch.zeros(1, 2, 8, 8, requires_grad=True), torch.ones(1, 2))


def test_upsample_py_argument_errors():
    from hrnet_hip import upsample
    x = torch.zeros(2, 3, 8, 9)
    with pytest.raises(TypeError, match="frames must be a torch.Tensor"):
        upsample.upsample([[1.0]], 3)
    with pytest.raises(TypeError, match="base must be"):
        upsample.upsample(x, 3, base=1.0)
    for bad in (1, 5, 2.0, True):
        with pytest.raises(ValueError, match="2, 3 or 4"):
            upsample.upsample(x, bad)
    with pytest.raises(TypeError, match="a must be a number"):
        upsample.upsample(x, 3, a="keys")
    with pytest.raises(ValueError, match="a must be finite"):
        upsample.upsample(x, 3, a=float("inf"))
    with pytest.raises(TypeError, match="floating-point"):
        upsample.upsample(x.int(), 3)
    with pytest.raises(ValueError, match=r"\(\.\.\., H, W\)"):
        upsample.upsample(x[0, 0, 0], 3)
    with pytest.raises(ValueError, match="16384 a side"):
        upsample.upsample(torch.zeros(1, 16385, device="meta"), 2)
    with pytest.raises(ValueError, match="base must be"):
        upsample.upsample(x, 3, base=torch.zeros(2, 3, 24, 28))
    with pytest.raises(TypeError, match="ROCm device only"):       # the device comes last: every error above was raised on CPU tensors
        upsample.upsample(x, 3, base=torch.zeros(2, 3, 24, 27))
    with pytest.raises(ValueError, match="names"):
        from hrnet_hip import validate
        validate.baseline_table([(x, torch.ones(2, 3), torch.zeros(2, 24, 27), torch.ones(2, 24, 27), ["only-one"])])


def test_norm_csv_round_trip(tmp_path):
    import utils
    table = {"imgset0000": 45.123456789012345, "imgset0594": 1.0 / 3.0, "imgset1159": 52.0, "x": 1e-300}
    path = tmp_path / "norm.csv"
    utils.writeBaselineCPSNR(str(path), table)
    assert utils.readBaselineCPSNR(str(path)) == table
    assert path.read_text().splitlines()[2] == "imgset1159 52.0"
    with pytest.raises(ValueError, match="without blanks"):
        utils.writeBaselineCPSNR(str(path), {"two words": 1.0})


def test_upsample_bench_command_line_and_byte_floors():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import upsample_bench
    o = upsample_bench.PARSER.parse_args([])
    assert (o.rounds, o.reps, o.skip_forward) == (7, 10, False)
    n, hw = 32, 128 * 128
    assert upsample_bench.floor_us(n, 128, 128, 3, True) == pytest.approx(4 * n * (hw + 18 * hw) / 6.3e12 * 1e6)
    assert upsample_bench.floor_us(n, 128, 128, 3, False) == pytest.approx(4 * n * (hw + 9 * hw) / 6.3e12 * 1e6)
    assert upsample_bench.floor_us(1, 2048, 1536, 3, False) == pytest.approx(4 * 10 * 2048 * 1536 / 6.3e12 * 1e6)
    assert [c[:4] for c in upsample_bench.CASES] == [(32, 128, 128, 2), (32, 128, 128, 3), (32, 128, 128, 4), (1, 2048, 1536, 3)]
