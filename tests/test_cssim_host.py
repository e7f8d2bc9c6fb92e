"""CPU: the restatement of the shift-searched SSIM (tests/cssim_ref.py) against an independent evaluation and against known properties,
and the host side of the new surface: exports, the argument checks of the C entry point (nothing is launched) and of
hrnet_hip.losses.shift_cssim, the op's shape inference, the bench tool's command line, and the two switches of hrnet_hip.validate."""
import ctypes
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

import cssim_ref as R
import util
from util import _free_port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("window", ["gaussian", "uniform"])
def test_restatement_matches_scipy(window):
    """correlate1d along each axis, cropped to the positions where the window fits, and the SSIM formula written out once more"""
    ndimage = pytest.importorskip("scipy.ndimage")
    sr, hr, mp = R.scene(5, 31, 38)
    border, nb = 2, 5
    taps, cov = R.window(window)
    T = len(taps)
    h, w = 31 - 2 * border, 38 - 2 * border
    s = np.clip(sr[border:border + h, border:border + w].astype(np.float64), 0, 1)

    def G(a):
        full = ndimage.correlate1d(ndimage.correlate1d(a, taps, axis=0, mode="constant"), taps, axis=1, mode="constant")
        return full[T // 2:T // 2 + h - T + 1, T // 2:T // 2 + w - T + 1]

    scores, k, bias, n = R.shift_cssim(sr, hr, mp, border, window)
    for u in range(nb):
        for v in range(nb):
            g, m = hr[u:u + h, v:v + w].astype(np.float64), (mp[u:u + h, v:v + w] != 0).astype(np.float64)
            b = (m * (g - s)).sum() / m.sum()
            X, Y = m * g, m * (s + b)
            mx, my = G(X), G(Y)
            vx, vy, vxy = cov * (G(X * X) - mx ** 2), cov * (G(Y * Y) - my ** 2), cov * (G(X * Y) - mx * my)
            want = (((2 * mx * my + 1e-4) * (2 * vxy + 9e-4)) / ((mx ** 2 + my ** 2 + 1e-4) * (vx + vy + 9e-4))).mean()
            assert abs(scores[u * nb + v] - want) <= 1e-12 and abs(bias[u * nb + v] - b) <= 1e-15
    assert k == int(np.argmax(scores))


def test_windows_are_the_stated_ones():
    g, cov = R.window("gaussian")
    assert len(g) == 11 and cov == 1.0 and abs(g.sum() - 1) < 1e-7 and np.array_equal(g, g[::-1]) and np.array_equal(g, g.astype(np.float32))
    assert abs(g[5] / g[4] - np.exp(1 / 4.5)) < 1e-6
    u, cov = R.window("uniform")
    assert len(u) == 7 and cov == 49.0 / 48.0 and np.all(u == 1.0 / 7.0)


@pytest.mark.parametrize("window", ["gaussian", "uniform"])
def test_identical_images_score_one_at_the_centre(window):
    _, hr, _ = R.scene(9, 28, 33)
    scores, k, bias, n = R.shift_cssim(hr, hr, np.ones_like(hr), 3, window)
    assert k == 24 and abs(scores[24] - 1.0) <= 1e-12 and abs(bias[24]) <= 1e-15 and n[24] == 22 * 27
    assert np.all(scores[np.arange(49) != 24] < 1.0 - 1e-3)


def test_an_offset_without_a_clear_pixel_scores_minus_infinity_and_is_never_selected():
    sr, hr, mp = R.scene(11, 30, 30)
    mp[:] = 0.0
    mp[:3, :3] = 1.0                            # inside the crop only at offsets u, v <= 2
    scores, k, _, n = R.shift_cssim(sr, hr, mp, 3)
    u, v = np.divmod(np.arange(49), 7)
    assert np.array_equal(n > 0, (u <= 2) & (v <= 2)) and np.array_equal(np.isneginf(scores), n == 0)
    assert n[k] > 0
    mp[:] = 0.0
    scores, k, _, n = R.shift_cssim(sr, hr, mp, 3)
    assert k == -1 and np.isneginf(scores).all()


def test_the_first_maximum_is_selected_and_a_nan_never():
    # a constant target under a full mask: the bias removes every difference, all offsets score exactly alike, the first one wins
    hr = np.full((26, 26), 0.5, np.float32)
    sr = np.full((26, 26), 0.25, np.float32)
    scores, k, bias, _ = R.shift_cssim(sr, hr, np.ones_like(hr), 2)
    assert np.all(scores == scores[0]) and k == 0 and np.all(bias == 0.25)
    sr[13, 13] = np.nan
    scores, k, _, _ = R.shift_cssim(sr, hr, np.ones_like(hr), 2)
    assert np.isnan(scores).all() and k == -1


def test_switches_of_the_restatement():
    sr, hr, mp = R.scene(13, 24, 30)
    sr = sr + 0.7
    a = R.shift_cssim(sr, hr, mp, 1, clip=True)[0]
    b = R.shift_cssim(sr, hr, mp, 1, clip=False)[0]
    c = R.shift_cssim(sr, hr, mp, 1, clip=False, correct_bias=False)
    d = R.shift_cssim(sr, hr, mp, 1, clip=False, data_range=2.0)[0]
    assert np.abs(a - b).max() > 1e-3 and np.abs(b - c[0]).max() > 1e-3 and np.abs(b - d).max() > 1e-4 and np.all(c[2] == 0)


# ----------------------------------------------------------------------------- the new surface, host side
NAMES = ("hrn_shift_cssim_workspace_bytes", "hrn_shift_cssim")


@pytest.fixture(scope="module")
def lib():
    from hrnet_hip import binding, build
    if not os.path.exists(binding.LIB_PATH):
        build.build_library(verbose=False)
    return binding.load_library()


def test_exports_are_present(lib):
    from hrnet_hip import binding, build, losses, validate
    header = open(os.path.join(ROOT, "include", "hrnet_hip.h")).read()
    for n in NAMES:
        assert n in binding.SIGNATURES and hasattr(lib, n) and n + "(" in header, n
    assert "cssim.hip" in build.SOURCES
    assert callable(losses.shift_cssim) and callable(binding.shift_cssim) and hasattr(torch.ops.hrnet_hip, "shift_cssim")
    assert validate.EvaluationCssim._fields == ("names", "cpsnr", "score", "cssim") and validate.Evaluation._fields == ("names", "cpsnr", "score")


def test_c_entry_point_refuses_bad_arguments_before_any_launch(lib):
    null, p = ctypes.c_void_p(0), ctypes.c_void_p(64)          # p: never dereferenced, every call below fails its checks first

    def f(B, H, W, border, window, a=p, data_range=1.0, ws_bytes=1 << 40, scores=p):
        return lib.hrn_shift_cssim(a, p, p, B, H, W, border, window, 1, 1, data_range, p, p, scores, p, ws_bytes, null)

    assert f(2, 24, 24, 3, 0, null) == -2 and b"null" in lib.hrn_last_error()
    assert f(2, 24, 24, 9, 0) == -2 and b"border" in lib.hrn_last_error()
    assert f(2, 24, 24, -1, 0) == -2
    assert f(2, 24, 24, 3, 2) == -2 and b"window" in lib.hrn_last_error()
    assert f(2, 16, 24, 3, 0) == -2 and f(2, 24, 16, 3, 0) == -2 and b"shape" in lib.hrn_last_error()       # a side below 2 border + 11
    assert f(2, 12, 24, 3, 1) == -2                                                                           # ... below 2 border + 7
    assert f(0, 24, 24, 3, 0) == -2
    assert f(65536, 24, 24, 3, 0) == -2 and b"grid" in lib.hrn_last_error()
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert f(2, 24, 24, 3, 0, data_range=bad) == -2 and b"data_range" in lib.hrn_last_error()
    assert f(2, 24, 24, 3, 0, ws_bytes=8) == -3
    ws = lib.hrn_shift_cssim_workspace_bytes
    assert ws(2, 24, 24, 9, 0) == 0 and ws(2, 16, 24, 3, 0) == 0 and ws(0, 24, 24, 3, 0) == 0 and ws(2, 24, 24, 3, 2) == 0
    assert ws(2, 17, 17, 3, 0) > 0 and ws(2, 13, 13, 3, 1) > 0 and ws(2, 13, 13, 3, 0) == 0
    assert ws(1, 4608, 6144, 3, 0) >= ws(1, 384, 384, 3, 0) >= ws(1, 24, 24, 3, 0)
    assert ws(4, 96, 96, 0, 0) == 4 * ws(1, 96, 96, 0, 0)


def test_python_argument_errors():
    from hrnet_hip import losses
    a = torch.zeros(2, 24, 24)
    with pytest.raises(TypeError, match="torch.Tensor"):
        losses.shift_cssim(a.numpy(), a, a)
    with pytest.raises(ValueError, match="equal"):
        losses.shift_cssim(a, a[:, :20], a)
    with pytest.raises(ValueError, match="equal"):
        losses.shift_cssim(torch.zeros(2, 2, 24, 24), a, a)
    with pytest.raises(ValueError, match="border_w"):
        losses.shift_cssim(torch.zeros(2, 40, 40), torch.zeros(2, 40, 40), torch.zeros(2, 40, 40), border_w=9)
    with pytest.raises(ValueError, match="border_w"):
        losses.shift_cssim(torch.zeros(2, 24, 16), torch.zeros(2, 24, 16), torch.zeros(2, 24, 16), border_w=3)          # 16 < 6 + 11
    with pytest.raises(ValueError, match="border_w"):
        losses.shift_cssim(torch.zeros(2, 12, 24), torch.zeros(2, 12, 24), torch.zeros(2, 12, 24), window="uniform")    # 12 < 6 + 7
    with pytest.raises(ValueError, match="window"):
        losses.shift_cssim(a, a, a, window="hann")
    for bad in (0.0, -2.0, float("nan")):
        with pytest.raises(ValueError, match="data_range"):
            losses.shift_cssim(a, a, a, data_range=bad)
    with pytest.raises(TypeError, match="no CPU fallback"):
        losses.shift_cssim(a, a, a)


def test_op_infers_shapes_on_the_meta_device():
    a = torch.zeros(3, 30, 41, device="meta")
    out, stats, scores = torch.ops.hrnet_hip.shift_cssim(a, a, a, 2, "uniform", True, True, 1.0)
    assert (out.shape, out.dtype) == ((3,), torch.float32) and (stats.shape, stats.dtype) == ((3, 4), torch.float64)
    assert (scores.shape, scores.dtype) == ((3, 25), torch.float64) and out.device.type == "meta"


def test_bench_tool_command_line():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import cssim_bench
    o = vars(cssim_bench.PARSER.parse_args([]))
    assert o == dict(B=32, sizes=[192, 384], border=3, windows=["gaussian", "uniform"], rounds=5, reps=10, torch_reps=2)
    o = vars(cssim_bench.PARSER.parse_args("8 --sizes 96 --windows uniform --rounds 3".split()))
    assert (o["B"], o["sizes"], o["windows"], o["rounds"]) == (8, [96], ["uniform"], 3)
    # its torch composition is the definition: against the restatement, fp32 against fp64
    sr, hr, mp = R.scene(3, 26, 31)
    for window in ("gaussian", "uniform"):
        taps, cov = cssim_bench.taps_of(window, "cpu")
        got = cssim_bench.torch_cssim(*(torch.from_numpy(x)[None] for x in (sr, hr, mp)), 2, taps, cov)[0].double().numpy()
        assert np.abs(got - R.shift_cssim(sr, hr, mp, 2, window)[0]).max() <= 2e-5


# ----------------------------------------------------------------------------- validate: the two switches
class _Toy(torch.nn.Module):
    def forward(self, lrs, alphas):
        return torch.nn.functional.interpolate(lrs[:, :1], scale_factor=3, mode="bicubic", align_corners=False)


def _sets(n):
    g = torch.Generator().manual_seed(3)
    return [(torch.rand(1, 3, 16, 16, generator=g), torch.ones(1, 3), torch.rand(1, 48, 48, generator=g),
             (torch.rand(1, 48, 48, generator=g) > 0.1).float(), [f"imgset{i:04d}"]) for i in range(n)]


def test_baseline_table_with_cssim_is_refused():
    from hrnet_hip import validate
    score = lambda s, h, m: torch.ones(s.shape[0])
    with pytest.raises(ValueError, match="cSSIM"):
        validate.sharded_val_score(_Toy(), _sets(2), score_fn=score, baseline_cpsnrs={"imgset0000": 50.0, "imgset0001": 50.0}, metric="cSSIM")
    with pytest.raises(ValueError, match="metric"):
        validate.sharded_val_score(_Toy(), _sets(2), score_fn=score, metric="SSIM")
    # the stub's mean comes back as it is for cSSIM, negated for cPSNR, as ever
    assert validate.sharded_val_score(_Toy(), _sets(2), score_fn=score, metric="cSSIM") == 1.0
    assert validate.sharded_val_score(_Toy(), _sets(2), score_fn=score) == -1.0
    assert type(validate.evaluate(_Toy(), _sets(2), score_fn=score)).__name__ == "Evaluation"


VAL_WORKER = textwrap.dedent("""
    import os, sys
    sys.path.insert(0, os.path.join(%r, "highres-net_amd"))
    sys.path.insert(0, os.path.join(%r, "tests"))
    import numpy as np, torch
    from hrnet_hip import dist as hdist, validate
    import cssim_ref as R
    rank, local_rank, ws = hdist.init(backend="gloo")
    # CPU stand-ins: a "fusion model" (bicubic x3 of the first view) and the fp64 restatement of cSSIM as the scorer; 5 imagesets of batch
    # size 1, dealt round-robin: rank 0 scores 3, rank 1 scores 2
    class Toy(torch.nn.Module):
        def forward(self, lrs, alphas):
            return torch.nn.functional.interpolate(lrs[:, :1], scale_factor=3, mode="bicubic", align_corners=False)
    def score(srs, hrs, maps):
        out = []
        for s, h, m in zip(srs, hrs, maps):
            sc, k, _, _ = R.shift_cssim(s.numpy(), h.numpy(), m.numpy(), 1)
            out.append(sc[k])
        return torch.tensor(out, dtype=torch.float64)
    g = torch.Generator().manual_seed(3)
    sets = []
    for i in range(5):
        lrs = torch.rand(1, 3, 10, 10, generator=g)
        sets.append((lrs, torch.ones(1, 3), torch.rand(1, 30, 30, generator=g), (torch.rand(1, 30, 30, generator=g) > 0.1).float()))
    model = Toy().train()
    mine = [sets[i] for i in validate.shard_indices(len(sets), rank, ws)]
    got = validate.sharded_val_score(model, mine, score_fn=score, metric="cSSIM")
    assert model.training
    want = float(np.mean([float(score(model(l, a)[:, 0], h, m)[0]) for l, a, h, m in sets]))
    assert abs(got - want) <= 1e-12 * abs(want), (got, want)
    hdist.barrier()
    if rank == 0:
        print("val cssim ok", got)
    hdist.finalize()
""") % (ROOT, ROOT)


def test_two_rank_sharded_cssim(tmp_path):
    """sharded_val_score(metric="cSSIM") over two gloo ranks: one all-reduce of (sum, count), the mean over all ranks' samples, not
    negated.  CPU stand-ins for the model and for hrn_shift_cssim (its restatement)."""
    script = tmp_path / "val_worker.py"
    script.write_text(VAL_WORKER)
    port = _free_port()
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    outs = [p.communicate(timeout=180) for p in procs]
    for p, (o, e) in zip(procs, outs):
        assert p.returncode == 0, e[-2000:]
    assert "val cssim ok" in outs[0][0]
