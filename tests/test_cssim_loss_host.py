"""CPU: what tests/test_gpu_cssim_loss.py relies on, shown without a GPU.

- The restatement.  tests/cssim_grad_ref.grad (fp64 numpy, direct form) against torch fp64 autograd through the direct composition of the
  score at a fixed offset with the bias attached: both windows, clip and the bias on and off, 24 x 24, 30 x 45 and the one-pixel map.
  Bound: 1e-10 of the sample's max |gradient| - fp64 rounding with three digits of margin over the 1.3e-13 the formulas measured.
- The bound.  The float32 model of the kernel's centred algebra (cssim_grad_ref.grad_f32) over the GPU test's cases: its largest error
  per family is what tests/cssim_loss_bounds.py records, and CSSIM_GRAD_TOL is 4 x the largest, rounded up to one digit.  The uncentred
  form misses that bound on the clear frames, which is why the kernel centres.
- The gaps.  On every case the restatement's best offset leads the runner-up by >= cssim_cases.PIN_GAP, so k* can be compared.
- The controls.  Each wrong variant of the restatement moves the gradient of a listed case by >= 10 x CSSIM_GRAD_TOL.
- The host side of the new surface: the wrapper's argument checks, the ABI table, the C entry point's refusals, the ops on the meta
  device, the tools' command lines."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

import cssim_cases as C
import cssim_grad_ref as G
import cssim_ref as R
from cssim_loss_bounds import CSSIM_GRAD_MODEL, CSSIM_GRAD_TOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE = {c[0]: c for c in G.CASES}


# ----------------------------------------------------------------------------- the restatement against autograd
@pytest.mark.parametrize("window", ["gaussian", "uniform"])
@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("correct_bias", [True, False])
def test_restatement_matches_fp64_autograd(window, clip, correct_bias):
    T = R.TAPS[window]
    for H, W, border in ((24, 24, 3), (30, 45, 3), (6 + T, 6 + T, 3), (T, T, 0)):
        # the clear frame sits at 0.9: moved to 0.95 it is clamped at 1 in places, the scene with holes at both ends
        for make, move in ((R.scene, 0.1), (lambda seed, H, W: R.scene_clear(seed, H, W, 0.9, 0.05, "blob"), 0.22)):
            sr, hr, mp = make(7 * H + W, H, W)
            if clip:
                sr = (np.float32(1.3) * sr - np.float32(move)).astype(np.float32)
                assert H < 24 or ((sr > 1).any() and (sr < 1).any())
            k = R.shift_cssim(sr, hr, mp, border, window, clip, correct_bias)[1]
            for kk in {k, 0}:                                     # the selected offset and a corner of the search
                want = G.grad_autograd(sr, hr, mp, kk, border, window, clip, correct_bias)
                got = G.grad(sr, hr, mp, kk, border, window, clip, correct_bias)
                assert np.abs(want).max() > 0
                err = G.rel_err(got, want)
                print(f"cssim gradient restatement {H}x{W} {window} clip {clip} bias {correct_bias} k {kk}: {err:.2e} of the max-norm")
                assert err <= 1e-10
                assert not got[:border].any() and not got[:, :border].any() and got.shape == (H, W)


def test_restatement_of_a_sample_without_an_offset_is_zero():
    sr, hr, mp = R.scene(3, 24, 24)
    assert not G.grad(sr, hr, np.zeros_like(mp), -1).any()


def test_the_mean_term_is_visible_only_with_holes():
    """M (the bias attached) is 3e-3 .. 1e-2 of the max-norm on the scenes with holes and about 1e-6 on clear frames"""
    sr, hr, mp = R.scene(17 * 24 + 24, 24, 24)
    k = R.shift_cssim(sr, hr, mp, 3, clip=False)[1]
    moved = G.rel_err(G.grad(sr, hr, mp, k, control="bias_detached"), G.grad(sr, hr, mp, k))
    assert 1e-3 <= moved <= 5e-2
    sr, hr, mp = R.scene_clear(5, 24, 24, 0.9, 0.05, "clear")
    k = R.shift_cssim(sr, hr, mp, 3, clip=False)[1]
    assert G.rel_err(G.grad(sr, hr, mp, k, control="bias_detached"), G.grad(sr, hr, mp, k)) <= 1e-4


# ----------------------------------------------------------------------------- the cases, the gaps, the model and the bound
def test_the_cases_are_the_ones_named():
    src = open(os.path.join(ROOT, "highres-net_amd", "hrnet_hip", "csrc", "cssim_bwd.hip")).read()
    import re
    const = lambda name: int(re.search(rf"constexpr int {name} = (\d+);", src).group(1))
    assert (const("CB_OR"), const("CB_WIN"), const("CB_RUN")) == (G.OR, G.WIN, G.RUN) and G.OC == {"gaussian": 44, "uniform": 52}
    assert set(G.FAMILIES) == {c[1] for c in G.CASES} == set(CSSIM_GRAD_MODEL) and len(CASE) == len(G.CASES)
    shape = lambda cid: G.case_input(CASE[cid])[0].shape
    for window, T in R.TAPS.items():
        assert shape(f"one-pixel-map-{window}")[1:] == (6 + T, 6 + T)
        assert shape(f"tile+1-{window}")[1:] == (G.OR + 1 + 6, G.OC[window] + 1 + 6)
        assert shape(f"two-tiles+1-{window}-holes")[1:] == shape(f"two-tiles+1-{window}-clear")[1:] == (2 * G.OR + 1 + 6, 2 * G.OC[window] + 1 + 6)
        assert shape(f"holes-24x24-{window}") == (2, 24, 24) and shape(f"holes-49x71-{window}") == (1, 49, 71)
        assert CASE[f"border0-{window}"][3] == 0 and CASE[f"border8-{window}"][3] == 8
        s = G.case_input(CASE[f"clip-{window}"])[0]
        assert (s > 1).any() and (s < 0).any()                      # pixels clamped at both ends
    cond = [c for c in G.CASES if c[1] == "conditioning"]
    assert len(cond) == 40 and {c[0] for c in cond} == {c[0] for c in C.PIN_CASES if c[1] == "conditioning"}


@pytest.mark.parametrize("case", G.CASES, ids=[c[0] for c in G.CASES])
def test_the_best_offset_leads_by_the_gap(case):
    (scores, k, _, _), grads = G.case_ref(case)
    for b in range(len(k)):
        assert k[b] >= 0 and R.gap(scores[b]) >= C.PIN_GAP, (case[0], b, R.gap(scores[b]), "replace the seed")
        assert np.isfinite(grads[b]).all() and np.abs(grads[b]).max() > 0


def _model_errors(form):
    worst = {}
    for case in G.CASES:
        cid, family, _, border, window, opt = case
        x = G.case_input(case)
        kw = dict(clip=opt.get("clip", False), correct_bias=opt.get("correct_bias", True))
        (_, k, bias, n), grads = G.case_ref(case)
        for b in range(len(k)):
            got = G.grad_f32(x[0][b], x[1][b], x[2][b], k[b], bias[b, k[b]], n[b, k[b]], border, window, form=form, **kw)
            e = G.rel_err(got, grads[b])
            if e > worst.get(family, (0.0, None))[0]:
                worst[family] = (e, f"{cid}[{b}]")
    return worst


def test_the_bound_is_four_times_the_centred_models_largest_error():
    worst = _model_errors("centred")
    for f, (e, where) in worst.items():
        print(f"cssim gradient float32 model, {f}: {e:.2e} of the max-norm at {where} (recorded {CSSIM_GRAD_MODEL[f]:.1e})")
        assert CSSIM_GRAD_MODEL[f] / 4 <= e <= CSSIM_GRAD_MODEL[f], (f, e)
    top = 4 * max(CSSIM_GRAD_MODEL.values())
    digit = 10.0 ** math.floor(math.log10(top))
    assert CSSIM_GRAD_TOL == pytest.approx(math.ceil(top / digit - 1e-9) * digit, rel=1e-12) and CSSIM_GRAD_TOL >= top


def test_the_uncentred_model_misses_the_bound_on_clear_frames():
    worst = _model_errors("uncentred")
    print("cssim gradient float32 model, uncentred: " + ", ".join(f"{f} {e:.2e} at {w}" for f, (e, w) in worst.items()))
    assert worst["conditioning"][0] > 10 * CSSIM_GRAD_TOL and worst["shapes"][0] > 10 * CSSIM_GRAD_TOL


# ----------------------------------------------------------------------------- the controls
CONTROL_CASES = [("bias_detached", "holes-24x24-gaussian"), ("bias_detached", "two-tiles+1-uniform-holes"),
                 ("adjoint_tap_dropped", "holes-49x71-gaussian"), ("adjoint_tap_dropped", "cond-24x24-uniform-L0.9-c0.05-clear"),
                 ("adjoint_valid", "holes-49x71-uniform"), ("adjoint_valid", "two-tiles+1-gaussian-clear"),
                 ("cov_norm_left_out", "holes-24x24-uniform"), ("cov_norm_left_out", "cond-49x71-uniform-L0.9-c0.05-edge"),
                 ("neighbouring_offset", "tile+1-gaussian"), ("neighbouring_offset", "cond-24x24-gaussian-L0.9-c0.005-clear"),
                 ("pass_ignored", "clip-gaussian"), ("pass_ignored", "clip-no-bias-uniform")]


@pytest.mark.parametrize("control,cid", CONTROL_CASES)
def test_a_control_moves_the_gradient_by_ten_bounds(control, cid):
    case = CASE[cid]
    _, _, _, border, window, opt = case
    x = G.case_input(case)
    kw = dict(clip=opt.get("clip", False), correct_bias=opt.get("correct_bias", True))
    (_, k, _, _), grads = G.case_ref(case)
    for b in range(len(k)):
        ratio = G.rel_err(G.grad(x[0][b], x[1][b], x[2][b], k[b], border, window, control=control, **kw), grads[b]) / CSSIM_GRAD_TOL
        print(f"cssim gradient control {control} on {cid}[{b}]: moves the gradient by {ratio:.1f} x the bound")
        assert ratio >= 10.0, (control, cid, b, ratio)


def test_every_control_is_shown():
    assert {c for c, _ in CONTROL_CASES} == set(G.CONTROLS)
    assert all(CASE[cid][4] == "uniform" for c, cid in CONTROL_CASES if c == "cov_norm_left_out")


# ----------------------------------------------------------------------------- the new surface, host side
NAMES = ("hrn_cssim_loss_backward_workspace_bytes", "hrn_cssim_loss_backward")


@pytest.fixture(scope="module")
def lib():
    from hrnet_hip import binding, build
    if not os.path.exists(binding.LIB_PATH):
        build.build_library(verbose=False)
    return binding.load_library()


def test_exports_are_present(lib):
    from hrnet_hip import binding, build, losses
    header = open(os.path.join(ROOT, "include", "hrnet_hip.h")).read()
    for n in NAMES:
        assert n in binding.SIGNATURES and hasattr(lib, n) and n + "(" in header, n
    assert "cssim_bwd.hip" in build.SOURCES
    assert callable(losses.cssim_loss) and callable(binding.cssim_loss_backward)
    assert hasattr(torch.ops.hrnet_hip, "shift_cssim_train") and hasattr(torch.ops.hrnet_hip, "cssim_loss_backward")


def test_c_entry_point_refuses_bad_arguments_before_any_launch(lib):
    null, p = ctypes.c_void_p(0), ctypes.c_void_p(64)          # p: never dereferenced, every call below fails its checks first

    def f(B, H, W, border, window, a=p, data_range=1.0, ws_bytes=1 << 40):
        return lib.hrn_cssim_loss_backward(a, p, p, p, p, B, H, W, border, window, 0, 1, data_range, p, p, ws_bytes, null)

    assert f(2, 24, 24, 3, 0, null) == -2 and b"null" in lib.hrn_last_error()
    assert f(2, 24, 24, 9, 0) == -2 and b"border" in lib.hrn_last_error()
    assert f(2, 24, 24, -1, 0) == -2
    assert f(2, 24, 24, 3, 2) == -2 and b"window" in lib.hrn_last_error()
    assert f(2, 16, 24, 3, 0) == -2 and f(2, 24, 16, 3, 0) == -2 and b"shape" in lib.hrn_last_error()
    assert f(2, 12, 24, 3, 1) == -2 and f(0, 24, 24, 3, 0) == -2
    assert f(65536, 24, 24, 3, 0) == -2 and b"grid" in lib.hrn_last_error()
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert f(2, 24, 24, 3, 0, data_range=bad) == -2 and b"data_range" in lib.hrn_last_error()
    assert f(2, 24, 24, 3, 0, ws_bytes=8) == -3
    ws = lib.hrn_cssim_loss_backward_workspace_bytes
    assert ws(2, 24, 24, 9, 0) == 0 and ws(2, 16, 24, 3, 0) == 0 and ws(0, 24, 24, 3, 0) == 0 and ws(2, 24, 24, 3, 2) == 0
    assert ws(2, 13, 13, 3, 1) > 0 and ws(2, 13, 13, 3, 0) == 0
    # per sample: four waves' sums per tile of 16 x 44 (16 x 52) crop pixels, and the mean
    assert ws(1, 24, 24, 3, 0) == (2 * 4 + 1) * 8 and ws(3, 24, 24, 3, 0) == 3 * (2 * 4 + 1) * 8 and ws(1, 19, 19, 3, 1) == (4 + 1) * 8
    assert ws(1, 17 + 6, 45 + 6, 3, 0) == (4 * 4 + 1) * 8 and ws(1, 17 + 6, 53 + 6, 3, 1) == (4 * 4 + 1) * 8


def test_python_argument_errors():
    from hrnet_hip import losses
    a = torch.zeros(2, 24, 24)
    with pytest.raises(TypeError, match="torch.Tensor"):
        losses.cssim_loss(a.numpy(), a, a)
    with pytest.raises(ValueError, match="equal"):
        losses.cssim_loss(a, a[:, :20], a)
    with pytest.raises(ValueError, match="equal"):
        losses.cssim_loss(torch.zeros(2, 2, 24, 24), a, a)
    for border_w in (9, -1):
        with pytest.raises(ValueError, match="border_w must be 0..8"):
            losses.cssim_loss(torch.zeros(2, 40, 40), torch.zeros(2, 40, 40), torch.zeros(2, 40, 40), border_w=border_w)
    with pytest.raises(ValueError, match=r"at least 2 border_w \+ 11"):
        losses.cssim_loss(torch.zeros(2, 24, 16), torch.zeros(2, 24, 16), torch.zeros(2, 24, 16), border_w=3)
    with pytest.raises(ValueError, match=r"at least 2 border_w \+ 7"):
        losses.cssim_loss(torch.zeros(2, 12, 24), torch.zeros(2, 12, 24), torch.zeros(2, 12, 24), window="uniform")
    with pytest.raises(ValueError, match="window must be one of"):
        losses.cssim_loss(a, a, a, window="hann")
    with pytest.raises(ValueError, match="data_range"):
        losses.cssim_loss(a, a, a, data_range=0.0)
    with pytest.raises(TypeError, match="no CPU fallback"):
        losses.cssim_loss(a, a, a)
    with pytest.raises(TypeError, match="no CPU fallback"):
        losses.cssim_loss(a.clone().requires_grad_(True), a, a)
    # shift_cssim's own messages, word for word
    for args, kw in (((a, a, a), dict(window="hann")), ((a, a[:, :20], a), {}), ((a, a, a), dict(border_w=7)), ((a, a, a), {})):
        with pytest.raises((TypeError, ValueError)) as e1:
            losses.shift_cssim(*args, **kw)
        with pytest.raises((TypeError, ValueError)) as e2:
            losses.cssim_loss(*args, **kw)
        assert type(e1.value) is type(e2.value) and str(e1.value) == str(e2.value)


def test_ops_infer_shapes_on_the_meta_device():
    a = torch.zeros(3, 30, 41, device="meta")
    out, stats = torch.ops.hrnet_hip.shift_cssim_train(a, a, a, 2, "uniform", False, True, 1.0)
    assert (out.shape, out.dtype) == ((3,), torch.float32) and (stats.shape, stats.dtype) == ((3, 4), torch.float64)
    d = torch.ops.hrnet_hip.cssim_loss_backward(a, a, a, stats, out, 2, "uniform", False, True, 1.0)
    assert (d.shape, d.dtype, d.device.type) == ((3, 30, 41), torch.float32, "meta")


def test_tools_command_lines():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import cssim_bench
    import train_step_bench
    o = vars(train_step_bench.options("32 32 64 10 --precision bf16 --loss shift,cssim --repeats 3".split()))
    assert o["loss"] == ["shift", "cssim"] and o["repeats"] == 3 and o["steps"] == 10
    assert vars(train_step_bench.options("8 4 16 2 --loss cssim".split()))["loss"] == ["cssim"]      # no ShiftNet: its window does not apply
    with pytest.raises(SystemExit):
        train_step_bench.options("--loss l2".split())
    o = cssim_bench.CLI.parse_args("8 --sizes 96 --backward --windows uniform".split())
    assert o.backward and (o.B, o.sizes, o.windows) == (8, [96], ["uniform"])
    assert vars(cssim_bench.CLI.parse_args([])) == dict(vars(cssim_bench.PARSER.parse_args([])), backward=False)
    assert cssim_bench.BWD_FAMILIES == ("cssim_bwd_tile", "cssim_bwd_finish")
    # the tool's torch composition of the selected offset is the definition: its autograd against the restatement, fp32 against fp64
    sr, hr, mp = R.scene(3, 26, 31)
    for window in ("gaussian", "uniform"):
        k = R.shift_cssim(sr, hr, mp, 2, window, clip=False)[1]
        taps, cov = cssim_bench.taps_of(window, "cpu")
        s = torch.from_numpy(sr)[None].requires_grad_(True)
        score = cssim_bench.torch_cssim_at(s, torch.from_numpy(hr)[None], torch.from_numpy(mp)[None], torch.tensor([k]), 2, taps, cov)
        score.sum().backward()
        assert G.rel_err(s.grad[0].numpy(), G.grad(sr, hr, mp, k, 2, window)) <= 1e-3
