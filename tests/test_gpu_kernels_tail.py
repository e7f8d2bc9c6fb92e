"""GPU (-m gpu): the registered tail - where the loss and the validation score are made - per element, against torch CPU float64.

Every kernel is reached through the public C ABI (the typed table of binding.load_library()), on tensors the test allocates: each output
and workspace lies in a buffer of sentinel bytes with GUARD words in front (the kernel gets an offset pointer) and behind, outputs start as
sentinels, workspaces as NaN; every launch runs twice into fresh buffers and the two must agree bit for bit (lanczos_bwd.hip and losses.hip
both claim determinism); afterwards the sentinels must be intact and the inputs unchanged.  The references, inputs, cases and checks are
those of tests/kernel_refs.py ("the registered tail"), which tests/test_kernels_tail_host.py runs on a float32 restatement on the CPU.

Bounds (tests/kernel_bounds.py).  The fp32 kernels, |got - want| <= c T.  Every case passes with the project's C = 1e-5 and needs at most
1.59e-7 of it on the MI355X, below C / 4, so the family is held to its own c = C_TAIL = 7e-7 (four times the largest measured value; the
per-family values and their cases stand next to it in kernel_bounds.py):
  lanczos_taps_kernel                  T_j = (1 + 7 |k_j|) / |sum u|: t is rounded to fp32 before the sine, an absolute error per u_j
  lanczos_shift_kernel                 c T = c sum |ky||kx||P| + sum [(|ky| + e_y)(|kx| + e_x) - |ky||kx|] |P|, e = c T_j: the sum's own
                                       roundings plus what the taps' errors move it by (P the reflect-padded image)
  lanczos_adjoint_kernel<1>, <0>       the same with |dout|, folded back through the reflection
  lanczos_tapgrad_kernel + lanczos_shiftgrad_finish_kernel
                                       sum_j |dk_j| T(G_j) + T(dk_j) sum |dout||HP|, + |start| (d_shift is accumulated); T(dk_j): ref_tap_grad
  loss_backward_kernel                 |coef| m (|sr| + |hr| + |b|)
The kernels that accumulate in fp64 (masked_cmse_kernel, loss_partial_kernel + loss_finish_kernel, shift_cpsnr_kernel + shift_max_kernel)
have a derived bound without a constant: n 2^-52 T for a double they store, T = (S2 + S1^2 / S0) / S0 for cMSE, carried through
-10 log10 for cPSNR, + 2^-23 |want| for a float.  One dropped pixel fails it at every size.  Where cMSE lies within rounding of zero
(a one-pixel window: cMSE = 0) the results are pinned by class: +inf, or NaN without a clear pixel, as numpy gives them; the gradient of
cPSNR is not determined there (autograd gives NaN) and only the stats are compared.
Exact: d_srs is 0 where the cropped map is; the fourth word of stats is +0.0; two runs agree bit for bit; with d_img or d_shift NULL the
other output is bit-identical.

NaN is pinned to numpy's behaviour: a NaN pixel of SR gives a NaN score with and without `clip` (np.clip keeps NaN), and one NaN
per-offset score makes the maximum NaN (np.max).  Both needed a kernel change, found by reading the code: fminf(fmaxf(s, 0), 1) turns NaN
into 0 (shift_cpsnr_kernel, shift_loss_partial_kernel: now two comparisons, which keep it), and shift_max_kernel's fmax dropped NaN
scores.  Pinned by test_nan_pixel_gives_nan_score, test_nan_score_gives_nan_maximum and test_nan_pixel_gives_nan_searched_loss;
test_shift_cpsnr[3-7-B65-*] needs the second change too: its one-pixel windows without a clear pixel score NaN.  shift_cpsnr is not tested on fractional maps: the kernel documents that it departs from
Evaluator.py's literal formula there.

Measured on the MI355X, error / bound of the fp64 kernels (no constant to fit): cMSE and its float at most 0.53 (S = 3: nine pixels, a
handful of roundings against n 2^-52), the per-offset scores 0.013, their float maximum 0.49 (the float store).  The negative controls
report 5e2 (the frozen tap) .. 3e13 against the wrong reference.  The frozen-tap control freezes the CENTRE tap instead of the t == 0 tap:
at an integer shift that gives the frozen tap its gradient back and takes a live tap's away.  Giving the frozen tap its gradient alone
changes nothing a bound could see - sinc'(1e-6) = -3.3e-7 - which tests/test_kernels_tail_host.py shows.
"""
import ctypes

import numpy as np
import pytest
import torch

import kernel_refs as K
from kernel_bounds import Guarded
from kt import _stream

pytestmark = pytest.mark.gpu

F, D = torch.float32, torch.float64


def _lib():
    from hrnet_hip import binding
    return binding.load_library()


def _ptr(t):
    return None if t is None else (t.ptr if isinstance(t, Guarded) else ctypes.c_void_p(t.data_ptr()))


class Dev:
    """the kernels through the C ABI: CPU float32 tensors in, what the kernels wrote out (CPU; float outputs widened to fp64)"""

    @staticmethod
    def _twice(make, launch, ins):
        """launch(*make()) twice: rc 0, guards intact, bit-identical buffers, inputs unchanged -> the first run's buffers"""
        dev = [t.contiguous().cuda() for t in ins]
        runs = []
        for _ in range(2):
            bufs = make()
            rc = launch(dev, bufs)
            torch.cuda.synchronize()
            assert rc == 0, rc
            assert all(b.guard_ok() for b in bufs if b is not None), "a write outside an output or workspace"
            runs.append(bufs)
        for a, b in zip(*runs):
            assert a is None or torch.equal(a.bits(), b.bits()), "two runs differ"
        assert all(torch.equal(d.cpu().view(torch.uint8), t.contiguous().view(torch.uint8)) for d, t in zip(dev, ins)), "an input was written"
        return runs[0]

    def taps(self, d):
        n = d.numel()
        out, = self._twice(lambda: [Guarded((n, 7))], lambda i, o: _lib().hrn_lanczos_kernel(_ptr(i[0]), n, _ptr(o[0]), _stream()), [d])
        return out.get().double()

    def shift(self, img, shift):
        b, c, H, W = img.shape
        out, = self._twice(lambda: [Guarded(img.shape)],
                           lambda i, o: _lib().hrn_lanczos_shift(_ptr(i[0]), _ptr(i[1]), b, c, H, W, _ptr(o[0]), _stream()), [img, shift])
        return out.get().double()

    def shift_bwd(self, img, shift, dout, start, need_img=True):
        """start: what d_shift holds before (+=), None: d_shift NULL.  The workspace starts as NaN: the NULL side's part is never needed"""
        b, c, H, W = img.shape
        nws = _lib().hrn_lanczos_shift_backward_workspace_bytes(b, c, H, W)
        assert nws % 4 == 0

        def make():
            return [Guarded(img.shape) if need_img else None, None if start is None else Guarded((c, 2), v=start), Guarded((nws // 4,), fill=0xFF)]

        d_img, d_shift, _ = self._twice(make, lambda i, o: _lib().hrn_lanczos_shift_backward(_ptr(i[0]), _ptr(i[1]), _ptr(i[2]), b, c, H, W, _ptr(o[0]),
                                                                                            _ptr(o[1]), _ptr(o[2]), nws, _stream()), [img, shift, dout])
        return None if d_img is None else d_img.get().double(), None if d_shift is None else d_shift.get().double()

    def get_loss(self, srs, hrs, maps, crop, metric):
        B, S, _ = srs.shape
        out, = self._twice(lambda: [Guarded((B,))], lambda i, o: _lib().hrn_get_loss(_ptr(i[0]), _ptr(i[1]), _ptr(i[2]), B, S, crop, metric, _ptr(o[0]),
                                                                                   _stream()), [srs, hrs, maps])
        return out.get().double()

    def loss_train(self, srs, hrs, maps, crop, metric):
        B, S, _ = srs.shape
        nws = _lib().hrn_get_loss_train_workspace_bytes(B)
        assert nws % 8 == 0
        out, stats, _ = self._twice(lambda: [Guarded((B,)), Guarded((B, 4), D), Guarded((nws // 8,), D, fill=0xFF)],
                                    lambda i, o: _lib().hrn_get_loss_train(_ptr(i[0]), _ptr(i[1]), _ptr(i[2]), B, S, crop, metric, _ptr(o[0]), _ptr(o[1]),
                                                                           _ptr(o[2]), nws, _stream()), [srs, hrs, maps])
        return out.get().double(), stats.get()

    def loss_bwd(self, srs, hrs, maps, stats, d_out, crop, metric):
        B, S, _ = srs.shape
        out, = self._twice(lambda: [Guarded(srs.shape)],
                           lambda i, o: _lib().hrn_get_loss_backward(_ptr(i[0]), _ptr(i[1]), _ptr(i[2]), _ptr(i[3]), _ptr(i[4]), B, S, crop, metric,
                                                                     _ptr(o[0]), _stream()), [srs, hrs, maps, stats, d_out])
        return out.get().double()

    def shift_cpsnr(self, srs, hrs, maps, border, clip):
        """-> the workspace's (B, (2 border + 1)^2) per-offset scores, and their maximum"""
        B, S, _ = srs.shape
        nshift = (2 * border + 1) ** 2
        nws = _lib().hrn_shift_cpsnr_workspace_bytes(B, border)
        assert nws == B * nshift * 8
        out, scores = self._twice(lambda: [Guarded((B,)), Guarded((B, nshift), D)],
                                  lambda i, o: _lib().hrn_shift_cpsnr(_ptr(i[0]), _ptr(i[1]), _ptr(i[2]), B, S, border, clip, _ptr(o[0]), _ptr(o[1]), nws,
                                                                      _stream()), [srs, hrs, maps])
        return scores.get(), out.get().double()


DEV = Dev()


# ----------------------------------------------------------------------------------------------------------- Lanczos
@pytest.mark.parametrize("n", K.TAP_N)
def test_taps(n):
    """lanczos_taps_kernel: one block of 64 and its neighbours; shifts on, beside and beyond the integers"""
    K.check_taps(DEV, n)


@pytest.mark.parametrize("b,c", K.LANCZOS_BC, ids=["b1c1", "b2c3"])
@pytest.mark.parametrize("H,W", K.LANCZOS_FWD_SHAPES, ids=[f"{h}x{w}" for h, w in K.LANCZOS_FWD_SHAPES])
def test_lanczos_shift(H, W, b, c):
    """lanczos_shift_kernel: the 4 x 4 minimum (every halo pixel a reflection), one 32 x 128 tile, one pixel and six more than it"""
    K.check_lanczos_fwd(DEV, b, c, H, W)


@pytest.mark.parametrize("b,c", K.LANCZOS_BC, ids=["b1c1", "b2c3"])
@pytest.mark.parametrize("H,W", K.LANCZOS_BWD_SHAPES, ids=[f"{h}x{w}" for h, w in K.LANCZOS_BWD_SHAPES])
def test_lanczos_shift_backward(H, W, b, c):
    """lanczos_tapgrad_kernel + lanczos_shiftgrad_finish_kernel, lanczos_adjoint_kernel<1> + <0>: H = W = 4 (the three terms of the fold on
    the same pixels), one 16 x 64 tile and one pixel more"""
    K.check_lanczos_bwd(DEV, b, c, H, W)


# ----------------------------------------------------------------------------------------------------------- losses
@pytest.mark.parametrize("kind", ["bin", "frac", "zero"])
@pytest.mark.parametrize("B", [1, 3], ids=["B1", "B3"])
@pytest.mark.parametrize("S,crop", [(S, cr) for S in K.LOSS_S for cr in K.crops(S)], ids=lambda v: str(v))
def test_get_loss(S, crop, B, kind):
    """masked_cmse_kernel, metrics 0 / 1 / 2; "zero": sample 0 has no clear pixel - NaN for cMSE / cPSNR, 0 for masked_MSE, as the numpy
    oracle of the reference's formula gives them"""
    K.check_get_loss(DEV, S, crop, B, kind)
    if kind == "zero":
        from oracle import hrnet_np as O
        srs, hrs, maps = (t.numpy() for t in K.loss_inputs(B, S, kind))
        maps = maps * K.crop_mask(S, crop).numpy()
        with np.errstate(all="ignore"):
            want = [O.get_loss(srs, hrs, maps, m)[0] for m in ("masked_MSE", "cMSE", "cPSNR")]
        assert want[0] == 0 and np.isnan(want[1]) and np.isnan(want[2])
        got = [float(DEV.get_loss(*K.loss_inputs(B, S, kind), crop, m)[0]) for m in (0, 1, 2)]
        assert got[0] == 0 and np.isnan(got[1]) and np.isnan(got[2]), got


def test_get_loss_ill_conditioned():
    """sr = hr + 0.2 + 1e-3 noise: S2 ~ S1^2 / S0 to four digits, float accumulators are 1e3 bounds off (the host file shows it)"""
    K.check_get_loss(DEV, 65, 3, 3, "bin", ill=True)


@pytest.mark.parametrize("metric", [1, 2], ids=["cMSE", "cPSNR"])
@pytest.mark.parametrize("B,kind", [(1, "bin"), (1, "frac"), (65, "mixed")], ids=["B1-bin", "B1-frac", "B65-mixed"])
@pytest.mark.parametrize("S,crop", [(S, cr) for S in K.TRAIN_S for cr in K.crops(S)], ids=lambda v: str(v))
def test_get_loss_train_and_backward(S, crop, B, kind, metric):
    """loss_partial_kernel + loss_finish_kernel (B = 65: past its 64-thread block), loss_backward_kernel (S = 129: past its 64-block grid)"""
    K.check_loss_train(DEV, S, crop, B, kind, metric)


# ----------------------------------------------------------------------------------------------------------- the score
@pytest.mark.parametrize("clip", [0, 1], ids=["raw", "clip"])
@pytest.mark.parametrize("B", [1, 65], ids=["B1", "B65"])
@pytest.mark.parametrize("border,S", [(b, S) for b in K.SCORE_BORDERS for S in (2 * b + 1, 23)], ids=lambda v: str(v))
def test_shift_cpsnr(border, S, B, clip):
    """shift_cpsnr_kernel: every per-offset score (they fix the row / column orientation), then shift_max_kernel's maximum.  S = 2 border + 1:
    one-pixel windows, cMSE = 0 and cPSNR = +inf (NaN without a clear pixel), as numpy gives them"""
    K.check_shift_cpsnr(DEV, border, S, B, clip)


@pytest.mark.parametrize("clip", [0, 1], ids=["raw", "clip"])
def test_nan_pixel_gives_nan_score(clip):
    """np.clip keeps NaN: a NaN pixel inside SR's centre crop makes every per-offset score, and the score, NaN - for that sample alone"""
    srs, hrs, maps = K.score_inputs(3, 23, 3)
    srs[1, 11, 9] = float("nan")
    scores, out = DEV.shift_cpsnr(srs, hrs, maps, 3, clip)
    want, bounds = K.ref_shift_scores(srs.double(), hrs.double(), maps.double(), 3, clip)
    assert bool(torch.isnan(want[1]).all()) and bool(torch.isfinite(want[[0, 2]]).all())
    K._assert_within(f"shift_cpsnr NaN pixel clip={clip} scores", scores, want, bounds, "b k")
    K._assert_within(f"shift_cpsnr NaN pixel clip={clip} max", out, *K.ref_score_max(want, bounds), "b")


@pytest.mark.parametrize("corner", ["first", "last"])
def test_nan_score_gives_nan_maximum(corner):
    """np.max: one NaN per-offset score (a NaN pixel of HR that only the first / the last offset's window reaches) makes the maximum NaN"""
    srs, hrs, maps = K.score_inputs(3, 23, 3)
    at = 0 if corner == "first" else 22
    hrs[1, at, at], maps[1, at, at] = float("nan"), 1.0
    scores, out = DEV.shift_cpsnr(srs, hrs, maps, 3, 1)
    want, bounds = K.ref_shift_scores(srs.double(), hrs.double(), maps.double(), 3, 1)
    k = 0 if corner == "first" else 48
    assert bool(torch.isnan(want[1, k])) and int(torch.isnan(want).sum()) == 1
    K._assert_within(f"shift_cpsnr NaN score {corner} scores", scores, want, bounds, "b k")
    wmax, bmax = K.ref_score_max(want, bounds)
    assert bool(torch.isnan(wmax[1])) and bool(torch.isfinite(wmax[[0, 2]]).all())
    K._assert_within(f"shift_cpsnr NaN score {corner} max", out, wmax, bmax, "b")


@pytest.mark.parametrize("clip", [False, True], ids=["raw", "clip"])
def test_nan_pixel_gives_nan_searched_loss(clip):
    """the searched loss clamps like the score: torch.clamp keeps NaN, so the sample's loss is NaN and the other samples' are untouched"""
    from hrnet_hip import binding
    srs, hrs, maps = K.score_inputs(3, 23, 3)
    clean, _ = binding.shift_loss_train(srs.cuda(), hrs.cuda(), maps.cuda(), "cPSNR", 3, clip)
    srs[1, 11, 9] = float("nan")
    out, stats = binding.shift_loss_train(srs.cuda(), hrs.cuda(), maps.cuda(), "cPSNR", 3, clip)
    out, clean = out.cpu(), clean.cpu()
    assert bool(torch.isnan(out[1])) and bool(torch.isnan(stats.cpu()[1, 2])) and torch.equal(out[[0, 2]], clean[[0, 2]]), (out, clean)


# ----------------------------------------------------------------------------------------------------------- negative controls
@pytest.mark.parametrize("control", K.TAIL_CONTROLS)
def test_negative_control(control):
    """The comparison against a reference that is wrong in one way must FAIL on the same GPU output that passes against the right one."""
    ok, worst = K.tail_control(DEV, control)
    print(f"{control}: error / bound against the wrong reference {worst:.3e} (right one {ok:.3e})")
    assert ok <= 1.0 and worst > 1.0, f"{control}: the comparison does not tell the wrong reference from the right one"
