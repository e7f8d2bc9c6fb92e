"""CPU: the fp64 references of tests/test_gpu_kernels_tail.py (the Lanczos shift, its backward, the loss and score kernels) against the
reference's own outputs (tests/golden/lanczos.npz, callers.npz) and the project's two ports (oracle/torch_port.py, oracle/hrnet_np.py); and
every case and negative control of the GPU file run on `F32Model` instead of the GPU: a float32 restatement of each kernel's arithmetic -
float32 operands, float32 sums where the kernel sums in float32, fp64 sums in one pass where it sums in fp64 - with none of the tile loops.
It must stay inside the bounds and every wrong reference outside them: the inputs and bounds are then known to tell the two apart before a
GPU is involved."""
import numpy as np
import pytest
import torch

import kernel_refs as K
import util
from oracle import hrnet_np as O
from oracle import torch_port

D = torch.float64
F = torch.float32


# ----------------------------------------------------------------------------------------------------------- the float32 restatement
class F32Model:
    def taps(self, d, grad=False):
        pi = torch.tensor(np.float32(np.pi))
        t = pi * ((torch.arange(7, dtype=F) - 3)[None, :] - d.reshape(-1, 1))
        t = torch.where(t == 0, torch.tensor(1e-6, dtype=F), t)
        u = torch.sin(t) / t * (torch.sin(t / 3) / (t / 3))
        k = u / u.sum(1, keepdim=True)
        assert k.dtype == F
        return k if grad else k.detach().double()

    def _forward(self, img, shift):
        b, c = img.shape[:2]
        rows = K._plane_rows(b, c)
        return K.shift_with_taps(img, self.taps(shift[:, 0], True)[rows], self.taps(shift[:, 1], True)[rows])

    def shift(self, img, shift):
        out = self._forward(img, shift)
        assert out.dtype == F
        return out.double()

    def shift_bwd(self, img, shift, dout, start, need_img=True):
        """float32 autograd of the float32 forward"""
        img, shift = img.clone().requires_grad_(True), shift.clone().requires_grad_(True)
        (self._forward(img, shift) * dout).sum().backward()
        return img.grad.double() if need_img else None, None if start is None else (start + shift.grad).double()

    @staticmethod
    def _sums(srs, hrs, maps, crop):
        """S0, S1, S2 in one pass, fp64 accumulators on float32 operands"""
        m = maps.double() * K.crop_mask(srs.shape[-1], crop)
        d = srs.double() - hrs.double()
        return m, d, m.sum((1, 2)), (m * d).sum((1, 2)), (m * d * d).sum((1, 2))

    def get_loss(self, srs, hrs, maps, crop, metric):
        m, d, s0, s1, s2 = self._sums(srs, hrs, maps, crop)
        if metric == 0:
            return ((m * d) ** 2).sum((1, 2)).div(d[0].numel()).float().double()
        cmse = (s2 - s1 * s1 / s0) / s0
        return (cmse if metric == 1 else -10 * torch.log10(cmse)).float().double()

    def loss_train(self, srs, hrs, maps, crop, metric):
        _, _, s0, s1, s2 = self._sums(srs, hrs, maps, crop)
        cmse = (s2 - s1 * s1 / s0) / s0
        return ((cmse if metric == 1 else -10 * torch.log10(cmse)).float().double(), torch.stack([s0, -s1 / s0, cmse, torch.zeros_like(s0)], 1))

    def loss_bwd(self, srs, hrs, maps, stats, d_out, crop, metric):
        dm = torch.ones_like(stats[:, 2]) if metric == 1 else -10.0 / (np.log(10.0) * stats[:, 2])
        coef = (d_out.double() * dm * 2 / stats[:, 0]).float()[:, None, None]
        m = maps * K.crop_mask(srs.shape[-1], crop).float()
        out = coef * m * (srs - hrs + stats[:, 1].float()[:, None, None])
        assert out.dtype == F
        return out.double()

    def shift_cpsnr(self, srs, hrs, maps, border, clip):
        B, S, _ = srs.shape
        size, nb = S - 2 * border, 2 * border + 1
        s = srs[:, border:border + size, border:border + size]
        s = (s.clamp(0, 1) if clip else s).double()
        scores = torch.zeros((B, nb * nb), dtype=D)
        for u in range(nb):
            for v in range(nb):
                m = maps[:, u:u + size, v:v + size].double()
                d = hrs[:, u:u + size, v:v + size].double() - s
                s0, s1, s2 = m.sum((1, 2)), (m * d).sum((1, 2)), (m * m * d * d).sum((1, 2))
                scores[:, u * nb + v] = -10 * torch.log10((s2 - s1 * s1 / s0) / s0)
        return scores, K.ref_score_max(scores, torch.zeros_like(scores))[0].float().double()


MODEL = F32Model()


# ----------------------------------------------------------------------------------------------------------- the references themselves
def _close(got, want, tol=1e-12):
    got, want = torch.as_tensor(got, dtype=D), torch.as_tensor(want, dtype=D)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert float((got - want).abs().max()) <= tol * (1.0 + float(want.abs().max())), float((got - want).abs().max())


def test_references_reproduce_the_lanczos_golden():
    """taps and shifted images the reference's lanczos.py wrote (float32), at test_oracle_golden.py's tolerances"""
    g = util.golden("lanczos")
    taps, _ = K.ref_taps(torch.from_numpy(g["d"]).double().reshape(-1))
    assert np.abs(taps.numpy() - g["taps"]).max() < 2e-6
    out = K.ref_lanczos_shift(torch.from_numpy(g["img"]).double(), torch.from_numpy(g["shift"]).double())
    assert np.abs(out.numpy() - g["shifted"]).max() < 5e-6


def test_references_reproduce_the_callers_golden():
    g = util.golden("callers")
    srs, hrs, maps = (torch.from_numpy(g[n]).double() for n in ("srs", "hrs", "maps"))
    r = K.ref_losses(srs, hrs, maps, 3)
    assert util.rel_err(r["cpsnr"].numpy(), g["loss_cpsnr"]) < 1e-5 and util.rel_err(r["cmse"].numpy(), g["loss_cmse"]) < 1e-5
    assert bool(torch.equal(K.crop_mask(96, 3), torch.from_numpy(g["crop"][0, 0]).double()))
    plain, _ = K.ref_shift_scores(srs, hrs, maps, 0, True)
    assert util.rel_err(plain[:, 0].numpy(), g["cpsnr"]) < 1e-9
    scores, bounds = K.ref_shift_scores(srs, hrs, maps, 3, True)
    assert util.rel_err(K.ref_score_max(scores, bounds)[0].numpy(), g["shift_cpsnr"]) < 1e-9


def test_references_agree_with_the_ports():
    img, shift, dout, _ = K.lanczos_inputs(2, 3, 17, 65)
    i64, s64 = img.double(), shift.double()
    # (the port multiplies by the fp64 pi, the kernels' definition by float32(pi): a relative 2.8e-8 of t)
    assert float((K.ref_lanczos_shift(i64, s64) - torch_port.lanczos_shift(i64, s64)).abs().max()) < 2e-6
    pi32 = K.PI32
    try:
        K.PI32 = float(np.pi)
        _close(K.ref_lanczos_shift(i64, s64), torch_port.lanczos_shift(i64, s64))
        _close(K.ref_taps(torch.tensor(K.TAP_D, dtype=D))[0], O.lanczos_kernel(np.array(K.TAP_D), dtype=np.float64))
    finally:
        K.PI32 = pi32
    srs, hrs, maps = (t.double() for t in K.loss_inputs(3, 17, "frac"))
    r = K.ref_losses(srs, hrs, maps, 0)
    for key, metric in (("mmse", "masked_MSE"), ("cmse", "cMSE"), ("cpsnr", "cPSNR")):
        _close(r[key], O.get_loss(srs.numpy(), hrs.numpy(), maps.numpy(), metric))
    cropped = K.ref_losses(srs, hrs, maps, 3)
    _close(cropped["cmse"], O.get_loss(srs.numpy(), hrs.numpy(), (maps * K.crop_mask(17, 3)).numpy(), "cMSE"))
    _close(cropped["cpsnr"], torch_port.registered_loss_cpsnr(srs, hrs, maps * K.crop_mask(17, 3)))
    srs, hrs, maps = (t.double() for t in K.score_inputs(3, 23, 3))
    scores, bounds = K.ref_shift_scores(srs, hrs, maps, 3, True)
    _close(K.ref_score_max(scores, bounds)[0], O.shift_cpsnr(srs.clamp(0, 1).numpy(), hrs.numpy(), maps.numpy()))
    _close(scores[:, 3 * 7 + 3], O.cpsnr(srs.clamp(0, 1).numpy()[:, 3:-3, 3:-3], hrs.numpy()[:, 3:-3, 3:-3], maps.numpy()[:, 3:-3, 3:-3]))
    # the planted offset is the best one, and it is not its own transpose
    pu, pv = K.PLANTED[3]
    assert pu != pv and int(scores[0].argmax()) == (3 + pu) * 7 + (3 + pv)


def test_loss_gradient_reference_is_autograd_of_the_loss():
    srs, hrs, maps = (t.double() for t in K.loss_inputs(3, 17, "mixed"))
    d_out = K.train_d_out(3).double()
    m = maps * K.crop_mask(17, 3)
    r = K.ref_losses(srs, hrs, maps, 3)
    for metric in (1, 2):
        x = srs.clone().requires_grad_(True)
        cpsnr = torch_port.registered_loss_cpsnr(x, hrs, m)
        ((cpsnr if metric == 2 else 10 ** (-cpsnr / 10)) * d_out).sum().backward()
        want, T = K.ref_loss_grad(srs, hrs, r, metric, d_out)
        _close(want, x.grad, 1e-10)
        assert bool((T >= want.abs() * (1 - 1e-12)).all())


def test_tap_gradient_closed_form_is_autograd_of_the_where_form():
    """dk / dd of ref_tap_grad (the bound's ingredient) against autograd; a frozen tap passes exactly nothing; and giving it its gradient
    back (the 1e-6 added rather than put through a where) moves no tap's derivative by more than 2e-6: sinc'(1e-6) = -3.3e-7.  A kernel
    that leaves the freeze out is therefore not what the frozen-tap control can catch; one that freezes the wrong tap is."""
    d = torch.tensor(K.TAP_D, dtype=D)
    dk, Tdk = K.ref_tap_grad(d)
    jac = torch.autograd.functional.jacobian(lambda x: K.ref_taps(x)[0], d)            # (n, 7, n)
    auto = torch.stack([jac[i, :, i] for i in range(len(d))])
    _close(dk, auto, 1e-9)
    assert bool((Tdk >= dk.abs()).all())
    whole = torch.tensor([1.0, -2.0, 3.0], dtype=D)
    live = torch.autograd.functional.jacobian(lambda x: K.ref_taps(x, "live")[0], whole)
    frozen = torch.autograd.functional.jacobian(lambda x: K.ref_taps(x)[0], whole)
    assert float((live - frozen).abs().max()) < 2e-6
    centre = torch.autograd.functional.jacobian(lambda x: K.ref_taps(x, "centre")[0], whole)
    assert float((centre - frozen).abs().max()) > 0.1


def test_tap_gradient_bound_holds_for_the_closed_form_in_float32():
    """taps7_and_grad's formula evaluated in float32, at every shift of the taps' cases: inside C_TAIL T(dk) per tap"""
    d = torch.tensor(K.TAP_D, dtype=F)
    pi = torch.tensor(np.float32(np.pi))
    t = pi * ((torch.arange(7, dtype=F) - 3)[None, :] - d[:, None])
    hit = t == 0
    t = torch.where(hit, torch.tensor(1e-6, dtype=F), t)
    t3 = t / 3
    A, B = torch.sin(t) / t, torch.sin(t3) / t3
    dA, dB = (torch.cos(t) * t - torch.sin(t)) / (t * t), (torch.cos(t3) * t3 - torch.sin(t3)) / (t3 * t3) * (1.0 / 3.0)
    u, du = A * B, torch.where(hit, torch.zeros_like(t), -pi * (dA * B + A * dB))
    s, ds = u.sum(1, keepdim=True), du.sum(1, keepdim=True)
    got = (du * s - u * ds) / (s * s)
    assert got.dtype == F
    want, T = K.ref_tap_grad(d.double())
    K._assert_close("dk / dd in float32", "f32", got.double(), want, T, layout="i j", c=K.C_TAIL)


def test_shift_gradient_is_the_tap_sums_through_the_tap_gradient():
    """d_shift = sum_j dk_j G_j: the decomposition lanczos_dshift_T bounds term by term"""
    img, shift, dout, _ = (t.double() for t in K.lanczos_inputs(2, 3, 7, 9))
    _, ds = K.ref_lanczos_grads(img, shift, dout)
    rows = K._plane_rows(2, 3)
    G = K.tap_sums(img, dout, K.ref_taps(shift[:, 0])[0][rows], K.ref_taps(shift[:, 1])[0][rows])
    for ax in (0, 1):
        _close((K.ref_tap_grad(shift[:, ax])[0] * G[:, ax]).sum(1), ds[:, ax], 1e-10)
    assert bool((K.lanczos_dshift_T(img, shift, dout) >= ds.abs()).all())


def test_cases_reach_what_they_name():
    d = K.tap_inputs(65)
    assert set(d.tolist()) == set(torch.tensor(K.TAP_D, dtype=F).tolist()) and bool(torch.signbit(d[d == 0]).any())
    t, hit = K._tap_t(K.TAIL_SHIFTS[:, 0].double())
    assert hit[0].tolist() == [False] * 5 + [True, False] and not bool(hit[1:].any())           # dy = 2: the frozen tap is j = 5
    assert bool(K._tap_t(K.TAIL_SHIFTS[:, 1].double())[1][2, 2]) and float(K.TAIL_SHIFTS.abs().max()) > 3
    assert {(H + W) % 3 for H, W in K.LANCZOS_FWD_SHAPES} == {0, 1, 2} == {(H + W) % 3 for H, W in K.LANCZOS_BWD_SHAPES}
    assert K.crops(1) == [0] and K.crops(3) == [0, 1] and K.crops(16) == [0, 3, 7] and K.crops(129) == [0, 3, 64]
    srs, hrs, maps = K.loss_inputs(3, 65, "bin", ill=True)
    r = K.ref_losses(srs.double(), hrs.double(), maps.double(), 3)
    assert bool((r["cmse"] * 1e4 < (srs.double() - hrs.double()).pow(2).mean((1, 2))).all())        # S2 / S0 ~ 0.04, cMSE ~ 1e-6
    srs, _, _ = K.score_inputs(1, 23, 3)
    assert float(srs.min()) < 0 and float(srs.max()) > 1


# ----------------------------------------------------------------------------------------------------------- the bounds on the float32 model
@pytest.mark.parametrize("n", K.TAP_N)
def test_taps(n):
    K.check_taps(MODEL, n)


@pytest.mark.parametrize("b,c", K.LANCZOS_BC)
@pytest.mark.parametrize("H,W", K.LANCZOS_FWD_SHAPES)
def test_lanczos_shift(H, W, b, c):
    K.check_lanczos_fwd(MODEL, b, c, H, W)


@pytest.mark.parametrize("b,c", K.LANCZOS_BC)
@pytest.mark.parametrize("H,W", K.LANCZOS_BWD_SHAPES)
def test_lanczos_shift_backward(H, W, b, c):
    K.check_lanczos_bwd(MODEL, b, c, H, W)


@pytest.mark.parametrize("kind", ["bin", "frac", "zero"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("S,crop", [(S, cr) for S in K.LOSS_S for cr in K.crops(S)])
def test_get_loss(S, crop, B, kind):
    K.check_get_loss(MODEL, S, crop, B, kind)


def test_get_loss_ill_conditioned():
    K.check_get_loss(MODEL, 65, 3, 3, "bin", ill=True)


def test_get_loss_float_accumulators_would_fail_the_ill_conditioned_case():
    """the same one-pass formula with float32 sums is far outside the bound: the case does need the fp64 accumulators"""
    srs, hrs, maps = K.loss_inputs(3, 65, "bin", ill=True)
    m = maps * K.crop_mask(65, 3).float()
    d = srs - hrs
    s0, s1, s2 = m.sum((1, 2)), (m * d).sum((1, 2)), (m * d * d).sum((1, 2))
    r = K.ref_losses(srs.double(), hrs.double(), maps.double(), 3)
    assert K._within_ratio(((s2 - s1 * s1 / s0) / s0).double(), r["cmse"], r["e_cmse"] + K.U32 * r["cmse"]) > 1e3


@pytest.mark.parametrize("metric", [1, 2])
@pytest.mark.parametrize("B,kind", [(1, "bin"), (1, "frac"), (65, "mixed")])
@pytest.mark.parametrize("S,crop", [(S, cr) for S in K.TRAIN_S for cr in K.crops(S)])
def test_get_loss_train_and_backward(S, crop, B, kind, metric):
    K.check_loss_train(MODEL, S, crop, B, kind, metric)


@pytest.mark.parametrize("clip", [0, 1])
@pytest.mark.parametrize("B", [1, 65])
@pytest.mark.parametrize("border,S", [(b, S) for b in K.SCORE_BORDERS for S in (2 * b + 1, 23)])
def test_shift_cpsnr(border, S, B, clip):
    K.check_shift_cpsnr(MODEL, border, S, B, clip)


@pytest.mark.parametrize("control", K.TAIL_CONTROLS)
def test_negative_control(control):
    ok, worst = K.tail_control(MODEL, control)
    print(f"{control}: error / bound against the wrong reference {worst:.3e} (right one {ok:.3e})")
    assert ok <= 1.0 and worst > 1.0, f"{control}: the bound does not tell the wrong reference from the right one"
