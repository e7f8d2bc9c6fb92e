"""GPU (-m gpu): the HRNet training path (`loss.backward()` through HRNet, train.py:172-190).

Oracle: torch autograd on the CPU through oracle/torch_port.hrnet_forward (the restatement the goldens pin), run in float64,
with the same seeded weights and inputs.  The HIP path goes HRNet.forward (grad enabled) -> hrn_hrnet_forward_train ->
loss.backward() -> hrn_hrnet_backward, all fp32.  Tolerance: 2e-4 relative per parameter tensor (max-norm), fp32
accumulation over up to 1e5 pixels; measured ~1e-6..1e-5.  No reference-side golden exists for gradients: the reference's
own backward is torch autograd over the same operator sequence, which is what the oracle side runs here.
"""
import numpy as np
import pytest
import torch

from oracle import synth, torch_port, weights
import util
from util import NONPOS, _SLOPE_KEYS, _fresh_model, _get_loss_cpsnr, _oracle_grads, _register_batch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("B,V,S,n_real,alpha_residual", [
    (2, 4, 16, 4, True),        # power of two
    (2, 5, 16, 4, True),        # odd view count (one view unpaired at the first level), one padded view
    (1, 7, 24, 7, True),        # 24 x 24: partial tiles in both directions; odd at two levels
    (2, 6, 16, 6, False),       # alpha_residual = false branch (HRNet.py:123)
    (2, 1, 16, 1, True),        # a single view: no fusion level at all
    (1, 3, 33, 3, True),        # H % 8 == 1, W % 32 == 1, odd V: the x halo's leftover columns, a one-pixel last bf16x3 strip
    (2, 2, 5, 2, True),         # smaller than one tile in both directions
    (1, 9, 37, 1, True),        # one real view among nine
])
@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
def test_hrnet_backward_vs_autograd_oracle(B, V, S, n_real, alpha_residual, prec):
    """prec "bf16x3": the same check for the split-bf16 training mode (forward, data gradients and weight gradients on the bf16 matrix
    cores, three MFMAs per product; activations and gradients as hi/lo bf16 pairs, ~2^-16 per product instead of fp32's 2^-24).  A
    PReLU's derivative jumps at zero: the handful of activations whose sign differs between a ~1e-5 forward and the fp64 oracle each
    move a weight gradient by ~1 / sqrt(#pixels) - the exact-fp32 path shows the same 2e-3..1e-2 at 64 x 64 (tools/x3_grad_debug.py) -,
    so the KERNELS are pinned with every PReLU slope at 1 (the network is then linear in its activations and nothing can flip:
    measured 1.4e-5, held to the fp32 bounds), and `test_bf16x3_gradients_with_default_slopes` bounds the flips."""
    k_tol = 1.0
    slopes = None if prec == "fp32" else {k: 1.0 for k in _SLOPE_KEYS}
    lrs, alphas, _ = synth.make_batch(5, B, V, S, n_real)
    rng = np.random.Generator(np.random.PCG64(77))
    cot = rng.standard_normal((B, 1, 3 * S, 3 * S)).astype(np.float32)
    want_sr, want = _oracle_grads(lrs, alphas, cot, alpha_residual, slopes=slopes)
    m = _fresh_model(alpha_residual, precision=prec, slopes=slopes)
    sr = m(util.dev(lrs), util.dev(alphas))
    assert sr.requires_grad
    assert util.rel_err(sr.detach().cpu().numpy(), want_sr) <= (2e-5 if prec == "fp32" else 1e-4)
    (sr * util.dev(cot)).sum().backward()
    # PReLU-slope / final-bias gradients are sums of ~1e4..1e5 signed terms that can cancel to a small net value (the stem's at
    # V = 1: 0.026 against a sum of |terms| in the tens).  A float32 implementation carries each TERM to ~1e-6..1e-5 relative, so
    # its error on the sum is bounded by that times sum |terms| - which the oracle records (torch_port.ABS_TERMS); scalars are
    # held to 2e-5 of sum |terms| of their own defining sum, tensors to 2e-4 of their own max-norm.
    abs_terms = want["__abs_terms__"]
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        got = p.grad.cpu().numpy()
        if p.numel() == 1:
            bound = 2e-5 * k_tol * abs_terms.get(k, 0.0) + 1e-12
            assert abs(float(got.ravel()[0]) - float(want[k].ravel()[0])) <= bound, (k, got, want[k], abs_terms.get(k))
        else:
            e = util.rel_err(got, want[k])
            assert e <= 2e-4 * k_tol, (k, e)
    # a second backward pass accumulates into .grad like autograd does
    sr2 = m(util.dev(lrs), util.dev(alphas))
    (sr2 * util.dev(cot)).sum().backward()
    k0, p0 = next(iter(m.named_parameters()))
    assert util.rel_err(p0.grad.cpu().numpy(), 2 * want[k0]) <= 2e-4 * k_tol


def test_bf16x3_gradients_with_default_slopes():
    """The split-bf16 training mode at the reference's PReLU slopes (0.25): gradients within 3e-2 of the fp64 oracle's max-norm per
    tensor (sign flips of near-zero activations, see above; measured 2e-4 .. 3e-3 here), the forward within 1e-4."""
    lrs, alphas, _ = synth.make_batch(5, 2, 4, 16, 4)
    rng = np.random.Generator(np.random.PCG64(77))
    cot = rng.standard_normal((2, 1, 48, 48)).astype(np.float32)
    want_sr, want = _oracle_grads(lrs, alphas, cot, True)
    m = _fresh_model(True, precision="bf16x3")
    sr = m(util.dev(lrs), util.dev(alphas))
    assert util.rel_err(sr.detach().cpu().numpy(), want_sr) <= 1e-4
    (sr * util.dev(cot)).sum().backward()
    for k, p in m.named_parameters():
        if p.numel() > 1:
            assert util.rel_err(p.grad.cpu().numpy(), want[k]) <= 3e-2, k


def test_backward_twice_with_retain_graph():
    """`loss.backward(retain_graph=True)` followed by a second backward through the same graph: the workspaces of the HIP
    forward-for-training stay intact (nothing in the backward kernels writes into them) and the gradients accumulate to twice
    the single-pass values, for HRNet and for ShiftNet."""
    from DeepNetworks.ShiftNet import ShiftNet
    lrs, alphas, _ = synth.make_batch(5, 2, 4, 16, 4)
    m = _fresh_model()
    out = (m(util.dev(lrs), util.dev(alphas)) ** 2).sum()
    out.backward(retain_graph=True)
    once = {k: p.grad.clone() for k, p in m.named_parameters()}
    out.backward()
    for k, p in m.named_parameters():
        assert torch.allclose(p.grad, 2 * once[k], rtol=1e-5, atol=1e-6 * float(once[k].abs().max()) + 1e-12), k
    sn = ShiftNet()
    sn.load_state_dict(weights.to_torch_state(weights.shiftnet_state(4321)))
    sn = sn.cuda().train()
    x = torch.rand(3, 2, 128, 128, device="cuda").requires_grad_(True)
    th = (sn(x) ** 2).sum()
    th.backward(retain_graph=True)
    gx = x.grad.clone()
    th.backward()
    assert torch.allclose(x.grad, 2 * gx, rtol=1e-5, atol=1e-6 * float(gx.abs().max()) + 1e-12)


def test_predict_py_path_hits_the_asked_precision():
    """src/predict.py never calls .eval() and uses no no_grad (load_model :86-100, get_sr_and_score :17-49): re-enact it on a FRESH
    module.  precision fp32: same numbers as the .eval() forward; precision bf16: the bf16 inference kernels run (bit-identical
    to .eval()), not the fp32 training kernels - and a backward pass through that result still works (recomputed in fp32)."""
    from DeepNetworks.HRNet import HRNet
    lrs, alphas, hrs = synth.make_batch(17, 1, 9, 32, 7)                 # one imageset, as get_sr_and_score collates it
    x, a = util.dev(lrs), util.dev(alphas)
    for prec in ("fp32", "bf16"):
        cfg = {k: dict(v) for k, v in weights.HRNET_CONFIG.items()}
        cfg["precision"] = prec
        model = HRNet(cfg).cuda()                                        # load_model: no .eval()
        model.load_state_dict(weights.to_torch_state(weights.hrnet_state(1234)))
        assert model.training
        sr = model(x, a)[:, 0]                                           # predict.py:39
        got = sr.detach().cpu().numpy()[0]                               # :40
        with torch.no_grad():
            want = model.eval()(x, a)[:, 0].cpu().numpy()[0]
        if prec == "bf16":
            assert np.array_equal(got, want)
        else:
            assert util.rel_err(got, want) <= 1e-6
        model.train()
        sr2 = model(x, a)
        (sr2 ** 2).sum().backward()
        ref_m = _fresh_model()
        (ref_m(x, a) ** 2).sum().backward()
        g1 = dict(model.named_parameters())["fuse.fuse.1.weight"].grad
        g0 = dict(ref_m.named_parameters())["fuse.fuse.1.weight"].grad
        tol = 1e-5 if prec == "fp32" else 5e-2           # bf16: d(sr^2) is taken at the bf16-rounded output, the chain itself is fp32
        assert float((g1 - g0).abs().max()) <= tol * float(g0.abs().max()), prec


def test_hrnet_train_step_reduces_loss():
    """A few Adam steps on the HIP forward/backward drive a plain L2 loss down; eval forward sees the updated weights."""
    lrs, alphas, _ = synth.make_batch(9, 2, 4, 16, 4)
    m = _fresh_model()
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    x, a = util.dev(lrs), util.dev(alphas)
    target = torch.zeros((2, 1, 48, 48), device="cuda") + 0.1
    losses = []
    for _ in range(6):
        opt.zero_grad()
        loss = ((m(x, a) - target) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert losses[-1] < 0.7 * losses[0], losses
    with torch.no_grad():
        after = ((m.eval()(x, a) - target) ** 2).mean()
    assert float(after) < losses[0]


def test_bf16x3_training_tracks_fp32_training():
    """Twenty Adam steps from the same initial weights on the same batch, HRNet once on the fp32 and once on the bf16x3 training
    kernels: the two loss curves stay together (the modes differ by ~2e-5 per forward; Adam's sign-like first steps amplify that, so
    the bound is on the curve, not on bits) and both fall."""
    lrs, alphas, _ = synth.make_batch(9, 2, 4, 16, 4)
    x, a = util.dev(lrs), util.dev(alphas)
    target = torch.zeros((2, 1, 48, 48), device="cuda") + 0.1
    curves = {}
    for prec in ("fp32", "bf16x3"):
        m = _fresh_model(precision=prec)
        opt = torch.optim.Adam(m.parameters(), lr=1e-3)
        curve = []
        for _ in range(20):
            opt.zero_grad()
            loss = ((m(x, a) - target) ** 2).mean()
            loss.backward()
            opt.step()
            curve.append(float(loss.detach()))
        curves[prec] = np.array(curve)
    rel = np.abs(curves["bf16x3"] - curves["fp32"]) / curves["fp32"]
    print("fp32 vs bf16x3 training: loss", curves["fp32"][[0, 9, 19]], curves["bf16x3"][[0, 9, 19]], "max rel diff", rel.max())
    assert curves["fp32"][-1] < 0.5 * curves["fp32"][0] and curves["bf16x3"][-1] < 0.5 * curves["bf16x3"][0]
    assert rel.max() <= 2e-2, rel


@pytest.mark.parametrize("slopes", [NONPOS, {"fuse.fuse.2.weight": -0.25}, {"encode.res_layers.1.block.1.weight": 1.5}])
def test_hrnet_backward_with_nonpositive_slopes(slopes):
    """nn.PReLU puts no constraint on its slope and training can drive one through zero.  With a positive slope the HIP backward reads
    the sign of the pre-activation off the stored post-activation; behind a slope <= 0 that is impossible (y >= 0 on both branches),
    and the backward recomputes the pre-activation - decided per PReLU ON THE DEVICE.  Every PReLU of the model at a non-positive
    slope (negative and exactly zero), one alone, and a slope above one (positive: the stored-activation path): forward and every
    gradient against fp64 autograd on the port."""
    B, V, S = 2, 5, 16
    lrs, alphas, _ = synth.make_batch(5, B, V, S, 4)
    rng = np.random.Generator(np.random.PCG64(78))
    cot = rng.standard_normal((B, 1, 3 * S, 3 * S)).astype(np.float32)
    want_sr, want = _oracle_grads(lrs, alphas, cot, True, slopes=slopes)
    m = _fresh_model(True, slopes=slopes)
    sr = m(util.dev(lrs), util.dev(alphas))
    assert util.rel_err(sr.detach().cpu().numpy(), want_sr) <= 2e-5
    (sr * util.dev(cot)).sum().backward()
    abs_terms = want["__abs_terms__"]
    for k, p in m.named_parameters():
        got = p.grad.cpu().numpy()
        if p.numel() == 1:
            bound = 2e-5 * abs_terms.get(k, 0.0) + 1e-12
            assert abs(float(got.ravel()[0]) - float(want[k].ravel()[0])) <= bound, (k, got, want[k], abs_terms.get(k))
        else:
            e = util.rel_err(got, want[k])
            assert e <= 2e-4, (k, e)
    # and the bf16 inference kernels take the same slopes (one activation path for every slope: conv3x3_v6 / conv3x3_r64)
    with torch.no_grad():
        from DeepNetworks.HRNet import HRNet
        cfg = {k: dict(v) for k, v in weights.HRNET_CONFIG.items()}
        cfg["precision"] = "bf16"
        mb = HRNet(cfg)
        mb.load_state_dict(m.state_dict())
        got = mb.cuda().eval()(util.dev(lrs), util.dev(alphas)).cpu().numpy()
    assert util.rel_err(got, want_sr) <= 4e-2


def test_bf16x3_backward_with_nonpositive_slopes():
    """The same recomputation (ConvParams::only_if_nonpos) on the bf16x3 kernels: every PReLU at a non-positive slope.  Forward to the
    bf16x3 bound; gradients against fp64 autograd in the L2 norm of each tensor - element-wise they carry the sign flips of
    pre-activations within ~1e-5 of zero (test_bf16x3_gradients_with_default_slopes), each worth (1 - slope) of a term."""
    B, V, S = 2, 5, 16
    lrs, alphas, _ = synth.make_batch(5, B, V, S, 4)
    rng = np.random.Generator(np.random.PCG64(78))
    cot = rng.standard_normal((B, 1, 3 * S, 3 * S)).astype(np.float32)
    want_sr, want = _oracle_grads(lrs, alphas, cot, True, slopes=NONPOS)
    m = _fresh_model(True, slopes=NONPOS, precision="bf16x3")
    sr = m(util.dev(lrs), util.dev(alphas))
    assert util.rel_err(sr.detach().cpu().numpy(), want_sr) <= 1e-4
    (sr * util.dev(cot)).sum().backward()
    worst = {}
    for k, p in m.named_parameters():
        if p.numel() == 1:
            continue
        got = p.grad.cpu().numpy().astype(np.float64)
        ref = np.asarray(want[k], np.float64)
        worst[k] = float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-30))
    top = sorted(worst.items(), key=lambda kv: -kv[1])[:4]
    print("bf16x3, non-positive slopes: worst relative L2 gradient errors", top)
    assert top[0][1] <= 2e-2, top


# ----------------------------------------------------------------------------- Lanczos shift backward
_torch_lanczos_shift = torch_port.lanczos_shift      # fp64 torch restatement of lanczos.py:5-107, pinned by tests/golden/train_step.npz


@pytest.mark.parametrize("b,c,H,W", [(1, 5, 48, 48), (2, 3, 20, 70), (1, 2, 7, 9),
                                     (1, 32, 192, 192),     # apply_shifts at the training shape: b = 1, c = B frames of 3S x 3S
                                     (1, 1, 520, 520)])     # above 512^2 px: lanczos_adjoint_kernel's grid (capped at 1024) strides
def test_lanczos_shift_backward_vs_autograd(b, c, H, W):
    import lanczos
    rng = np.random.Generator(np.random.PCG64(11))
    img = rng.random((b, c, H, W), dtype=np.float32)
    shift = rng.uniform(-1.5, 1.5, (c, 2)).astype(np.float32)
    shift[0] = (0.0, 0.25)                                   # an exact-zero shift: pi*x == 0 at the centre tap (frozen to 1e-6)
    cot = rng.standard_normal((b, c, H, W)).astype(np.float32)
    ti = torch.from_numpy(img).double().requires_grad_(True)
    ts = torch.from_numpy(shift).double().requires_grad_(True)
    want = _torch_lanczos_shift(ti, ts)
    (want * torch.from_numpy(cot).double()).sum().backward()
    gi = util.dev(img).requires_grad_(True)
    gs = util.dev(shift).requires_grad_(True)
    got = lanczos.lanczos_shift(gi, gs)
    assert got.requires_grad
    assert np.abs(got.detach().cpu().numpy() - want.detach().numpy()).max() <= 2e-5
    (got * util.dev(cot)).sum().backward()
    assert util.rel_err(gi.grad.cpu().numpy(), ti.grad.numpy()) <= 1e-4
    assert np.abs(gs.grad.cpu().numpy() - ts.grad.numpy()).max() <= 1e-3 * max(1.0, float(ts.grad.abs().max()))
    # image-only and shift-only requests
    gi2 = util.dev(img).requires_grad_(True)
    (lanczos.lanczos_shift(gi2, util.dev(shift)) * util.dev(cot)).sum().backward()
    assert util.rel_err(gi2.grad.cpu().numpy(), ti.grad.numpy()) <= 1e-4


# ----------------------------------------------------------------------------- ShiftNet backward
_torch_shiftnet = torch_port.shiftnet_forward_train   # ShiftNet.forward in train mode with a given dropout keep-mask (same pin)


@pytest.mark.parametrize("B", [3, 35])          # 35: more pairs than one fc1 data-gradient launch holds (groups of 32)
def test_shiftnet_backward_vs_autograd(B):
    from DeepNetworks.ShiftNet import ShiftNet
    rng = np.random.Generator(np.random.PCG64(21))
    x = (rng.random((B, 2, 128, 128), dtype=np.float32) * 0.25).astype(np.float32)
    x[:, 1] = 0.7 * x[:, 0] + 0.3 * x[:, 1]                  # correlated pair, like (reference, image)
    mask = (rng.random((B, 32768)) >= 0.5)
    cot = rng.standard_normal((B, 2)).astype(np.float32)
    state = weights.to_torch_state(weights.shiftnet_state(4321))
    st = {k: v.double().requires_grad_(v.dtype.is_floating_point and "running" not in k and "num_batches" not in k) for k, v in state.items()}
    tx = torch.from_numpy(x).double().requires_grad_(True)
    want = _torch_shiftnet(tx, st, torch.from_numpy(mask).double())
    (want * torch.from_numpy(cot).double()).sum().backward()

    m = ShiftNet()
    m.load_state_dict(state)
    m = m.cuda().train()
    gx = util.dev(x).requires_grad_(True)
    torch.manual_seed(0)
    # feed the same keep-mask the oracle used: patch the module's RNG draw
    dmask = torch.from_numpy(mask.astype(np.uint8)).cuda()
    orig_rand = torch.rand
    try:
        torch.rand = lambda *a, **k: (dmask.float() * 0.75 + 0.125).reshape(a[0]) if a and tuple(a[0]) == (B, 32768) else orig_rand(*a, **k)
        theta = m(gx)
    finally:
        torch.rand = orig_rand
    assert theta.requires_grad
    assert util.rel_err(theta.detach().cpu().numpy(), want.detach().numpy()) <= 2e-4
    (theta * util.dev(cot)).sum().backward()
    # the input gradient: ReLU and max-pool are discontinuous in their derivative, so a pre-activation that is +1e-9 in fp64 and
    # -1e-9 in fp32 (or a pool window whose two largest values swap) moves single elements by O(1 %) of the largest gradient: with
    # more samples such events become certain (measured: per sample either ~1e-5 or ~1e-2 at B = 16..35, B <= 32 included).  All
    # but 0.5 % of the elements (one flipped unit of a deep layer reaches a large input patch; 0.10 % measured at B = 35) must agree
    # to 2e-3, and none may be off by more than 5e-2.
    err = np.abs(gx.grad.cpu().numpy() - tx.grad.numpy()) / np.abs(tx.grad.numpy()).max()
    assert err.max() <= (2e-3 if B <= 4 else 5e-2) and float((err > 2e-3).mean()) <= 5e-3, (err.max(), float((err > 2e-3).mean()))
    for k, p in m.named_parameters():
        got, ref = p.grad.cpu().numpy(), st[k].grad.numpy()
        if k.endswith(".0.bias"):
            # a conv bias in front of a train-mode BatchNorm has a mathematically zero gradient: both sides hold rounding noise
            scale = float(np.abs(st[k.replace(".0.bias", ".1.bias")].grad.numpy()).max())
            assert np.abs(got).max() <= 1e-3 * scale and np.abs(ref).max() <= 1e-3 * scale, k
            continue
        # B = 35: the same flips, summed over 35 x 16384 positions - 1e-3..1.7e-2 per tensor, exactly as at B = 32 (layer5.0.weight
        # 1.4e-2 there): the grouped fc1 launches add nothing to it
        assert util.rel_err(got, ref) <= (2e-3 if B <= 4 else 2.5e-2), (k, util.rel_err(got, ref))


# ----------------------------------------------------------------------------- the whole train step of src/train.py
def test_full_train_step_vs_autograd_oracle():
    """srs = fusion_model(lrs, alphas); shifts = register_batch(...); srs_shifted = apply_shifts(...); loss = -cPSNR + lambda
    mean(shifts)^2; loss.backward()  (train.py:172-190) on the HIP modules, against the same chain in fp64 torch on the CPU."""
    from DeepNetworks.ShiftNet import ShiftNet
    B, V, S, lam = 2, 3, 48, 1e-6
    lrs, alphas, hrs = synth.make_batch(31, B, V, S, V)
    rng = np.random.Generator(np.random.PCG64(5))
    maps = (rng.random((B, 3 * S, 3 * S)) > 0.1).astype(np.float32)
    crop = np.ones((3 * S, 3 * S), np.float32)
    crop[:3] = 0; crop[-3:] = 0; crop[:, :3] = 0; crop[:, -3:] = 0
    mask = (rng.random((B, 32768)) >= 0.5)
    off = (3 * S - 128) // 2
    hstate = weights.to_torch_state(weights.hrnet_state(1234))
    sstate = weights.to_torch_state(weights.shiftnet_state(4321))

    # ---- oracle chain, fp64 on the CPU
    hst = {k: v.double().requires_grad_(True) for k, v in hstate.items()}
    sst = {k: v.double().requires_grad_("running" not in k and "num_batches" not in k) for k, v in sstate.items()}
    with torch.enable_grad():
        srs = torch_port.hrnet_forward.__wrapped__(torch.from_numpy(lrs).double(), torch.from_numpy(alphas).double(), hst,
                                                  num_layers=weights.HRNET_CONFIG["encoder"]["num_layers"], alpha_residual=True)
        t_hrs = torch.from_numpy(hrs).double()
        net = lambda pairs: _torch_shiftnet(pairs, sst, torch.from_numpy(mask).double())
        shifts = _register_batch(net, srs[:, :, off:off + 128, off:off + 128], t_hrs[:, off:off + 128, off:off + 128].reshape(-1, 1, 128, 128))
        imgs = srs.view(-1, 1, 3 * S, 3 * S)
        shifted = _torch_lanczos_shift(imgs.transpose(0, 1), shifts.view(-1, 2).flip(-1))[:, None].view(-1, 1, 3 * S, 3 * S)[:, 0]
        loss = -_get_loss_cpsnr(shifted, t_hrs, torch.from_numpy(crop * maps).double())
        loss = loss.mean() + lam * shifts.mean() ** 2
        loss.backward()
    want_loss = float(loss.detach())

    # ---- HIP modules, the statements of train.py
    fusion = _fresh_model(True)
    regis = ShiftNet()
    regis.load_state_dict(sstate)
    regis = regis.cuda().train()
    d_lrs, d_alphas, d_hrs = util.dev(lrs), util.dev(alphas), util.dev(hrs)
    dmask = torch.from_numpy(mask.astype(np.uint8)).cuda()
    orig_rand = torch.rand
    try:
        torch.rand = lambda *a, **k: (dmask.float() * 0.75 + 0.125).reshape(a[0]) if a and tuple(a[0]) == (B, 32768) else orig_rand(*a, **k)
        g_srs = fusion(d_lrs, d_alphas)
        g_shifts = _register_batch(regis, g_srs[:, :, off:off + 128, off:off + 128],
                                   d_hrs[:, off:off + 128, off:off + 128].reshape(-1, 1, 128, 128))
        bsz, nv, hh, ww = g_srs.shape                          # apply_shifts, train.py:47-63
        g_shifted = regis.transform(g_shifts.view(-1, 2), g_srs.view(-1, 1, hh, ww), device="cuda").view(-1, nv, hh, ww)[:, 0]
    finally:
        torch.rand = orig_rand
    g_loss = -_get_loss_cpsnr(g_shifted, d_hrs, util.dev(crop * maps))
    g_loss = g_loss.mean() + lam * g_shifts.mean() ** 2
    g_loss.backward()
    assert abs(float(g_loss.detach()) - want_loss) <= 2e-4 * abs(want_loss)
    assert util.rel_err(g_shifts.detach().cpu().numpy(), shifts.detach().numpy()) <= 1e-3
    # Conditioning: through -10 log10(cMSE) with the brightness correction this chain is ill-conditioned in fp32 - torch's own
    # fp32 CPU autograd differs from the fp64 value by 3e-3..7e-3 on most tensors here (1.5e-2 on one PReLU slope; measured
    # with the same ports), and gradients that are zero by construction (decode.final.bias under the brightness correction,
    # conv biases in front of train-mode BatchNorm) are pure rounding noise on both sides.  Hence 2e-2 / the skips below.
    for name, model, st in (("hrnet", fusion, hst), ("shiftnet", regis, sst)):
        scalar_scale = max([float(np.abs(st[k].grad.numpy()).max()) for k, p in model.named_parameters()
                            if p.numel() == 1 and k != "decode.final.bias"] or [1.0])
        for k, p in model.named_parameters():
            assert p.grad is not None, (name, k)
            got, ref = p.grad.cpu().numpy(), st[k].grad.numpy()
            if k == "decode.final.bias" or (name == "shiftnet" and k.endswith(".0.bias")):
                continue
            if p.numel() == 1:
                assert abs(float(got.ravel()[0]) - float(ref.ravel()[0])) <= 2e-2 * scalar_scale, (name, k, got, ref)
            else:
                assert util.rel_err(got, ref) <= 2e-2, (name, k, util.rel_err(got, ref))


@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
def test_train_step_vs_reference_fixture(prec):
    """(prec "bf16x3": HRNet's forward, data gradients and weight gradients in split-bf16 - the opt-in training mode of
    HRNet(precision="bf16x3") - against the same fixture: loss, shifts and ShiftNet's gradients at the same tolerances, the SR crops to
    1e-4 instead of 2e-5, the gradients' L2 norms at the same tolerances and their sampled elements to 1e-1 of the max-norm.)
    The statements of train.py:172-190 on the HIP modules - with the loss tail on device (hrnet_hip.losses.get_loss: forward AND
    backward, row f1) - against ONE TRAIN STEP OF THE REFERENCE ITSELF (tests/golden/train_step.npz, written by
    oracle/make_goldens.py from the reference's modules in fp64): loss, shifts, SR crops, every parameter gradient.
    Tolerances: tensors 1.5e-2 (HRNet) / 2e-2 (ShiftNet) of their own max-norm on the stored strided sample and on the L2 norm (the chain through
    -10 log10(cMSE) is ill-conditioned in fp32: torch's own fp32 CPU autograd is 3e-3..7e-3 off fp64 here); single-slope PReLU
    gradients, which are cancelling sums, to 1e-2 of SUM |terms| of that sum as the reference computed it (stored in the fixture),
    not of some other parameter's magnitude."""
    from DeepNetworks.ShiftNet import ShiftNet
    from hrnet_hip import losses
    g = util.golden("train_step")
    B, V, S = (int(v) for v in g["shape"])
    lam, crop_w = float(g["lam"]), int(g["crop"])
    lrs, alphas, hrs = synth.make_batch(31, B, V, S, V)
    rng = np.random.Generator(np.random.PCG64(5))
    maps = (rng.random((B, 3 * S, 3 * S)) > 0.1).astype(np.float32)
    mask = (rng.random((B, 32768)) >= 0.5)
    off = (3 * S - 128) // 2
    fusion = _fresh_model(True, precision=prec)
    regis = ShiftNet()
    regis.load_state_dict(weights.to_torch_state(weights.shiftnet_state(4321)))
    regis = regis.cuda().train()
    d_lrs, d_alphas, d_hrs, d_maps = util.dev(lrs), util.dev(alphas), util.dev(hrs), util.dev(maps)
    dmask = torch.from_numpy(mask.astype(np.uint8)).cuda()
    orig_rand = torch.rand
    try:
        torch.rand = lambda *a, **k: (dmask.float() * 0.75 + 0.125).reshape(a[0]) if a and tuple(a[0]) == (B, 32768) else orig_rand(*a, **k)
        srs = fusion(d_lrs, d_alphas)
        shifts = _register_batch(regis, srs[:, :, off:off + 128, off:off + 128], d_hrs[:, off:off + 128, off:off + 128].reshape(-1, 1, 128, 128))
        bsz, nv, hh, ww = srs.shape
        srs_shifted = regis.transform(shifts.view(-1, 2), srs.view(-1, 1, hh, ww), device="cuda").view(-1, nv, hh, ww)[:, 0]
    finally:
        torch.rand = orig_rand
    loss = -losses.get_loss(srs_shifted, d_hrs, d_maps, metric="cPSNR", crop=crop_w)      # get_crop_mask folded into the kernel
    loss = torch.mean(loss) + lam * torch.mean(shifts) ** 2
    loss.backward()
    assert abs(float(loss.detach()) - float(g["loss"])) <= 2e-4 * abs(float(g["loss"]))
    assert util.rel_err(shifts.detach().cpu().numpy(), g["shifts"]) <= 1e-3
    assert util.rel_err(srs.detach().cpu().numpy()[:, :, 40:72, 40:72], g["srs_crop"]) <= (2e-5 if prec == "fp32" else 1e-4)
    # (the shifted SR inherits ShiftNet's answer: a shift off by 1e-3 of its size moves the Lanczos-resampled image by ~3e-4 of its range,
    #  so the bf16x3 bound follows from the shifts' bound above, not from the conv kernels' 2e-5)
    print("train-step fixture", prec, "shifts", util.rel_err(shifts.detach().cpu().numpy(), g["shifts"]),
          "srs", util.rel_err(srs.detach().cpu().numpy()[:, :, 40:72, 40:72], g["srs_crop"]),
          "srs_shifted", util.rel_err(srs_shifted.detach().cpu().numpy()[:, 40:72, 40:72], g["srs_shifted_crop"]))
    assert util.rel_err(srs_shifted.detach().cpu().numpy()[:, 40:72, 40:72], g["srs_shifted_crop"]) <= (1e-4 if prec == "fp32" else 5e-4)
    worst, bad = {}, []
    for prefix, model in (("hrnet", fusion), ("shiftnet", regis)):
        for k, p in model.named_parameters():
            assert p.grad is not None, (prefix, k)
            if prefix == "shiftnet" and k.endswith(".0.bias"):
                continue                # conv bias in front of a train-mode BatchNorm: a mathematically zero gradient
            got = p.grad.detach().cpu().numpy().ravel().astype(np.float64)
            stride = int(g[f"{prefix}/{k}/stride"])
            want = g[f"{prefix}/{k}/sample"]
            if f"{prefix}/{k}/abs_terms" in g.files:
                bound = 1e-2 * float(g[f"{prefix}/{k}/abs_terms"])
                err = float(np.abs(got[::stride] - want).max())
                worst[f"{prefix}/{k}"] = err / max(float(g[f"{prefix}/{k}/abs_terms"]), 1e-300)
                assert err <= bound, (prefix, k, got, want, bound)
                continue
            scale = float(g[f"{prefix}/{k}/absmax"])
            err = float(np.abs(got[::stride] - want).max()) / scale
            nerr = abs(float(np.sqrt((got * got).sum())) - float(g[f"{prefix}/{k}/norm"])) / float(g[f"{prefix}/{k}/norm"])
            worst[f"{prefix}/{k}"] = max(err, nerr)
            # measured (deterministic kernels): HRNet worst 1.0e-2 (fuse.fuse.0.block.2.bias), ShiftNet worst 1.6e-2 (a BatchNorm bias)
            # bf16x3: a ~13x larger forward error (1.6e-5 instead of 1.3e-6) flips the PReLU / ReLU / max-pool decisions of ~1e-5 of
            # the near-zero activations - in HRNet AND in ShiftNet, whose input is HRNet's output -, and every flip moves single
            # gradient elements by O(1 / sqrt(#terms)) (test_hrnet_backward_vs_autograd_oracle pins the kernels with linear PReLUs
            # at 1e-5).  The L2 norms keep the fp32 tolerances (measured <= 7e-3); single elements of the strided sample are held
            # to 1e-1 (HRNet; measured worst 5.1e-2: decode.deconv.0.bias) / 2e-1 (ShiftNet - the fp32 kernels reacting to a 1e-5
            # change of their input at B = 2; worst 1.0e-1: layer6.1.bias, L2 norm 1.5e-3) of the tensor's max-norm.
            tol = 1.5e-2 if prefix == "hrnet" else 2e-2
            if prec != "fp32":
                err = err if err > (1e-1 if prefix == "hrnet" else 2e-1) else 0.0
            if not (err <= tol and nerr <= tol):
                bad.append((prefix, k, round(err, 5), round(nerr, 5), tol))
    assert not bad, bad
    print("worst relative gradient errors vs the reference's train step:", sorted(worst.items(), key=lambda kv: -kv[1])[:6])


# ----------------------------------------------------------------------------- fused Adam
def test_fused_adam_matches_torch_adam():
    """hrn_adam_step on one flat buffer == torch.optim.Adam tensor by tensor (train.py:252), incl. an lr change by a
    scheduler through param_groups and weight decay; the HIP modules see the updated weights (packed-cache epoch)."""
    from hrnet_hip.optim import FusedAdam
    torch.manual_seed(3)
    ref = torch.nn.Sequential(torch.nn.Linear(37, 19), torch.nn.PReLU(), torch.nn.Linear(19, 5)).cuda()
    new = torch.nn.Sequential(torch.nn.Linear(37, 19), torch.nn.PReLU(), torch.nn.Linear(19, 5)).cuda()
    new.load_state_dict(ref.state_dict())
    o_ref = torch.optim.Adam(ref.parameters(), lr=3e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=1e-2)
    o_new = FusedAdam(new.parameters(), lr=3e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=1e-2)
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(o_new, mode="max", factor=0.5, patience=0)
    x = torch.randn(11, 37, device="cuda")
    for it in range(6):
        for m, o in ((ref, o_ref), (new, o_new)):
            o.zero_grad()
            (m(x) ** 2).mean().backward()
            o.step()
        if it == 2:                                       # a plateau: the scheduler halves the lr of the fused optimiser
            sched.step(1.0); sched.step(0.5)
            for g in o_ref.param_groups:
                g["lr"] = o_new.param_groups[0]["lr"]
            assert o_new.param_groups[0]["lr"] == 1.5e-3
    for (k, a), (_, b) in zip(ref.named_parameters(), new.named_parameters()):
        assert torch.allclose(a, b, rtol=2e-5, atol=1e-7), (k, (a - b).abs().max())

    # on the HIP HRNet: parameters re-homed into the flat buffer, training step, eval forward sees the update
    lrs, alphas, _ = synth.make_batch(9, 2, 4, 16, 4)
    m = _fresh_model()
    opt = FusedAdam(m.parameters(), lr=1e-3)
    xs, al = util.dev(lrs), util.dev(alphas)
    with torch.no_grad():
        before = m.eval()(xs, al).clone()
    m.train()
    for _ in range(3):
        opt.zero_grad()
        ((m(xs, al) - 0.1) ** 2).mean().backward()
        opt.step()
    with torch.no_grad():
        after = m.eval()(xs, al)
    assert float((after - before).abs().max()) > 1e-4
    assert float(((after - 0.1) ** 2).mean()) < float(((before - 0.1) ** 2).mean())


def test_config3_train_step_is_bit_reproducible_and_sample_independent():
    """BASELINE configs[3] per rank (B=32, 32 views, 64 x 64 patches: the shape `bench.py --mode train` times): the whole step
    (HRNet -> ShiftNet -> Lanczos -> registered cPSNR loss -> backward) twice from the same weights gives bit-identical gradients
    (every reduction is two-stage with a fixed order, no float atomics), every gradient is finite and non-zero, and the per-sample
    loss of sample 0 does not depend on which other samples share the batch (no cross-sample leak in the HRNet path; ShiftNet's
    train-mode BatchNorm couples samples by design, so the comparison holds the shifts fixed)."""
    import bench
    from DeepNetworks.HRNet import HRNet
    from DeepNetworks.ShiftNet import ShiftNet
    from hrnet_hip import losses
    dev = torch.device("cuda", 0)
    torch.manual_seed(4321)
    fusion = HRNet(dict(bench.NETWORK)).to(dev).train()
    regis = ShiftNet().to(dev).train()
    with torch.no_grad():
        regis.fc2.weight.normal_(0.0, 1e-3)
    B, V, P = 32, 32, 64
    lrs, alphas = bench.synth_inputs(B, V, P, dev, seed=77)
    g = torch.Generator(device="cpu").manual_seed(5)
    hrs = (torch.rand((B, 3 * P, 3 * P), generator=g) * 0.25).to(dev)
    maps = torch.ones((B, 3 * P, 3 * P), device=dev)
    off = (3 * P - 128) // 2
    params = list(fusion.parameters()) + list(regis.parameters())

    def grads(dropout_seed):
        for p in params:
            p.grad = None
        torch.manual_seed(dropout_seed)                       # ShiftNet's dropout mask
        srs = fusion(lrs, alphas)
        ref = hrs[:, off:off + 128, off:off + 128].reshape(-1, 1, 128, 128)
        shifts = torch.stack([regis(torch.cat([ref, srs[:, :, off:off + 128, off:off + 128]], 1))], 1)
        b, n, h, w = srs.shape
        shifted = regis.transform(shifts.view(-1, 2), srs.view(-1, 1, h, w), device=dev).view(-1, n, h, w)[:, 0]
        per_sample = -losses.get_loss(shifted, hrs, maps, metric="cPSNR", crop=3)
        loss = torch.mean(per_sample) + 1e-6 * torch.mean(shifts) ** 2
        loss.backward()
        return float(loss.detach()), [p.grad.detach().clone() for p in params], shifts.detach(), per_sample.detach()

    l1, g1, shifts1, ps1 = grads(11)
    l2, g2, _, _ = grads(11)
    assert l1 == l2
    for a, b in zip(g1, g2):
        assert torch.equal(a, b)
        assert bool(torch.isfinite(a).all())
    assert all(float(a.abs().max()) > 0 for a in g1[:len(list(fusion.parameters()))])
    # sample 0 in a batch of 32 and alone: same SR frame, same registered loss for the same shift
    with torch.no_grad():
        fusion.eval()
        sr_all = fusion(lrs, alphas)
        sr_one = fusion(lrs[:1].contiguous(), alphas[:1].contiguous())
        assert torch.equal(sr_all[:1], sr_one)
        sh = regis.transform(shifts1[:1].view(-1, 2), sr_one.view(-1, 1, 3 * P, 3 * P), device=dev).view(-1, 1, 3 * P, 3 * P)[:, 0]
        one = -losses.get_loss(sh, hrs[:1], maps[:1], metric="cPSNR", crop=3)
    assert abs(float(one[0]) - float(ps1[0])) <= 1e-4 * abs(float(ps1[0]))
