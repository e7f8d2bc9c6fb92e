"""GPU (-m gpu): HRNet with the reference frame given, `forward(lrs, alphas, ref=ref)` and its ensemble / tiled forms
(hrn_hrnet_forward_ref, hrn_hrnet_forward_train_ref, hrn_hrnet_backward_ref).

  identity       ref = the network's own median: bit-equal to the plain call in every precision, eval and training; parameter gradients
                 bit-equal; the plain d_lrs is the ref path's d_lrs with d_ref added at the view the median picked
  independence   a frame that is NOT the median (the masked composite): the forward against the numpy oracle composed from its stages
                 on the hand-stacked (view, ref) input, with the parity bounds of tests/test_gpu_parity.py (util._check); d_lrs, d_ref and
                 the parameter gradients against fp64 torch autograd of the restatement below, with the d_lrs bound of
                 tests/test_gpu_input_grad.py (2e-4 of the max-norm, in fp32 and bf16x3, the two precisions that file bounds: with every
                 slope at 1 at (2, 5, 16, 16) and at the ragged (2, 3, 17, 50), and in fp32 at the default slopes on a small case that no PReLU flip
                 can reach.  Measured:
                 worst of d_lrs / d_ref / any parameter gradient 1.7e-6 fp32 and 2.5e-5 bf16x3 at slopes 1, 2.6e-5 at the default slopes;
                 at (2, 3, 17, 50) 9.6e-6 fp32 and 1.7e-4 bf16x3 (both fuse.fuse.2.weight, one slope: a single sum; every other
                 parameter gradient <= 7.3e-5, d_lrs / d_ref 1.1e-6 / 1.5e-6 and 1.3e-5 / 1.2e-5);
                 at the default slopes at (2, 5, 16, 16) the same kernels gave 7.9e-3 with an sr within 1.8e-6: a flipped activation)
  frozen, tiled, ensemble, end to end, the dispatcher ops
"""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import composite_ref as R
import kt
import util
from hrnet_hip import augment
from oracle import hrnet_np as O
from oracle import synth, torch_port, weights
from util import _SLOPE_KEYS, _fresh_model, _model, _state

pytestmark = pytest.mark.gpu

PRECS = ["fp32", "bf16", "bf16x3"]


def _median(x):
    B, V, H, W = x.shape
    med = torch.empty((B, H, W), dtype=torch.float32, device="cuda")
    assert kt.lib().hrn_kt_median(kt._p(x), kt._p(med), B, V, H, W, kt._stream()) == 0
    return med


def _batch(V, seed=5, B=2, S=16):
    lrs, alphas, _ = synth.make_batch(seed, B, V, S, [V, max(1, V - 1)][:B])
    return lrs, alphas


def _cot(B, S, scale=3, W=None):
    return np.random.Generator(np.random.PCG64(77)).standard_normal((B, 1, scale * S, scale * (W or S))).astype(np.float32)


def _first_tied(lrs, med):
    """the lowest-indexed of the first min(V, 9) views equal to the median, per pixel: (B,H,W) indices"""
    n = min(lrs.shape[1], 9)
    return np.argmax(lrs[:, :n] == med[:, None], 1)


# ----------------------------------------------------------------------------- identity
@pytest.mark.parametrize("V", [1, 4, 5])
@pytest.mark.parametrize("prec", PRECS)
def test_identity_eval(prec, V):
    lrs, alphas = _batch(V)
    x, a = util.dev(lrs), util.dev(alphas)
    m = util.hip_hrnet(prec)
    with torch.no_grad():
        plain = m(x, a)
        got = m(x, a, ref=_median(x))
    assert got.dtype == torch.float32 and not got.requires_grad and torch.equal(got, plain)


def _train_pair(m, lrs, alphas, scale=3):
    """one training step of m without and with ref = the median -> (sr, param grads, d_lrs[, d_ref]) of each, numpy"""
    cot = util.dev(_cot(lrs.shape[0], lrs.shape[2], scale))
    out = []
    for with_ref in (False, True):
        m.zero_grad(set_to_none=True)
        x, a = util.dev(lrs).requires_grad_(True), util.dev(alphas).requires_grad_(True)
        ref = _median(x.detach()).requires_grad_(True) if with_ref else None
        sr = m(x, a, ref=ref) if with_ref else m(x, a)
        assert sr.requires_grad
        (sr * cot).sum().backward()
        out.append((sr.detach(), {k: p.grad.clone() for k, p in m.named_parameters()}, x.grad.cpu().numpy(),
                    None if a.grad is None else a.grad.clone(), None if ref is None else (ref.detach().cpu().numpy(), ref.grad.cpu().numpy())))
    return out


def _assert_identity(plain, withref, lrs):
    sr0, g0, dl0, da0, _ = plain
    sr1, g1, dl1, da1, (med, d_ref) = withref
    assert torch.equal(sr0, sr1)
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k
    assert (da0 is None) == (da1 is None) and (da0 is None or torch.equal(da0, da1))
    # d_lrs: the plain path routes the frame's gradient to the view the median picked; one fp32 add, possibly associated differently
    want = dl1.copy()
    first = _first_tied(lrs, med)
    np.put_along_axis(want, first[:, None], np.take_along_axis(want, first[:, None], 1) + d_ref[:, None], 1)
    err = float(np.abs(dl0 - want).max())
    print(f"max |d_lrs_plain - (d_lrs_ref + routed d_ref)| = {err:.3e} of max |d_lrs| {np.abs(dl0).max():.3e}")
    assert err <= 4 * 2.0 ** -24 * float(np.abs(dl0).max())
    assert np.abs(d_ref).max() > 0


@pytest.mark.parametrize("V", [1, 4, 5])
@pytest.mark.parametrize("prec", PRECS)
def test_identity_training(prec, V):
    lrs, alphas = _batch(V)
    m = _fresh_model(True, precision=prec)
    m.train_precision = prec
    plain, withref = _train_pair(m, lrs, alphas)
    _assert_identity(plain, withref, lrs)


@pytest.mark.parametrize("prec", PRECS)
def test_identity_at_scale_2(prec):
    lrs, alphas = _batch(4)
    m = _model(2, precision=prec, train=True)
    m.train_precision = prec
    plain, withref = _train_pair(m, lrs, alphas, scale=2)
    _assert_identity(plain, withref, lrs)
    m.eval()
    with torch.no_grad():
        x, a = util.dev(lrs), util.dev(alphas)
        assert torch.equal(m(x, a, ref=_median(x)), m(x, a))


def test_lazy_bf16_training_with_ref_is_refused_clearly():
    lrs, alphas = _batch(4)
    m = _fresh_model(True, precision="bf16")
    x = util.dev(lrs)
    with pytest.raises(NotImplementedError, match="train_precision"):
        m(x, util.dev(alphas), ref=_median(x))


# ----------------------------------------------------------------------------- independence
_indep = {}


def _masked_case():
    """(lrs, alphas, masks, ref, filled): a (2, 5, 16, 16) batch, ~60 % clear masks, ref = the masked composite; made once, shared.
    The network is given the views as they are (lrs) with that frame: the median of the FILLED views is the composite again wherever the
    real views fill the median's window, so only the unfilled views tell the two frames apart."""
    if not _indep:
        lrs, alphas = _batch(5, seed=11)
        masks = (np.random.Generator(np.random.PCG64(4)).random(lrs.shape) < 0.6).astype(np.float32)
        ref, _, filled = R.masked_composite(lrs, masks, alphas, 9)
        assert not np.array_equal(ref, O.reference_frame(lrs))
        _indep["case"] = (lrs, alphas, masks, ref, filled)
    return _indep["case"]


@pytest.mark.parametrize("prec", PRECS)
def test_forward_with_a_composite_frame_vs_the_oracle_stages(prec):
    from hrnet_hip import composite
    lrs, alphas, masks, ref, filled = _masked_case()
    if "sr" not in _indep:
        st = weights.hrnet_state(1234)
        b, v, h, w = lrs.shape
        f64, r64 = lrs.astype(np.float64), ref.astype(np.float64)
        stacked = np.stack([f64, np.broadcast_to(r64[:, None], f64.shape)], axis=2).reshape(b * v, 2, h, w)
        emb = O.encoder(stacked, st, 2).reshape(b, v, -1, h, w)
        _indep["sr"] = O.decoder(O.fuse(emb, alphas.astype(np.float64), st, True), st)
    g_ref, g_filled = composite.masked_composite(util.dev(lrs), util.dev(masks), util.dev(alphas))
    assert np.array_equal(g_ref.cpu().numpy(), ref) and np.array_equal(g_filled.cpu().numpy(), filled)
    m = util.hip_hrnet(prec)
    with torch.no_grad():
        got = m(util.dev(lrs), util.dev(alphas), ref=g_ref)
        plain = m(util.dev(lrs), util.dev(alphas))
    print(f"{prec}: max-rel vs the oracle stages {util.rel_err(got.cpu().numpy(), _indep['sr']):.3e}")
    util._check(prec, got.cpu().numpy(), _indep["sr"])
    assert not torch.equal(got, plain)


def _torch_forward(lrs, alphas, ref, st, alpha_residual=True, num_layers=2):
    """HRNet.forward (HRNet.py:186-211) with `ref` (B,H,W) in the median's place, in torch (fp64 when its inputs are)"""
    b, v, h, w = lrs.shape
    x = torch.stack([lrs, ref[:, None].expand(-1, v, -1, -1)], 2).reshape(b * v, 2, h, w)
    x = torch_port._prelu(F.conv2d(x, st["encode.init_layer.0.weight"], st["encode.init_layer.0.bias"], padding=1), st,
                          "encode.init_layer.1.weight")
    for i in range(num_layers):
        x = torch_port._res_block(x, st, f"encode.res_layers.{i}")
    x = F.conv2d(x, st["encode.final.0.weight"], st["encode.final.0.bias"], padding=1).reshape(b, v, 64, h, w)
    n = v
    while n // 2 > 0:
        parity, half = n % 2, n // 2
        alice, bob = x[:, :half], x[:, half:n - parity].flip(1)
        z = torch_port._res_block(torch.cat([alice, bob], 2).reshape(b * half, 128, h, w), st, "fuse.fuse.0")
        f = torch_port._prelu(F.conv2d(z, st["fuse.fuse.1.weight"], st["fuse.fuse.1.bias"], padding=1), st, "fuse.fuse.2.weight")
        f = f.reshape(b, half, 64, h, w)
        x, n = (alice + alphas[:, half:n - parity].flip(1).reshape(b, half, 1, 1, 1) * f if alpha_residual else f), half
    return util._decode_s(x.mean(1), st, 3)


def _small_case():
    """A (1, 3, 8, 8) batch with its masked composite, chosen by its fp64 forward alone: no PReLU pre-activation within 1e-5 of its
    tensor's max-norm of zero (asserted where it is used).  The fp32 forward is ~2e-6 from fp64, so no activation can take the other
    PReLU branch on the device, which at the default slopes would move a gradient behind it by O(1) - see
    tests/test_gpu_backward.test_hrnet_backward_vs_autograd_oracle; at (2, 5, 16, 16) there are always a few within 1e-6."""
    lrs, alphas, _ = synth.make_batch(648, 1, 3, 8, 3)
    masks = (np.random.Generator(np.random.PCG64(648)).random(lrs.shape) < 0.6).astype(np.float32)
    ref = R.masked_composite(lrs, masks, alphas, 9)[0]
    assert not np.array_equal(ref, O.reference_frame(lrs))
    return lrs, alphas, ref


def _ragged_case():
    """A (2, 3, 17, 50) batch (a 50 x 50 scene cut down; the second sample's last view is padding) with its masked composite: no strip,
    tile or segment size of the backward divides the frame, and the stem's data gradient runs two tile columns by three tile rows"""
    lrs, alphas, _ = synth.make_batch(1750, 2, 3, 50, [3, 2])
    lrs = np.ascontiguousarray(lrs[:, :, :17, :])
    masks = (np.random.Generator(np.random.PCG64(1750)).random(lrs.shape) < 0.6).astype(np.float32)
    ref = R.masked_composite(lrs, masks, alphas, 9)[0]
    assert lrs.shape == (2, 3, 17, 50) and not np.array_equal(ref, O.reference_frame(lrs))
    return lrs, alphas, ref


@pytest.mark.parametrize("prec,slopes_at_1,small", [("fp32", False, True), ("fp32", True, False), ("bf16x3", True, False),
                                                    ("fp32", True, "ragged"), ("bf16x3", True, "ragged")])
def test_gradients_with_a_composite_frame_vs_fp64_autograd(prec, slopes_at_1, small):
    """The kernels are pinned at (2, 5, 16, 16) with every PReLU slope at 1, where nothing can flip (as tests/test_gpu_input_grad.py does
    for bf16x3 and for fp32 at V = 32); the default slopes, PReLU backward included, on the small case no activation of which can flip;
    and with every slope at 1 again at (2, 3, 17, 50), where the frame is wider than one 32-column tile and ragged in both directions
    (hrn_hrnet_forward_train_ref / hrn_hrnet_backward_ref through their dispatcher op: HRNet.forward itself refuses a frame that is not square)."""
    if small == "ragged":
        lrs, alphas, ref = _ragged_case()
    elif small:
        lrs, alphas, ref = _small_case()
    else:
        lrs, alphas, _, ref, _ = _masked_case()
    slopes = {k: 1.0 for k in _SLOPE_KEYS} if slopes_at_1 else None
    cot = _cot(lrs.shape[0], lrs.shape[2], W=lrs.shape[3])
    st = {k: v.double().requires_grad_(True) for k, v in _state(3, slopes=slopes).items()}
    tx = torch.from_numpy(lrs).double().requires_grad_(True)
    ta = torch.from_numpy(alphas).double().requires_grad_(True)
    tr = torch.from_numpy(ref).double().requires_grad_(True)
    nearest = [1.0]
    real_prelu = torch_port._prelu

    def prelu(t, st_, key):
        mag = t.detach().abs()
        nearest[0] = min(nearest[0], float(mag.min() / mag.max()))
        return real_prelu(t, st_, key)

    try:
        torch_port._prelu = prelu
        with torch.enable_grad():
            want_sr = _torch_forward(tx, ta, tr, st)
            (want_sr * torch.from_numpy(cot).double()).sum().backward()
    finally:
        torch_port._prelu = real_prelu
    assert slopes_at_1 or nearest[0] >= 1e-5, nearest
    m = _fresh_model(True, precision=prec, slopes=slopes)
    x, a, r = util.dev(lrs).requires_grad_(True), util.dev(alphas).requires_grad_(True), util.dev(ref).requires_grad_(True)
    if small == "ragged":
        # the module's forward takes square frames only (the reference's .view()); the training op behind it takes any, and is called
        # here exactly as HRNet._forward_ref calls it
        from hrnet_hip import binding
        dt = m._train_dtype()
        dt = m._dtype() if dt is None else dt
        assert [k for k, _ in m.named_parameters()] == binding.hrnet_param_names(m._num_layers)
        sr, _ = torch.ops.hrnet_hip.hrnet_forward_train_ref(m._packed_for(dt), x.float().contiguous(), a.float().contiguous(),
                                                            binding._ref_frame(r, x), [p for _, p in m.named_parameters()], m._num_layers,
                                                            bool(m.fuse.alpha_residual), dt, m._scale)
    else:
        sr = m(x, a, ref=r)
    (sr * util.dev(cot)).sum().backward()
    tol = 2e-4                                                  # tests/test_gpu_input_grad.py: d lrs, of the max-norm
    e_sr = util.rel_err(sr.detach().cpu().numpy(), want_sr.detach().numpy())
    e_lrs, e_ref = util.rel_err(x.grad.cpu().numpy(), tx.grad.numpy()), util.rel_err(r.grad.cpu().numpy(), tr.grad.numpy())
    e_par = {k: util.rel_err(p.grad.cpu().numpy(), st[k].grad.numpy()) for k, p in m.named_parameters()}
    worst = max(e_par, key=e_par.get)
    print(f"{prec}: sr {e_sr:.2e}, d_lrs {e_lrs:.2e}, d_ref {e_ref:.2e}, d_alphas {util.rel_err(a.grad.cpu().numpy(), ta.grad.numpy()):.2e}, "
          f"worst parameter gradient {worst} {e_par[worst]:.2e}; all: " + ", ".join(f"{k} {e:.1e}" for k, e in e_par.items()))
    assert tuple(r.grad.shape) == ref.shape and tuple(x.grad.shape) == lrs.shape
    assert e_lrs <= tol, e_lrs
    assert e_ref <= tol, e_ref
    for k, e in e_par.items():
        assert e <= tol, (k, e)


# ----------------------------------------------------------------------------- frozen
@pytest.mark.parametrize("prec", PRECS)
def test_frozen_parameters_only_the_frame_wants_a_gradient(prec):
    lrs, alphas, _, ref, filled = _masked_case()
    cot = util.dev(_cot(2, 16))
    m = _fresh_model(True, precision=prec)
    m.train_precision = prec
    x, a = util.dev(filled), util.dev(alphas)
    r = util.dev(ref).requires_grad_(True)
    (m(x, a, ref=r) * cot).sum().backward()
    full = r.grad.clone()
    m.zero_grad(set_to_none=True)
    m.requires_grad_(False)
    r = util.dev(ref).requires_grad_(True)
    sr = m(x, a, ref=r)
    assert sr.requires_grad
    counts, _ = kt._launches(lambda: (sr * cot).sum().backward())
    assert torch.equal(r.grad, full) and float(full.abs().max()) > 0
    assert all(p.grad is None for p in m.parameters()) and x.grad is None and a.grad is None
    assert counts["conv_wgrad_f32"] == 0 and counts["stem_wgrad"] == 0 and counts["bias_finish"] == 0 and counts["slope_finish"] == 0, counts
    assert counts.get("prof:stem_dgrad_ref") == 1 and "prof:stem_dgrad_route" not in counts and "prof:median9" not in counts, counts


# ----------------------------------------------------------------------------- tiled and ensemble
def _tiling_model(scale, precision):
    from DeepNetworks.HRNet import HRNet
    cfg = copy.deepcopy(weights.HRNET_CONFIG)
    cfg["decoder"]["deconv"]["kernel_size"] = cfg["decoder"]["deconv"]["stride"] = scale
    m = HRNet(cfg)
    m.load_state_dict(_state(scale))
    m.precision = precision
    return m.cuda().eval()


@pytest.mark.parametrize("prec", PRECS)
def test_tiled_with_ref_equals_the_whole_frame(prec):
    """(2, 4, 56, 56) in tiles of 32: the smallest square scene of tests/test_gpu_tiled.py"""
    lrs, alphas, _ = synth.make_batch(304 + 56, 2, 4, 56, 4)
    x, a = util.dev(lrs), util.dev(alphas)
    masks = util.dev((np.random.Generator(np.random.PCG64(8)).random(lrs.shape) < 0.6).astype(np.float32))
    from hrnet_hip import composite
    ref, filled = composite.masked_composite(x, masks, a)
    m = _tiling_model(3, prec)
    with torch.no_grad():
        whole = m(filled, a, ref=ref)
        assert not torch.equal(whole, m(filled, a, ref=ref + 0.125))         # the frame is read
        for wpp in (1, None):
            assert torch.equal(m.forward_tiled(filled, a, 32, windows_per_pass=wpp, ref=ref), whole)
        m.tile = 32
        assert torch.equal(m(filled, a, ref=ref), whole)
        m.tile = None
        # one window: straight to the op
        assert torch.equal(m.forward_tiled(filled, a, 56, ref=ref), whole)
        # with the ensemble: forward_ensemble of the whole frame
        want = m.forward_ensemble(filled, a, "flip", ref=ref)
        assert torch.equal(m.forward_tiled(filled, a, 32, ensemble="flip", members_per_pass=3, ref=ref), want)


@pytest.mark.parametrize("prec", PRECS)
def test_ensemble_with_ref_is_the_mean_over_members_given_the_transformed_frame(prec):
    """(2, 4, 32, 32): the scene of tests/test_gpu_ensemble.py"""
    lrs, alphas, _ = synth.make_batch(63, 2, 4, 32, [4, 3])
    x, a = util.dev(lrs), util.dev(alphas)
    masks = util.dev((np.random.Generator(np.random.PCG64(9)).random(lrs.shape) < 0.6).astype(np.float32))
    from hrnet_hip import composite
    ref, filled = composite.masked_composite(x, masks, a)
    m = _tiling_model(3, prec)
    for mode in ("dihedral", "flip"):
        codes = augment.ensemble_codes(mode)
        with torch.no_grad():
            members = torch.stack([m(augment.apply(filled, c).contiguous(), a, ref=augment.apply(ref, c).contiguous()) for c in codes])
            want = augment.mean_inverse(members, codes)
            got = m.forward_ensemble(filled, a, mode, ref=ref)
            assert torch.equal(got, want), (mode, float((got - want).abs().max()))
            assert torch.equal(m.forward_ensemble(filled, a, mode, members_per_pass=3, ref=ref), want)
    with torch.no_grad():
        m.ensemble = "flip"
        assert torch.equal(m(filled, a, ref=ref), m.forward_ensemble(filled, a, "flip", ref=ref))
        assert not torch.equal(m(filled, a, ref=ref), m(filled, a))
        m.ensemble = None


# ----------------------------------------------------------------------------- end to end
def test_register_composite_train_step():
    """loader -> register_views -> masked_composite -> training forward -> cl1_loss, one (2, 6, 32, 32) batch"""
    from hrnet_hip import composite, losses, registration
    lrs, alphas, hrs = synth.make_batch(21, 2, 6, 32, [6, 4])
    rng = np.random.Generator(np.random.PCG64(2))
    masks = (rng.random(lrs.shape) < 0.7).astype(np.float32)
    maps = (rng.random(hrs.shape) > 0.1).astype(np.float32)
    x, a, mk, h, mp = (util.dev(t) for t in (lrs, alphas, masks, hrs, maps))

    def step(with_ref):
        m = _fresh_model(True)
        registered, valid, _ = registration.register_views(x, mk)
        ref, filled = composite.masked_composite(registered, valid, a)
        sr = m(filled, a, ref=ref) if with_ref else m(filled, a)
        loss = losses.cl1_loss(sr[:, 0], h, mp).mean()
        loss.backward()
        return loss.detach(), {k: p.grad.clone() for k, p in m.named_parameters()}

    l1, g1 = step(True)
    l2, g2 = step(True)
    l0, _ = step(False)
    assert bool(torch.isfinite(l1)) and all(bool(torch.isfinite(g).all()) for g in g1.values())
    assert torch.equal(l1, l2) and all(torch.equal(g1[k], g2[k]) for k in g1)
    assert not torch.equal(l1, l0)


# ----------------------------------------------------------------------------- dispatcher
def test_opcheck():
    from hrnet_hip import binding
    ops = torch.ops.hrnet_hip
    lrs, alphas = _batch(4, S=8)
    x, a = util.dev(lrs), util.dev(alphas)
    ref = _median(x) + 0.01
    m = _fresh_model(True)
    params = [p for _, p in m.named_parameters()]
    pk = m._packed_f32()
    torch.library.opcheck(ops.hrnet_forward_ref.default, (pk, binding.F32, 2, True, x, a, ref, 3), test_utils=("test_schema", "test_faketensor"))
    full = ("test_schema", "test_faketensor", "test_autograd_registration")
    for r in (ref, ref.clone().requires_grad_(True)):
        torch.library.opcheck(ops.hrnet_forward_train_ref.default, (pk, x, a, r, params, 2, True, binding.F32, 3), test_utils=full)
    _, tws = ops.hrnet_forward_train_ref(pk, x, a, ref, params, 2, True, binding.F32, 3)
    d = torch.randn((2, 1, 24, 24), device="cuda")
    det = [p.detach() for p in params]
    need = [i % 2 == 0 for i in range(len(params))]
    for args in ((need, True, True, True), ([False] * len(params), False, False, True), ([True] * len(params), True, False, False)):
        torch.library.opcheck(ops.hrnet_backward_ref.default, (pk, det, x, a, ref, d, tws, 2, True, binding.F32, 3) + args,
                              test_utils=("test_schema", "test_faketensor"))
