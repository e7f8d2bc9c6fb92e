"""GPU (-m gpu): HRNet at upscale factors x2 / x4 (decoder.deconv kernel_size == stride == S, src/DeepNetworks/HRNet.py:147-156).

Oracle: `util._hrnet_forward_s`, oracle/torch_port.hrnet_forward restated with the decoder's stride as a parameter (built from
the port's own helpers), run in float64 on the CPU.  It is first pinned to torch_port.hrnet_forward at S = 3.  Bounds are those of
test_gpu_parity.py (forward) and test_gpu_backward.py (gradients, train step).  At S = 3 every scale-taking entry point must give
the very bits of the entry point it generalises."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import synth, torch_port, weights
import util
from util import _decode_s, _hrnet_forward_s, _model, _state

pytestmark = pytest.mark.gpu

FP32_REL, X3_REL, BF16_REL, BF16_PSNR = 2e-5, 1e-4, 2.5e-2, 45.0
_SLOPE_KEYS = [k for k, shape in weights.HRNET_SHAPES if shape == (1,) and k.endswith(".weight")]


def _check(got, want, prec):
    e = util.rel_err(got, want)
    if prec == "fp32":
        assert e <= FP32_REL, e
    elif prec == "bf16x3":
        assert e <= X3_REL, e
    else:
        ps = util.psnr_db(got, want)
        assert e <= BF16_REL and ps >= BF16_PSNR, (e, ps)


def test_restatement_matches_the_port_at_x3():
    lrs, alphas, _ = synth.make_batch(5, 2, 5, 16, 4)
    st = {k: v.double() for k, v in _state(3).items()}
    x, a = torch.from_numpy(lrs).double(), torch.from_numpy(alphas).double()
    for ar in (True, False):
        want = torch_port.hrnet_forward(x, a, st, num_layers=2, alpha_residual=ar)
        with torch.no_grad():
            got = _hrnet_forward_s(x, a, st, 2, ar, scale=3)
        assert torch.equal(got, want)


@pytest.mark.parametrize("B,V,S,n_real,alpha_residual", [
    (2, 5, 16, 4, True),        # odd view count, one padded view
    (2, 4, 20, 4, False),       # alpha_residual = false; N*H*W = 800, not a multiple of the decoder's 256-pixel workgroup
    (1, 1, 24, 1, True),        # a single view: no fusion level
])
@pytest.mark.parametrize("prec", ["fp32", "bf16", "bf16x3"])
@pytest.mark.parametrize("scale", [2, 4])
def test_forward_vs_oracle(scale, prec, B, V, S, n_real, alpha_residual):
    lrs, alphas, _ = synth.make_batch(11, B, V, S, n_real)
    st = {k: v.double() for k, v in _state(scale).items()}
    with torch.no_grad():
        want = _hrnet_forward_s(torch.from_numpy(lrs).double(), torch.from_numpy(alphas).double(), st, 2, alpha_residual, scale).numpy()
    m = _model(scale, prec, alpha_residual)
    with torch.no_grad():
        got = m(util.dev(lrs), util.dev(alphas))
    assert tuple(got.shape) == (B, 1, scale * S, scale * S)
    _check(got.cpu().numpy(), want, prec)


@pytest.mark.parametrize("prec", ["fp32", "bf16", "bf16x3"])
@pytest.mark.parametrize("scale", [2, 4])
def test_decode_state_vs_oracle(scale, prec):
    """Decoder.forward alone (HRNet.py:158-169) on the fused state the device produced, in its storage precision."""
    lrs, alphas, _ = synth.make_batch(13, 3, 4, 20, 4)
    m = _model(scale, prec)
    with torch.no_grad():
        fused = m.fuse_views(m.encode_views(util.dev(lrs)), util.dev(alphas))
        got = m.decode_state(fused)
    x = torch.from_numpy(util.nhwc_to_nchw(fused, prec)).double()
    st = {k: v.double() for k, v in _state(scale).items()}
    with torch.no_grad():
        want = _decode_s(x, st, scale).numpy()
    assert tuple(got.shape) == (3, 1, 20 * scale, 20 * scale)
    _check(got.cpu().numpy(), want, "fp32" if prec == "bf16x3" else prec)      # bf16x3 decodes on the fp32 kernel


# ----------------------------------------------------------------------------- x3 through the new entry points: the same bits
def _raw_forward(lib, packed, dt, scale, lrs, alphas, nl=2):
    from hrnet_hip import binding
    B, V, H, W = lrs.shape
    ws = torch.empty(lib.hrn_hrnet_workspace_bytes(dt, B, V, H, W), dtype=torch.uint8, device="cuda")
    sr = torch.full((B, 1, 3 * H, 3 * W), float("nan"), device="cuda")
    p = binding._ptr
    if scale is None:
        rc = lib.hrn_hrnet_forward(p(packed), dt, nl, 1, p(lrs), p(alphas), B, V, H, W, p(sr), p(ws), ws.numel(), None)
    else:
        rc = lib.hrn_hrnet_forward_s(p(packed), dt, nl, scale, 1, p(lrs), p(alphas), B, V, H, W, p(sr), p(ws), ws.numel(), None)
    assert rc == 0, lib.hrn_last_error()
    torch.cuda.synchronize()
    return sr


@pytest.mark.parametrize("dt", [0, 1, 2])
def test_x3_forward_bits_unchanged(dt):
    from hrnet_hip import binding
    lib = binding.load_library()
    lrs, alphas, _ = synth.make_batch(17, 2, 5, 20, 4)
    x, a = util.dev(lrs), util.dev(alphas)
    named = {k: v.cuda() for k, v in _state(3).items()}
    P, keep = binding.hrnet_param_struct(named, 2)
    blobs = []
    for pack_s in (False, True):
        n = lib.hrn_hrnet_packed_bytes(dt, 2)
        blob = torch.zeros(n, dtype=torch.uint8, device="cuda")
        rc = (lib.hrn_hrnet_pack_s(ctypes.byref(P), dt, 3, binding._ptr(blob), n, None) if pack_s
              else lib.hrn_hrnet_pack(ctypes.byref(P), dt, binding._ptr(blob), n, None))
        assert rc == 0
        blobs.append(blob)
    torch.cuda.synchronize()
    assert torch.equal(blobs[0], blobs[1])
    old = _raw_forward(lib, blobs[0], dt, None, x, a)
    new = _raw_forward(lib, blobs[0], dt, 3, x, a)
    assert torch.equal(old, new) and bool(torch.isfinite(new).all())
    # the decoder stage on its own
    m = _model(3, {0: "fp32", 1: "bf16", 2: "bf16x3"}[dt])
    with torch.no_grad():
        fused = m.fuse_views(m.encode_views(x), a)
    N, H, W = fused.shape[-4:-1]
    outs = []
    for scale in (None, 3):
        sr = torch.full((N, 1, 3 * H, 3 * W), float("nan"), device="cuda")
        p = binding._ptr
        rc = (lib.hrn_decoder_forward(p(blobs[0]), dt, 2, p(fused), N, H, W, p(sr), None) if scale is None
              else lib.hrn_decoder_forward_s(p(blobs[0]), dt, 2, 3, p(fused), N, H, W, p(sr), None))
        assert rc == 0
        outs.append(sr)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("dt", [0, 2])
def test_x3_training_bits_unchanged(dt):
    """hrn_hrnet_forward_train_dt / hrn_hrnet_backward_dt against the _s forms at scale 3: SR and every gradient bit-identical."""
    from hrnet_hip import binding
    lib = binding.load_library()
    B, V, S = 2, 5, 16
    lrs, alphas, _ = synth.make_batch(19, B, V, S, 4)
    x, a = util.dev(lrs), util.dev(alphas)
    named = {k: v.cuda() for k, v in _state(3).items()}
    packed = binding.hrnet_pack(named, 2, dt)
    P, keep_p = binding.hrnet_param_struct(named, 2)
    cot = util.dev(np.random.Generator(np.random.PCG64(3)).standard_normal((B, 1, 3 * S, 3 * S)).astype(np.float32))
    nbytes = lib.hrn_hrnet_train_workspace_bytes(2, B, V, S, S)
    p = binding._ptr
    results = []
    for use_s in (False, True):
        tws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        sr = torch.full((B, 1, 3 * S, 3 * S), float("nan"), device="cuda")
        grads = {k: torch.zeros_like(v) for k, v in named.items()}
        G, keep_g = binding.hrnet_param_struct(grads, 2)
        if use_s:
            rc = lib.hrn_hrnet_forward_train_s(p(packed), dt, 2, 3, 1, p(x), p(a), B, V, S, S, p(sr), p(tws), nbytes, None)
        else:
            rc = lib.hrn_hrnet_forward_train_dt(p(packed), dt, 2, 1, p(x), p(a), B, V, S, S, p(sr), p(tws), nbytes, None)
        assert rc == 0, lib.hrn_last_error()
        if use_s:
            rc = lib.hrn_hrnet_backward_s(p(packed), dt, 3, ctypes.byref(P), 1, p(x), p(a), B, V, S, S, p(cot), ctypes.byref(G), p(tws),
                                          nbytes, None)
        else:
            rc = lib.hrn_hrnet_backward_dt(p(packed), dt, ctypes.byref(P), 1, p(x), p(a), B, V, S, S, p(cot), ctypes.byref(G), p(tws),
                                           nbytes, None)
        assert rc == 0, lib.hrn_last_error()
        torch.cuda.synchronize()
        results.append((sr, grads))
    (sr0, g0), (sr1, g1) = results
    assert torch.equal(sr0, sr1)
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k
    assert float(g1["decode.deconv.0.weight"].abs().max()) > 0


# ----------------------------------------------------------------------------- gradients at x2 / x4
@pytest.mark.parametrize("B,V,S,n_real,alpha_residual", [(2, 5, 16, 4, True), (1, 4, 20, 4, False), (1, 3, 33, 3, True)])
@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
@pytest.mark.parametrize("scale", [2, 4])
def test_backward_vs_autograd_oracle(scale, prec, B, V, S, n_real, alpha_residual):
    """test_gpu_backward.py::test_hrnet_backward_vs_autograd_oracle's scheme: bf16x3 with every PReLU slope at 1; tensors to 2e-4
    of their max-norm, scalars to 2e-5 of the sum of |terms| of their defining sum."""
    slopes = None if prec == "fp32" else {k: 1.0 for k in _SLOPE_KEYS}
    lrs, alphas, _ = synth.make_batch(23, B, V, S, n_real)
    cot = np.random.Generator(np.random.PCG64(77)).standard_normal((B, 1, scale * S, scale * S)).astype(np.float32)
    st = {k: v.double().requires_grad_(True) for k, v in _state(scale, slopes=slopes).items()}
    abs_terms = {}
    torch_port.ABS_TERMS = abs_terms
    try:
        with torch.enable_grad():
            want_sr = _hrnet_forward_s(torch.from_numpy(lrs).double(), torch.from_numpy(alphas).double(), st, 2, alpha_residual, scale)
            (want_sr * torch.from_numpy(cot).double()).sum().backward()
    finally:
        torch_port.ABS_TERMS = None
    m = _model(scale, prec, alpha_residual, slopes=slopes, train=True)
    sr = m(util.dev(lrs), util.dev(alphas))
    assert sr.requires_grad and tuple(sr.shape) == (B, 1, scale * S, scale * S)
    assert util.rel_err(sr.detach().cpu().numpy(), want_sr.detach().numpy()) <= (2e-5 if prec == "fp32" else 1e-4)
    (sr * util.dev(cot)).sum().backward()
    checked = set()
    for k, p in m.named_parameters():
        got, want = p.grad.cpu().numpy(), st[k].grad.numpy()
        if p.numel() == 1:
            bound = 2e-5 * abs_terms.get(k, 0.0) + 1e-12
            assert abs(float(got.ravel()[0]) - float(want.ravel()[0])) <= bound, (k, got, want, abs_terms.get(k))
        else:
            assert util.rel_err(got, want) <= 2e-4, (k, util.rel_err(got, want))
        checked.add(k)
    assert {"decode.deconv.0.weight", "decode.deconv.0.bias", "decode.deconv.1.weight", "decode.final.weight",
            "decode.final.bias"} <= checked


# ----------------------------------------------------------------------------- one training step at x2
def test_x2_train_step_vs_autograd_oracle():
    """src/train.py:172-191 at x2 with 64 x 64 LR patches, whose 128 x 128 SR is ShiftNet's input as it stands: HRNet -> ShiftNet
    registration -> Lanczos -> get_loss (cPSNR, crop 3) -> FusedAdam, against the same chain in fp64 torch on the CPU (the tolerances
    of test_gpu_backward.py::test_full_train_step_vs_autograd_oracle)."""
    from DeepNetworks.ShiftNet import ShiftNet
    from hrnet_hip import losses
    from hrnet_hip.optim import FusedAdam
    B, V, S, scale, lam, lr = 2, 4, 64, 2, 1e-6, 1e-4
    s2 = scale * S
    lrs, alphas, _ = synth.make_batch(31, B, V, S, V)
    rng = np.random.Generator(np.random.PCG64(5))
    hrs = rng.random((B, s2, s2), dtype=np.float32)
    maps = (rng.random((B, s2, s2)) > 0.1).astype(np.float32)
    crop = np.ones((s2, s2), np.float32)
    crop[:3] = 0; crop[-3:] = 0; crop[:, :3] = 0; crop[:, -3:] = 0
    mask = rng.random((B, 32768)) >= 0.5
    hstate = _state(scale)
    sstate = weights.to_torch_state(weights.shiftnet_state(4321))

    # ---- oracle chain, fp64 on the CPU
    hst = {k: v.double().requires_grad_(True) for k, v in hstate.items()}
    sst = {k: v.double().requires_grad_("running" not in k and "num_batches" not in k) for k, v in sstate.items()}
    t_hrs = torch.from_numpy(hrs).double()
    with torch.enable_grad():
        srs = _hrnet_forward_s(torch.from_numpy(lrs).double(), torch.from_numpy(alphas).double(), hst, 2, True, scale)
        pairs = torch.cat([t_hrs.reshape(-1, 1, s2, s2), srs], 1)
        shifts = torch_port.shiftnet_forward_train(pairs, sst, torch.from_numpy(mask).double())[:, None]
        shifted = torch_port.lanczos_shift(srs.reshape(-1, 1, s2, s2).transpose(0, 1), shifts.reshape(-1, 2).flip(-1))[0]
        loss = -torch_port.registered_loss_cpsnr(shifted, t_hrs, torch.from_numpy(crop * maps).double())
        loss = loss.mean() + lam * shifts.mean() ** 2
        loss.backward()

    # ---- HIP modules, the statements of train.py
    fusion = _model(scale, "fp32", train=True)
    regis = ShiftNet()
    regis.load_state_dict(sstate)
    regis = regis.cuda().train()
    opt = FusedAdam(list(fusion.parameters()) + list(regis.parameters()), lr=lr)
    opt.zero_grad()
    d_lrs, d_alphas, d_hrs = util.dev(lrs), util.dev(alphas), util.dev(hrs)
    dmask = torch.from_numpy(mask.astype(np.uint8)).cuda()
    orig_rand = torch.rand
    try:
        torch.rand = lambda *a, **k: (dmask.float() * 0.75 + 0.125).reshape(a[0]) if a and tuple(a[0]) == (B, 32768) else orig_rand(*a, **k)
        g_srs = fusion(d_lrs, d_alphas)
        assert tuple(g_srs.shape) == (B, 1, 128, 128)
        g_shifts = torch.stack([regis(torch.cat([d_hrs.reshape(-1, 1, s2, s2), g_srs], 1))], 1)
        g_shifted = regis.transform(g_shifts.view(-1, 2), g_srs.view(-1, 1, s2, s2), device="cuda").view(-1, 1, s2, s2)[:, 0]
    finally:
        torch.rand = orig_rand
    g_loss = -losses.get_loss(g_shifted, d_hrs, util.dev(maps), metric="cPSNR", crop=3)
    g_loss = g_loss.mean() + lam * g_shifts.mean() ** 2
    g_loss.backward()
    want_loss = float(loss.detach())
    assert abs(float(g_loss.detach()) - want_loss) <= 2e-4 * abs(want_loss)
    assert util.rel_err(g_shifts.detach().cpu().numpy(), shifts.detach().numpy()) <= 1e-3
    scalar_scale = max(float(np.abs(hst[k].grad.numpy()).max()) for k, p in fusion.named_parameters()
                       if p.numel() == 1 and k != "decode.final.bias")
    before, grads = {}, {}
    for k, p in fusion.named_parameters():
        got, ref = p.grad.cpu().numpy(), hst[k].grad.numpy()
        before[k], grads[k] = p.detach().clone(), p.grad.detach().clone()
        if k == "decode.final.bias":            # zero by construction under the brightness correction: rounding noise on both sides
            continue
        if p.numel() == 1:
            assert abs(float(got.ravel()[0]) - float(ref.ravel()[0])) <= 2e-2 * scalar_scale, (k, got, ref)
        else:
            assert util.rel_err(got, ref) <= 2e-2, (k, util.rel_err(got, ref))
    # the optimiser step (train.py:191) moves the x2 decoder like torch.optim.Adam would with the same gradients
    opt.step()
    for k, p in fusion.named_parameters():
        ref_p = before[k].clone().requires_grad_(True)
        ref_p.grad = grads[k]
        torch.optim.Adam([ref_p], lr=lr).step()
        assert torch.allclose(p.detach(), ref_p.detach(), rtol=2e-5, atol=1e-7), k
    with torch.no_grad():
        assert bool(torch.isfinite(fusion.eval()(d_lrs, d_alphas)).all())


def test_opcheck_at_x2():
    """The three HRNet ops with scale = 2: schema, fake (meta) shapes, autograd registration."""
    from hrnet_hip import binding
    ops = torch.ops.hrnet_hip
    lrs, alphas = synth.fast_batch(5, 2, 4, 16)
    x, a = util.dev(lrs), util.dev(alphas)
    m = _model(2, "fp32")
    packed, dt = m.packed_parameters()
    torch.library.opcheck(ops.hrnet_forward.default, (packed, dt, 2, True, x, a, 2), test_utils=("test_schema", "test_faketensor"))
    with torch.no_grad():
        assert tuple(ops.hrnet_forward(packed, dt, 2, True, x, a, 2).shape) == (2, 1, 32, 32)
    params = [p for _, p in m.named_parameters()]
    p32 = m._packed_f32()
    full = ("test_schema", "test_faketensor", "test_autograd_registration")
    torch.library.opcheck(ops.hrnet_forward_train.default, (p32, x, a, params, 2, True, binding.F32, 2), test_utils=full)
    sr, tws = ops.hrnet_forward_train(p32, x, a, params, 2, True, binding.F32, 2)
    assert tuple(sr.shape) == (2, 1, 32, 32)
    torch.library.opcheck(ops.hrnet_backward.default, (p32, [p.detach() for p in params], x, a, torch.rand_like(sr), tws, 2, True,
                                                       binding.F32, 2), test_utils=("test_schema", "test_faketensor"))
