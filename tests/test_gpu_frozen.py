"""GPU (-m gpu): frozen parameters (`requires_grad_(False)`) in HRNet and ShiftNet, through hrn_hrnet_backward_sel /
hrn_shiftnet_backward_sel and the registered ops hrnet_backward_sel / shiftnet_backward_sel.

1. Bit-identity: with part of a model frozen, every gradient autograd still asks for (parameters, d lrs, d alphas, ShiftNet's d x) is
   torch.equal to the one of the same step with everything trainable, and a frozen parameter's .grad stays None.
2. The work is really skipped: the host-side launch counters (hrn_kt_launch_count) and the built-in profiler show no launch of what
   nothing downstream reads, and the all-trainable step launches exactly what the entry points of the parent release launch.
"""
import copy

import numpy as np
import pytest
import torch

from oracle import weights
from kt import _launches
from util import _state

pytestmark = pytest.mark.gpu

PRECS = ("fp32", "bf16", "bf16x3")
PATTERNS = {
    "encoder": lambda k: k.startswith("encode."),
    "encoder+fuse": lambda k: k.startswith(("encode.", "fuse.")),
    "decoder": lambda k: k.startswith("decode."),
    "hrnet+inputs": lambda k: True,
    "one_slope": lambda k: k == "fuse.fuse.2.weight",
}


def _hrnet(scale, prec, alpha_residual=True):
    from DeepNetworks.HRNet import HRNet
    cfg = copy.deepcopy(weights.HRNET_CONFIG)
    cfg["decoder"]["deconv"]["kernel_size"] = cfg["decoder"]["deconv"]["stride"] = scale
    cfg["recursive"]["alpha_residual"] = alpha_residual
    m = HRNet(cfg)
    m.load_state_dict(_state(scale))
    m.train_precision = prec
    return m.cuda().train()


def _inputs(B, V, H, scale, seed=3):
    rng = np.random.Generator(np.random.PCG64(seed))
    lrs = torch.from_numpy(rng.random((B, V, H, H), dtype=np.float32)).cuda()
    alphas = torch.from_numpy((rng.random((B, V)) > 0.3).astype(np.float32)).cuda()
    cot = torch.from_numpy(rng.standard_normal((B, 1, scale * H, scale * H)).astype(np.float32)).cuda()
    return lrs, alphas, cot


def _hrnet_step(scale, prec, frozen, inputs_grad, alpha_residual=True, B=2, V=5, H=16):
    """One forward + backward of (sr * cot).sum() -> ({name: .grad}, d lrs, d alphas)."""
    m = _hrnet(scale, prec, alpha_residual)
    for k, p in m.named_parameters():
        p.requires_grad_(not frozen(k))
    lrs, alphas, cot = _inputs(B, V, H, scale)
    lrs.requires_grad_(inputs_grad)
    alphas.requires_grad_(inputs_grad)
    (m(lrs, alphas) * cot).sum().backward()
    return {k: p.grad for k, p in m.named_parameters()}, lrs.grad, alphas.grad


def _assert_same(frozen, got, want):
    g, gl, ga = got
    w, wl, wa = want
    for k in w:
        if frozen(k):
            assert g[k] is None, k
        else:
            assert g[k] is not None and torch.equal(g[k], w[k]), k
    for a, b in ((gl, wl), (ga, wa)):
        assert (a is None) == (b is None)
        if a is not None:
            assert torch.equal(a, b)


# ----------------------------------------------------------------------------- 1. bit-identity
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("scale", [2, 3])
@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_frozen_hrnet_gradients_equal_the_full_backward(prec, scale, pattern):
    frozen = PATTERNS[pattern]
    inputs_grad = pattern == "hrnet+inputs"
    want = _hrnet_step(scale, prec, lambda k: False, inputs_grad)
    got = _hrnet_step(scale, prec, frozen, inputs_grad)
    _assert_same(frozen, got, want)
    if inputs_grad:
        assert got[1] is not None and got[2] is not None and float(got[2].abs().sum()) > 0


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("pattern", ["encoder", "encoder+fuse", "hrnet+inputs"])
def test_frozen_hrnet_without_alpha_residual_even_views_scale4(prec, pattern):
    """No alpha residual (alphas get no gradient, and d_alphas asks for no fusion data gradient), V even, scale 4."""
    frozen = PATTERNS[pattern]
    inputs_grad = pattern == "hrnet+inputs"
    kw = dict(alpha_residual=False, V=4, H=12)
    want = _hrnet_step(4, prec, lambda k: False, inputs_grad, **kw)
    got = _hrnet_step(4, prec, frozen, inputs_grad, **kw)
    _assert_same(frozen, got, want)


def test_alphas_only_gradient_equals_the_full_backward():
    """Only d alphas asked for (frozen model, lrs without grad): the fusion levels' data gradients, no encoder."""
    want = _hrnet_step(3, "fp32", lambda k: False, True)
    m = _hrnet(3, "fp32")
    for p in m.parameters():
        p.requires_grad_(False)
    lrs, alphas, cot = _inputs(2, 5, 16, 3)
    alphas.requires_grad_(True)
    counts, _ = _launches(lambda: (m(lrs, alphas) * cot).sum().backward())
    assert torch.equal(alphas.grad, want[2])
    assert counts["conv_wgrad_f32"] == 0 and counts["stem_wgrad"] == 0 and counts["decoder_bwd_finish"] == 0
    assert counts["fuse_scatter"] > 0 and counts.get("prof:stem_dgrad_route", 0) == 0


# ----------------------------------------------------------------------------- 2. the work is skipped
def _levels(V):
    n, T = V, 0
    while n // 2 > 0:
        n //= 2
        T += 1
    return T


def _counted_step(prec, frozen, scale=3, V=5):
    m = _hrnet(scale, prec)
    for k, p in m.named_parameters():
        p.requires_grad_(not frozen(k))
    lrs, alphas, cot = _inputs(2, V, 16, scale)
    loss = (m(lrs, alphas) * cot).sum()
    counts, _ = _launches(loss.backward)
    return counts


@pytest.mark.parametrize("prec", PRECS)
def test_decoder_only_step_launches_no_encoder_or_fusion_work(prec):
    c = _counted_step(prec, PATTERNS["encoder+fuse"])
    assert c["decoder_bwd"] >= 1 and c["decoder_bwd_finish"] == 1
    for k in ("conv_wgrad_f32", "stem_wgrad", "prelu_bwd", "bias_finish", "slope_finish", "conv_dgrad", "fuse_scatter"):
        assert c[k] == 0, (k, c)
    prof = [k for k, v in c.items() if k.startswith("prof:") and v]
    assert not [k for k in prof if k.startswith(("prof:conv", "prof:stem", "prof:alpha"))], prof


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_frozen_encoder_step_stops_at_the_first_fusion_level(prec):
    T = _levels(5)
    full = _counted_step(prec, lambda k: False)
    c = _counted_step(prec, PATTERNS["encoder"])
    # every level but the first walks its three data gradients; the first stops after convB's (nothing reads its input gradient)
    assert c["conv_dgrad"] == 3 * (T - 1) + 2 and c["fuse_scatter"] == T - 1
    assert full["conv_dgrad"] == 3 * T + 1 + 2 * weights.HRNET_CONFIG["encoder"]["num_layers"]
    assert c["stem_wgrad"] == 0 and full["stem_wgrad"] == 1
    wg = "conv_wgrad_f32" if prec == "fp32" else "prof:conv_wgrad_bf16"
    nl = weights.HRNET_CONFIG["encoder"]["num_layers"]
    per_level = 4 + 4 + 2                                     # one launch per 64 x 64 chunk pair: 128 -> 128 twice, 128 -> 64
    assert c[wg] == T * per_level and full[wg] == T * per_level + 2 * nl + 1


@pytest.mark.parametrize("prec", PRECS)
def test_all_trainable_launches_what_the_parent_entry_points_launch(prec):
    """The module's all-trainable backward, the parent's op (hrn_hrnet_backward_s) and hrnet_backward_sel with every parameter
    requested launch the same kernels, as many times, and give the same gradients."""
    from hrnet_hip import binding
    ops = torch.ops.hrnet_hip
    dt = {"fp32": binding.F32, "bf16": binding.BF16, "bf16x3": binding.BF16X3}[prec]
    m = _hrnet(3, prec)
    lrs, alphas, cot = _inputs(2, 5, 16, 3)
    loss = (m(lrs, alphas) * cot).sum()
    module_counts, _ = _launches(loss.backward)
    params = [p.detach() for p in m.parameters()]
    pk = m._packed_for(dt)
    sr, tws = ops.hrnet_forward_train(pk, lrs, alphas, params, 2, True, dt, 3)
    old_counts, old = _launches(lambda: ops.hrnet_backward(pk, params, lrs, alphas, cot, tws, 2, True, dt, 3))
    sel_counts, sel = _launches(lambda: ops.hrnet_backward_sel(pk, params, lrs, alphas, cot, tws, 2, True, dt, 3, [True] * len(params),
                                                               False, False))
    assert module_counts == old_counts == sel_counts
    assert old_counts["conv_dgrad"] > 0 and old_counts["fuse_scatter"] > 0
    for a, b, p in zip(old, sel[0], m.parameters()):
        assert torch.equal(a, b) and torch.equal(a, p.grad)


def test_hrnet_backward_sel_opcheck():
    from hrnet_hip import binding
    ops = torch.ops.hrnet_hip
    m = _hrnet(2, "bf16")
    params = [p.detach() for p in m.parameters()]
    lrs, alphas, _ = _inputs(2, 3, 8, 2)
    pk = m._packed_for(binding.BF16)
    sr, tws = ops.hrnet_forward_train(pk, lrs, alphas, params, 2, True, binding.BF16, 2)
    need = [k.startswith("decode.") for k, _ in m.named_parameters()]
    d = torch.rand_like(sr)
    for args in ((need, False, True), ([False] * len(params), True, False)):
        torch.library.opcheck(ops.hrnet_backward_sel.default, (pk, params, lrs, alphas, d, tws, 2, True, binding.BF16, 2) + args,
                              test_utils=("test_schema", "test_faketensor"))
    grads, d_lrs, d_alphas = ops.hrnet_backward_sel(pk, params, lrs, alphas, d, tws, 2, True, binding.BF16, 2, need, False, True)
    assert [g.numel() > 0 for g in grads] == need and d_lrs.numel() == 0 and tuple(d_alphas.shape) == (2, 3)


# ----------------------------------------------------------------------------- ShiftNet
def _shiftnet(prec):
    from DeepNetworks.ShiftNet import ShiftNet
    m = ShiftNet()
    m.load_state_dict(weights.to_torch_state(weights.shiftnet_state(4321)))
    if prec is not None:
        m.train_precision = prec
    return m.cuda().train()


def _register_batch(shiftnet, lrs, reference, pairs):            # train.py:26-44, keeping each pair's gradient
    out = []
    for i in range(lrs.size(1)):
        x = torch.cat([reference, lrs[:, i:i + 1]], 1)
        x.retain_grad()
        pairs.append(x)
        out.append(shiftnet(x))
    return torch.stack(out, 1)


def _train_step(hprec, sprec, shiftnet_frozen):
    """The training step of tools/train_step_bench.py (train.py:164-190) at a small shape -> (HRNet .grad, ShiftNet .grad, d pairs)."""
    fusion, regis = _hrnet(3, hprec), _shiftnet(sprec)
    for p in regis.parameters():
        p.requires_grad_(not shiftnet_frozen)
    B, V, S = 2, 4, 48
    lrs, alphas, _ = _inputs(B, V, S, 3, seed=11)
    rng = np.random.Generator(np.random.PCG64(12))
    hrs = torch.from_numpy(rng.random((B, 3 * S, 3 * S), dtype=np.float32) * 0.25).cuda()
    maps = torch.ones((B, 3 * S, 3 * S), device="cuda")
    maps[:, :3] = 0
    off = (3 * S - 128) // 2
    torch.manual_seed(5)                                      # the dropout masks
    srs = fusion(lrs, alphas)
    pairs = []
    shifts = _register_batch(regis, srs[:, :, off:off + 128, off:off + 128], hrs[:, off:off + 128, off:off + 128].reshape(-1, 1, 128, 128),
                             pairs)
    shifted = regis.transform(shifts.view(-1, 2), srs.view(-1, 1, 3 * S, 3 * S)).view(-1, 1, 3 * S, 3 * S)[:, 0]   # apply_shifts
    nclear = torch.sum(maps, dim=(1, 2))
    bright = torch.sum(maps * (hrs - shifted), dim=(1, 2)).clone().detach() / nclear
    loss = torch.mean(10 * torch.log10(torch.sum(maps * (shifted + bright.view(-1, 1, 1) - hrs) ** 2, dim=(1, 2)) / nclear))
    loss = loss + 1e-6 * torch.mean(shifts) ** 2
    counts, _ = _launches(loss.backward)
    return ({k: p.grad for k, p in fusion.named_parameters()}, {k: p.grad for k, p in regis.named_parameters()}, [x.grad for x in pairs],
            counts)


@pytest.mark.parametrize("hprec,sprec", [("fp32", None), ("bf16", "bf16")])
def test_frozen_shiftnet_train_step(hprec, sprec):
    hf, sf, pf, cf = _train_step(hprec, sprec, False)
    hz, sz, pz, cz = _train_step(hprec, sprec, True)
    for k in hf:
        assert torch.equal(hf[k], hz[k]), k
    assert all(g is None for g in sz.values()) and all(g is not None for g in sf.values())
    for a, b in zip(pf, pz):
        assert torch.equal(a, b)
    n = 1                                                     # register_batch over srs: one ShiftNet call per step
    assert cf["fc1_bwd_w"] == n and cz["fc1_bwd_w"] == 0
    assert cf["fc1_bwd_x"] == cz["fc1_bwd_x"] == n and cf["sn_bn_bwd"] == cz["sn_bn_bwd"] == 8 * n
    assert cf["stem_wgrad"] == 1 + n and cz["stem_wgrad"] == 1          # HRNet's stem + ShiftNet's first layer per call
    if sprec is None:
        # fp32 conv weight gradients: HRNet's are the same in both steps, ShiftNet's seven 3x3 layers go
        assert cf["conv_wgrad_f32"] - cz["conv_wgrad_f32"] == n * (1 + 1 + 1 + 2 + 4 + 4 + 4)


def test_partly_frozen_shiftnet_stops_at_the_deepest_trainable_layer():
    """fc1 / fc2 and layers 1-5 frozen, d x not wanted: the walk stops at layer 6; gradients equal the full backward's."""
    from hrnet_hip import binding
    x = torch.rand(3, 2, 128, 128, device="cuda")

    def run(frozen):
        m = _shiftnet(None)
        for k, p in m.named_parameters():
            p.requires_grad_(not frozen(k))
        torch.manual_seed(7)
        theta = m(x)
        counts, _ = _launches(lambda: (theta * torch.tensor([1.0, -2.0], device="cuda")).sum().backward())
        return {k: p.grad for k, p in m.named_parameters()}, counts

    def frozen(k):
        return not k.startswith(("layer6.", "layer7.", "layer8."))

    want, cfull = run(lambda k: False)
    got, c = run(frozen)
    for k in want:
        assert (got[k] is None) if frozen(k) else torch.equal(got[k], want[k]), k
    assert c["sn_bn_bwd"] == 3 and c["fc1_bwd_w"] == 0 and c["fc1_bwd_x"] == 1 and c["stem_wgrad"] == 0
    assert cfull["sn_bn_bwd"] == 8 and cfull["fc1_bwd_w"] == 1
    assert binding.SHIFTNET_PARAM_NAMES == [k for k, _ in _shiftnet(None).named_parameters()]


def test_shiftnet_backward_sel_opcheck():
    from hrnet_hip import binding
    ops = torch.ops.hrnet_hip
    sn = _shiftnet(None)
    named = sn._named()
    sp = [named[k] for k in binding.SHIFTNET_PARAM_NAMES]
    sb = [named[k] for k in binding.SHIFTNET_BUFFER_NAMES]
    pairs = torch.rand(2, 2, 128, 128, device="cuda")
    mask = (torch.rand(2, 32768, device="cuda") >= 0.5).to(torch.uint8)
    theta, stws, _ = ops.shiftnet_forward_train(sn.packed_parameters(), pairs, sp, sb, 0.1, mask)
    need = [k.startswith("layer8.") or k == "fc2.weight" for k in binding.SHIFTNET_PARAM_NAMES]
    det = [p.detach() for p in sp]
    torch.library.opcheck(ops.shiftnet_backward_sel.default, (det, pairs, mask, torch.rand_like(theta), stws, True, 0, need),
                          test_utils=("test_schema", "test_faketensor"))
    grads, d_x = ops.shiftnet_backward_sel(det, pairs, mask, torch.rand_like(theta), stws, False, 0, need)
    assert [g.numel() > 0 for g in grads] == need and d_x.numel() == 0
