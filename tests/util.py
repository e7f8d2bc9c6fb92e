"""Helpers shared by test modules: goldens and error measures, the models and fp64 oracles of the HRNet forward and training path, the
forward's parity bounds, and the stand-ins of the multi-process tests."""
import copy
import os
import socket
import types

import numpy as np
import torch
import torch.nn.functional as F

from hrnet_hip import augment
from oracle import hrnet_np as O
from oracle import torch_port, weights

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def rel_err(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def psnr_db(a, b):
    """10 log10(peak^2 / mse) with peak = max|b|: a scale-free agreement measure for the bf16 path."""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    mse = ((a - b) ** 2).mean()
    return float(10 * np.log10(max(np.abs(b).max(), 1e-30) ** 2 / max(mse, 1e-300)))


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


_models = {}


def hip_hrnet(precision="fp32", alpha_residual=True, seed=1234):
    from DeepNetworks.HRNet import HRNet
    key = (precision, alpha_residual, seed)
    if key not in _models:
        cfg = {k: dict(v) for k, v in weights.HRNET_CONFIG.items()}
        cfg["recursive"]["alpha_residual"] = alpha_residual
        m = HRNet(cfg)
        m.load_state_dict(weights.to_torch_state(weights.hrnet_state(seed)))
        m.precision = precision
        _models[key] = m.cuda().eval()
    return _models[key]


def hip_shiftnet(seed=4321):
    from DeepNetworks.ShiftNet import ShiftNet
    m = ShiftNet()
    m.load_state_dict(weights.to_torch_state(weights.shiftnet_state(seed)))
    return m.cuda().eval()


def nhwc_to_nchw(t, prec=None):
    """(..., H, W, C) storage tensor -> float32 numpy (..., C, H, W); bf16x3 stage tensors are (2, ...) planes: hi + lo."""
    if prec == "bf16x3":
        t = t[0].float() + t[1].float()
    nd = t.dim()
    perm = list(range(nd - 3)) + [nd - 1, nd - 3, nd - 2]
    return t.float().permute(*perm).contiguous().cpu().numpy()


# ----------------------------------------------------------------------------- HRNet at any scale: state, model, fp64 restatement
def _hrnet_forward_s(lrs, alphas, st, num_layers=2, alpha_residual=True, scale=3):
    """torch_port.hrnet_forward (HRNet.py:186-211) with ConvTranspose2d(64, 64, scale, stride=scale) in the decoder."""
    b, v, h, w = lrs.shape
    ref = torch.median(lrs[:, :9], 1, keepdim=True).values
    x = torch.stack([lrs, ref.expand(-1, v, -1, -1)], 2).reshape(b * v, 2, h, w)
    x = torch_port._prelu(F.conv2d(x, st["encode.init_layer.0.weight"], st["encode.init_layer.0.bias"], padding=1), st,
                          "encode.init_layer.1.weight")
    for i in range(num_layers):
        x = torch_port._res_block(x, st, f"encode.res_layers.{i}")
    x = F.conv2d(x, st["encode.final.0.weight"], st["encode.final.0.bias"], padding=1).reshape(b, v, 64, h, w)
    n = v
    while n // 2 > 0:
        parity, half = n % 2, n // 2
        alice = x[:, :half]
        bob = x[:, half:n - parity].flip(1)
        z = torch_port._res_block(torch.cat([alice, bob], 2).reshape(b * half, 128, h, w), st, "fuse.fuse.0")
        f = torch_port._prelu(F.conv2d(z, st["fuse.fuse.1.weight"], st["fuse.fuse.1.bias"], padding=1), st, "fuse.fuse.2.weight")
        f = f.reshape(b, half, 64, h, w)
        if alpha_residual:
            f = alice + alphas[:, half:n - parity].flip(1).reshape(b, half, 1, 1, 1) * f
        x, n = f, half
    return _decode_s(x.mean(1), st, scale)


def _decode_s(x, st, scale):
    x = torch_port._prelu(F.conv_transpose2d(x, st["decode.deconv.0.weight"], st["decode.deconv.0.bias"], stride=scale), st,
                          "decode.deconv.1.weight")
    y = F.conv2d(x, st["decode.final.weight"], st["decode.final.bias"])
    if torch_port.ABS_TERMS is not None and y.requires_grad:
        rec = torch_port.ABS_TERMS
        y.register_hook(lambda g: rec.__setitem__("decode.final.bias", rec.get("decode.final.bias", 0.0) + float(g.abs().sum())))
    return y


def _state(scale, seed=1234, slopes=None):
    """weights.hrnet_state with a seeded (64, 64, S, S) deconv weight of the same scale as the x3 one."""
    st = weights.to_torch_state(weights.hrnet_state(seed))
    if scale != 3:
        rng = np.random.Generator(np.random.PCG64(seed + 100 * scale))
        w3 = st["decode.deconv.0.weight"]
        w = rng.standard_normal((64, 64, scale, scale)) * float(w3.std())
        st["decode.deconv.0.weight"] = torch.from_numpy(w.astype(np.float32))
    st.update({k: torch.full_like(st[k], v) for k, v in (slopes or {}).items()})
    return st


def _model(scale, precision="fp32", alpha_residual=True, slopes=None, train=False):
    from DeepNetworks.HRNet import HRNet
    cfg = copy.deepcopy(weights.HRNET_CONFIG)
    cfg["decoder"]["deconv"]["kernel_size"] = cfg["decoder"]["deconv"]["stride"] = scale
    cfg["recursive"]["alpha_residual"] = alpha_residual
    m = HRNet(cfg)
    m.load_state_dict(_state(scale, slopes=slopes))
    m.precision = precision
    m = m.cuda()
    return m.train() if train else m.eval()


# ----------------------------------------------------------------------------- the training path's oracles
_SLOPE_KEYS = ["encode.init_layer.1.weight", "encode.res_layers.0.block.1.weight", "encode.res_layers.0.block.3.weight",
               "encode.res_layers.1.block.1.weight", "encode.res_layers.1.block.3.weight", "fuse.fuse.0.block.1.weight",
               "fuse.fuse.0.block.3.weight", "fuse.fuse.2.weight", "decode.deconv.1.weight"]


def _fresh_model(alpha_residual=True, seed=1234, slopes=None, precision="fp32"):
    from DeepNetworks.HRNet import HRNet
    cfg = {k: dict(v) for k, v in weights.HRNET_CONFIG.items()}
    cfg["recursive"]["alpha_residual"] = alpha_residual
    m = HRNet(cfg)
    st = weights.to_torch_state(weights.hrnet_state(seed))
    st.update({k: torch.full_like(st[k], v) for k, v in (slopes or {}).items()})
    m.load_state_dict(st)
    m.precision = precision
    return m.cuda().train()


def _oracle_grads(lrs, alphas, cot, alpha_residual, seed=1234, slopes=None):
    st = weights.to_torch_state(weights.hrnet_state(seed))
    st.update({k: torch.full_like(st[k], v) for k, v in (slopes or {}).items()})
    st = {k: v.double().requires_grad_(True) for k, v in st.items()}
    abs_terms = {}
    torch_port.ABS_TERMS = abs_terms             # sum |terms| of every single-slope / final-bias gradient (oracle/torch_port.py)
    try:
        with torch.enable_grad():
            sr = torch_port.hrnet_forward.__wrapped__(torch.from_numpy(lrs).double(), torch.from_numpy(alphas).double(), st,
                                                      num_layers=weights.HRNET_CONFIG["encoder"]["num_layers"], alpha_residual=alpha_residual)
            (sr * torch.from_numpy(cot).double()).sum().backward()
    finally:
        torch_port.ABS_TERMS = None
    # parameters the graph never touched (the fusion block when V == 1) have no gradient in torch: zero here
    grads = {k: (v.grad.numpy() if v.grad is not None else np.zeros(tuple(v.shape))) for k, v in st.items()}
    grads["__abs_terms__"] = abs_terms
    return sr.detach().numpy(), grads


NONPOS = {"encode.init_layer.1.weight": -0.2, "encode.res_layers.0.block.1.weight": 0.0, "encode.res_layers.0.block.3.weight": -0.05,
          "encode.res_layers.1.block.3.weight": -0.3, "fuse.fuse.0.block.1.weight": -0.1, "fuse.fuse.0.block.3.weight": 0.0,
          "fuse.fuse.2.weight": -0.25, "decode.deconv.1.weight": -0.1}


def _register_batch(shiftNet, lrs, reference):                 # train.py:26-44, restated
    thetas = [shiftNet(torch.cat([reference, lrs[:, i:i + 1]], 1)) for i in range(lrs.size(1))]
    return torch.stack(thetas, 1)


def _get_loss_cpsnr(srs, hrs, hr_maps):                        # train.py:66-87, metric='cPSNR'
    nclear = torch.sum(hr_maps, dim=(1, 2))
    bright = torch.sum(hr_maps * (hrs - srs), dim=(1, 2)).clone().detach() / nclear
    loss = torch.sum(hr_maps * (srs + bright.view(-1, 1, 1) - hrs) ** 2, dim=(1, 2)) / nclear
    return -10 * torch.log10(loss)


_real_median = torch.median


def _forward(x, a, st, alpha_residual, scale):
    return _hrnet_forward_s(x, a, st, num_layers=weights.HRNET_CONFIG["encoder"]["num_layers"], alpha_residual=alpha_residual, scale=scale)


def _oracle(lrs, alphas, cot, alpha_residual, slopes=None, scale=3, split=False):
    """-> (d lrs, d alphas or None, R or None).  split: the median's values as a leaf of their own, so d lrs is c0 and R comes apart."""
    st = {k: v.double() for k, v in _state(scale, slopes=slopes).items()}
    x = torch.from_numpy(lrs).double().requires_grad_(True)
    a = torch.from_numpy(alphas).double().requires_grad_(True)
    leaves = []

    def median(t, dim, keepdim=False):
        r = _real_median(t.detach(), dim, keepdim=keepdim)
        leaf = r.values.clone().requires_grad_(True)
        leaves.append(leaf)
        return types.SimpleNamespace(values=leaf, indices=r.indices)

    try:
        if split:
            torch.median = median
        with torch.enable_grad():
            (_forward(x, a, st, alpha_residual, scale) * torch.from_numpy(cot).double()).sum().backward()
    finally:
        torch.median = _real_median
    return x.grad.numpy(), (None if a.grad is None else a.grad.numpy()), (leaves[0].grad.numpy()[:, 0] if split else None)


def _tie_invariant_err(got, want, lrs):
    """max-norm relative error of d lrs with the tied views of each pixel (several of the first min(V, 9) equal to the median) compared
    by their sum, every other element directly."""
    n = min(lrs.shape[1], 9)
    med = _real_median(torch.from_numpy(lrs[:, :n]), 1).values.numpy()
    tied = lrs[:, :n] == med[:, None]
    multi = np.broadcast_to(tied.sum(1)[:, None] > 1, tied.shape)
    direct = np.concatenate([~multi, np.ones((lrs.shape[0], lrs.shape[1] - n) + lrs.shape[2:], bool)], 1)
    e = np.abs(got - want)[direct].max(initial=0.0)
    e_sum = np.abs(np.where(tied, got[:, :n], 0).sum(1) - np.where(tied, want[:, :n], 0).sum(1)).max()
    return float(max(e, e_sum) / max(np.abs(want).max(), 1e-30))


# ----------------------------------------------------------------------------- the forward's parity bounds (tests/test_gpu_parity.py)
FP32_CONTRACT, FP32_GUARD = 1e-3, 2e-5
BF16_REL, BF16_PSNR = 2.5e-2, 45.0
X3_REL = 1e-4          # bf16x3 (split-bf16, three MFMAs per product): inside the 1e-3 contract by 10x; measured worst ~2e-5


def _check(prec, got, want):
    if prec == "fp32":
        e = rel_err(got, want)
        assert e <= FP32_CONTRACT and e <= FP32_GUARD, e
    elif prec == "bf16x3":
        e = rel_err(got, want)
        if os.environ.get("HRN_TEST_RECORD"):
            with open(os.environ["HRN_TEST_RECORD"], "a") as f:
                f.write(f"bf16x3 {e:.4e}\n")
        assert e <= FP32_CONTRACT and e <= X3_REL, e
    else:
        if os.environ.get("HRN_TEST_RECORD"):      # measured margins of the bf16 bounds: one line per check
            with open(os.environ["HRN_TEST_RECORD"], "a") as f:
                f.write(f"{rel_err(got, want):.4e} {psnr_db(got, want):.2f}\n")
        assert rel_err(got, want) <= BF16_REL and psnr_db(got, want) >= BF16_PSNR, (rel_err(got, want), psnr_db(got, want))


# ----------------------------------------------------------------------------- multi-process tests and their CPU stand-ins
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


class Toy(torch.nn.Module):
    """Bicubic x3 of the first view; its "ensemble" is the rule of augment.py around its own forward."""

    def forward(self, lrs, alphas):
        return torch.nn.functional.interpolate(lrs[:, :1], scale_factor=3, mode="bicubic", align_corners=False)

    def forward_ensemble(self, lrs, alphas, mode="dihedral", members_per_pass=None):
        codes = augment.ensemble_codes(mode)
        self.seen = (mode, members_per_pass)
        y = torch.stack([self.forward(m, alphas) for m in augment.expand(lrs, codes)])
        return augment.mean_inverse(y, codes)


def _score(srs, hrs, maps):
    return torch.tensor([O.shift_cpsnr(np.clip(s.numpy(), 0, 1), h.numpy(), m.numpy()) for s, h, m in zip(srs, hrs, maps)])


def _sets(n, with_names=True, batch=1):
    g = torch.Generator().manual_seed(3)
    sets = []
    for i in range(n):
        b = batch + (i % 2 if batch > 1 else 0)
        item = (torch.rand(b, 3, 16, 16, generator=g), torch.ones(b, 3), torch.rand(b, 48, 48, generator=g),
                (torch.rand(b, 48, 48, generator=g) > 0.1).float())
        sets.append(item + ([f"imgset{i:04d}_{j}" for j in range(b)],) if with_names else item)
    return sets


def _esa_table(sets):
    rng = np.random.Generator(np.random.PCG64(9))
    return {n: float(40 + 10 * rng.random()) for s in sets for n in s[4]}
