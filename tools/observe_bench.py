#!/usr/bin/env python3
"""Time the observation model: hrn_consistency_residual / _finish and hrn_observe_adjoint.

In ONE process, after a warm-up, at (B, V, H, W) = (32, 32, 128, 128) and at one (1, 32, 2048, 1536) scene, both x3, masks 30 % hidden,
shifts within 1.5 px, brightness on.  With lr = B V H W and sr = S^2 B H W elements of four bytes:

    residual       hrn_consistency_residual + hrn_consistency_finish:  4 (sr + 3 lr)   x read once, views and masks read, the residual written
    adjoint        hrn_observe_adjoint, out = coef G:                  4 (2 lr + sr)   residual and masks read, d_x written
    loss_fwd_bwd   the two above, as consistency_loss + backward:      their sum
    iteration      residual + finish + adjoint in place:               4 (sr + 3 lr) + 4 (2 lr + 2 sr)   x read and written by the adjoint too
    ten            ten iterations (binding.back_project)
    torch_*        the same definition composed in torch on the device: the windows of every view gathered from the padded frame, ONE
                   grouped strided conv2d with the (S + 5)^2 kernels of all views, the masked sums; the backward (and with it the
                   adjoint and an iteration) is autograd through it

Every time is a pair of device events around `reps` calls enqueued back to back on one stream; the calls walk over enough input sets to
exceed the 256 MB last-level cache, so the bytes come from HBM.  A round is `reps` calls of each; the figure is the median over the
rounds, with min and max as the run-to-run spread.  The byte floors are the algorithmic bytes at the 6.3 TB/s a streaming kernel reaches
on an MI355X.  Before anything is timed the kernels' results are compared with the composition's.  There is no pass / fail threshold on
time.

usage: python tools/observe_bench.py [--rounds R] [--reps N]
"""
import _common
import torch
import torch.nn.functional as F

from _common import HBM_ACHIEVABLE, LLC_BYTES
from hrnet_hip import binding

PARSER = _common.parser(__doc__, rounds=7, reps=10)
CASES = [(32, 32, 128, 128, 3), (1, 32, 2048, 1536, 3)]          # (B, V, H, W, scale)


def floor_us(B, V, H, W, scale, what):
    """the byte floor in microseconds (the formulas of the module's text)"""
    lr, sr = B * V * H * W, B * H * W * scale * scale
    residual, adjoint = sr + 3 * lr, 2 * lr + sr
    n = {"residual": residual, "adjoint": adjoint, "loss_fwd_bwd": residual + adjoint, "iteration": residual + adjoint + sr,
         "ten": 10 * (residual + adjoint + sr)}[what]
    return 4.0 * n / HBM_ACHIEVABLE * 1e6


def weights(shift, S):
    """shift (...,) f32 -> (n (...,) long, w (..., S + 5) f32, reach (...,) bool): the library's weight vector (include/hrnet_hip.h)"""
    c = (-float(S) * shift.double()).float()
    reach = c.abs() < 256.0
    c = c.clamp(-256.0, 256.0)
    n = torch.floor(c)
    f = c.double() - n.double()
    x = torch.arange(-2, 4, dtype=torch.float64, device=shift.device) - f[..., None]
    t = torch.sinc(x) * torch.sinc(x / 3.0)
    t = torch.where(x.abs() >= 3.0, torch.zeros_like(t), t)
    t = t / t.sum(-1, keepdim=True)
    w = torch.zeros(shift.shape + (S + 5,), dtype=torch.float64, device=shift.device)
    for k in range(S):
        w[..., k:k + 6] += t
    return n.long(), (w / S).float(), reach


def torch_observe(x, shifts, S):
    """x (B,SH,SW), shifts (B,V,2) -> (views (B,V,H,W), valid bool): hrn_observe's definition composed in torch, in x's dtype"""
    B, SH, SW = x.shape
    V, H, W = shifts.shape[1], SH // S, SW // S
    finite = torch.isfinite(shifts).all(-1)
    sh = torch.where(finite[..., None], shifts, torch.zeros_like(shifts))
    (ny, wy, ry), (nx, wx, rx) = weights(sh[..., 0], S), weights(sh[..., 1], S)
    P = int(max(ny.abs().max(), nx.abs().max())) + 3
    xp = F.pad(x, (P, P, P, P))
    rows = (P + ny - 2)[..., None] + torch.arange(S * H + 5, device=x.device)                   # (B,V,SH+5)
    cols = (P + nx - 2)[..., None] + torch.arange(S * W + 5, device=x.device)
    b = torch.arange(B, device=x.device)[:, None, None, None]
    crops = xp[b, rows[..., :, None], cols[..., None, :]]                                        # (B,V,SH+5,SW+5)
    kern = (wy.to(x.dtype)[..., :, None] * wx.to(x.dtype)[..., None, :]).reshape(B * V, 1, S + 5, S + 5)
    views = F.conv2d(crops.reshape(1, B * V, S * H + 5, S * W + 5), kern, stride=S, groups=B * V).reshape(B, V, H, W)
    iy, ix = torch.arange(H, device=x.device), torch.arange(W, device=x.device)
    vy = (S * iy + ny[..., None] - 2 >= 0) & (S * iy + ny[..., None] + S + 2 <= S * H - 1)
    vx = (S * ix + nx[..., None] - 2 >= 0) & (S * ix + nx[..., None] + S + 2 <= S * W - 1)
    valid = vy[..., :, None] & vx[..., None, :] & (finite & ry & rx)[..., None, None]
    return torch.where(valid, views, torch.zeros_like(views)), valid


def torch_consistency_loss(x, lrs, masks, shifts, S, brightness=True, return_residual=False):
    """-> L (B,) [, r (B,V,H,W)]: the consistency loss composed in torch (alphas None)"""
    views, valid = torch_observe(x, shifts, S)
    cm = valid if masks is None else valid & (masks != 0)
    e = torch.where(cm, views - lrs.to(x.dtype), torch.zeros_like(views))
    n = cm.sum((2, 3)).to(x.dtype)
    safe = n.clamp_min(1)
    beta = -e.sum((2, 3)) / safe if brightness else torch.zeros_like(n)
    r = torch.where(cm, e + beta[..., None, None], torch.zeros_like(e))
    tot = n.sum(1)
    L = (r * r).sum((1, 2, 3)) / tot.clamp_min(1)
    return (L, r) if return_residual else L


def _times(call, nsets, rounds, reps):
    for i in range(max(nsets, 2)):
        call(i)
    torch.cuda.synchronize()
    out = []
    for r in range(rounds):
        k = [r * reps]

        def one():
            call(k[0])
            k[0] += 1
        out.append(_common.timed_us(one, reps))
    return out


def bench_case(B, V, H, W, S, rounds, reps):
    dev = torch.device("cuda:0")
    lr, sr = B * V * H * W, B * H * W * S * S
    per_set = 4 * (3 * lr + 2 * sr)
    nsets = min(16, max(2, -(-2 * LLC_BYTES // per_set)))
    gen = torch.Generator(device=dev).manual_seed(S)
    xs = [torch.rand((B, S * H, S * W), device=dev, generator=gen) for _ in range(nsets)]
    lrs = [torch.rand((B, V, H, W), device=dev, generator=gen) for _ in range(nsets)]
    masks = [(torch.rand((B, V, H, W), device=dev, generator=gen) >= 0.3).float() for _ in range(nsets)]
    shifts = (torch.rand((B, V, 2), device=dev, generator=gen) * 3.0 - 1.5).contiguous()
    state = binding.ConsistencyState(B, V, H, W, dev)
    loss = torch.empty((B,), device=dev)
    gl = torch.ones((B,), device=dev)
    outs = [torch.empty((B, S * H, S * W), device=dev) for _ in range(2)]
    residual = lambda i: binding.consistency_residual(xs[i % nsets], lrs[i % nsets], masks[i % nsets], None, shifts, S, 1.0, True, state, loss)
    # the adjoint is timed on residual planes of its own (one per input set), so that it reads what it would read in a run
    residual(0)
    beta = state.beta.clone()
    planes = []
    for i in range(nsets):
        residual(i)
        planes.append(state.residual.clone())
    residual(0)
    adjoint = lambda i: binding.observe_adjoint(planes[i % nsets], masks[i % nsets], None, shifts, beta, state.coef_loss, gl, None, S, out=outs[i % 2])

    def fwd_bwd(i):
        residual(i)
        binding.observe_adjoint(state.residual, masks[i % nsets], None, shifts, state.beta, state.coef_loss, gl, None, S, out=outs[i % 2])

    def iteration(i):
        residual(i)
        binding.observe_adjoint(state.residual, masks[i % nsets], None, shifts, state.beta, state.coef_step, None, xs[i % nsets], S, out=outs[i % 2])

    ten = lambda i: binding.back_project(xs[i % nsets], lrs[i % nsets], masks[i % nsets], None, shifts, S, 10, 1.0, True)
    # what is timed computes what the composition computes: the composition in fp64, the bound 1e-5 of the sums of absolute terms (<= 2)
    xr = xs[0].double().requires_grad_(True)
    t_L, t_r = torch_consistency_loss(xr, lrs[0].double(), masks[0], shifts, S, return_residual=True)
    residual(0)
    k_r = state.residual + torch.where(t_r.detach() != 0, state.beta[..., None, None], torch.zeros_like(state.residual))    # r = e + beta where counted
    e_L, e_r = float((loss.double() - t_L.detach()).abs().max() / t_L.detach().abs().max()), float((k_r.double() - t_r.detach()).abs().max())
    (t_g,) = torch.autograd.grad(t_L.sum(), xr)
    k_g = binding.observe_adjoint(state.residual, masks[0], None, shifts, state.beta, state.coef_loss, gl, None, S)
    e_g = float((k_g.double() - t_g).abs().max() / t_g.abs().max())
    print(f"({B}, {V}, {H}, {W}) -> x{S}: against the fp64 composition: loss {e_L:.1e} relative, residual {e_r:.1e}, gradient {e_g:.1e} of its largest")
    assert e_L <= 1e-5 and e_r <= 2e-5 and e_g <= 1e-4, (e_L, e_r, e_g)
    del xr, t_L, t_r, t_g, k_r

    def t_fwd(i):
        with torch.no_grad():
            return torch_consistency_loss(xs[i % nsets], lrs[i % nsets], masks[i % nsets], shifts, S)

    def t_fwd_bwd(i):
        x = xs[i % nsets].detach().requires_grad_(True)
        torch_consistency_loss(x, lrs[i % nsets], masks[i % nsets], shifts, S).sum().backward()
        return x.grad

    def t_adjoint(i):                                                    # autograd's backward alone cannot be cut out: the whole pair
        return t_fwd_bwd(i)

    def t_iteration(i):
        x = xs[i % nsets].detach().requires_grad_(True)
        L, r = torch_consistency_loss(x, lrs[i % nsets], masks[i % nsets], shifts, S, return_residual=True)
        (g,) = torch.autograd.grad(0.5 * (r * r).sum(), x)
        return x.detach() - (S * S / V) * g

    res = {"B": B, "V": V, "H": H, "W": W, "scale": S, "input_sets": nsets, "rounds": rounds, "reps": reps}
    runs = {"residual": (residual, t_fwd), "adjoint": (adjoint, t_adjoint), "loss_fwd_bwd": (fwd_bwd, t_fwd_bwd),
            "iteration": (iteration, t_iteration), "ten": (ten, None)}
    print(f"({B}, {V}, {H}, {W}) -> x{S}: median of {rounds} rounds x {reps} calls over {nsets} input sets")
    for name, (call, tcall) in runs.items():
        med, lo, hi = _common.spread(_times(call, nsets, rounds, reps if name != "ten" else max(1, reps // 5)))
        floor = floor_us(B, V, H, W, S, name)
        res[name] = {"median_us": med, "min_us": lo, "max_us": hi, "floor_us": floor}
        line = f"    {name:13s} {med:9.1f} us   (min {lo:.1f}, max {hi:.1f})   byte floor {floor:.1f} us = {100 * floor / med:.0f} % of it"
        if tcall is not None:
            tmed, tlo, thi = _common.spread(_times(tcall, 2, max(3, rounds // 2), 1))
            res["torch_" + name] = {"median_us": tmed, "min_us": tlo, "max_us": thi}
            line += f";   torch {tmed:9.1f} us (min {tlo:.1f}, max {thi:.1f}) = {tmed / med:.1f} x"
        print(line)
    return res


def main():
    o = PARSER.parse_args()
    _common.require_gpu("observe_bench")
    _common.emit("observe_bench", [bench_case(B, V, H, W, S, o.rounds, o.reps) for B, V, H, W, S in CASES])


if __name__ == "__main__":
    main()
