"""The shift-searched, brightness-corrected L1 / Charbonnier loss restated in torch fp64 (the definition is in
include/hrnet_hip.h), for the tests of hrnet_hip.losses.cl1_loss.  With beta = border, s the centre crop of srs (clamped to [0, 1] when
clip), and for the offset k = u (2 beta + 1) + v: g = hrs[u:u+h, v:v+w], m = maps[u:u+h, v:v+w] (a weight),
    n_k = sum m,  b_k = sum m (g - s) / n_k,  e = s + b_k - g,  cL1_k = sum m rho(e) / n_k,  sigma_k = sum m rho'(e) / n_k,
rho(e) = |e| for eps == 0 and sqrt(e^2 + eps^2) otherwise.  Autograd gives the gradient: the selected offset is picked on detached
values and the bias stays attached, so the gradient is the derivative of the returned number through that offset alone.
`closed_form_grad` is the same gradient written out, independently of autograd.  No test logic here."""
import torch


def rho(e, eps):
    return e.abs() if eps == 0 else torch.sqrt(e * e + eps * eps)


def drho(e, eps):
    return torch.sign(e) if eps == 0 else e / torch.sqrt(e * e + eps * eps)


def _crop(srs, border, clip):
    H, W = srs.shape[-2:]
    h, w = H - 2 * border, W - 2 * border
    s = srs[:, border:border + h, border:border + w]
    return (torch.clamp(s, 0.0, 1.0) if clip else s), h, w


def all_cl1(srs, hrs, maps, border, clip=False, eps=0.0):
    """(B,H,W) x 3 -> (cL1, n, b, sigma), each (B, (2 border + 1)^2) float64, k = u (2 border + 1) + v; cL1 differentiable in srs."""
    srs, hrs, maps = srs.double(), hrs.double(), maps.double()
    s, h, w = _crop(srs, border, clip)
    cl, ns, bs, sg = [], [], [], []
    for u in range(2 * border + 1):
        for v in range(2 * border + 1):
            g, m = hrs[:, u:u + h, v:v + w], maps[:, u:u + h, v:v + w]
            n = m.sum((1, 2))
            bias = (m * (g - s)).sum((1, 2)) / n
            e = s + bias[:, None, None] - g
            cl.append((m * rho(e, eps)).sum((1, 2)) / n)
            ns.append(n)
            bs.append(bias.detach())
            sg.append((m * drho(e.detach(), eps)).sum((1, 2)) / n)
    return torch.stack(cl, 1), torch.stack(ns, 1), torch.stack(bs, 1), torch.stack(sg, 1)


def select(cl, ns):
    """The lowest k of minimal cL1 among n_k > 0 (-1 without any), per sample; a NaN is never selected over a number."""
    ok = ns > 0
    c = torch.where(ok & ~torch.isnan(cl.detach()), cl.detach(), torch.full_like(cl, float("inf")))
    hit = ok & (c == c.min(1, keepdim=True).values)
    k = torch.where(hit, torch.arange(c.shape[1])[None], c.shape[1]).min(1).values
    return torch.where(ok.any(1), k, torch.full_like(k, -1))


def cl1_loss(srs, hrs, maps, border=3, clip=False, eps=0.0):
    """-> (out (B,) float64 = cL1_k*, NaN without a clear pixel, differentiable in srs; k* (B,) int64; cL1 (B, K) detached;
    stats (B,5) = {n*, b*, cL1*, k*, sigma*}, {0, 0, NaN, -1, 0} without a clear pixel)."""
    cl, ns, bs, sg = all_cl1(srs, hrs, maps, border, clip, eps)
    k = select(cl, ns)
    at = lambda t: t.gather(1, k.clamp(min=0)[:, None])[:, 0]
    some = k >= 0
    nan, zero = torch.full_like(ns[:, 0], float("nan")), torch.zeros_like(ns[:, 0])
    best = torch.where(some, at(cl), nan)
    stats = torch.stack([torch.where(some, at(ns), zero), torch.where(some, at(bs), zero), best.detach(), k.double(),
                         torch.where(some, at(sg), zero)], 1)
    return best, k, cl.detach(), stats


def _at_selected(srs, hrs, maps, border, clip, k):
    """per sample b with k*[b] >= 0: (b, s, g, m) at the selected offset"""
    srs, hrs, maps = srs.double(), hrs.double(), maps.double()
    s, h, w = _crop(srs, border, clip)
    nb = 2 * border + 1
    for b in range(srs.shape[0]):
        if int(k[b]) >= 0:
            u, v = int(k[b]) // nb, int(k[b]) % nb
            yield b, s[b], hrs[b, u:u + h, v:v + w], maps[b, u:u + h, v:v + w]


def closed_form_grad(srs, hrs, maps, k, d_out, border=3, clip=False, eps=0.0):
    """d sum_b d_out[b] out[b] / d srs (B,H,W) float64 by the closed form: d_out m* / n* (rho'(e*) - sigma*) on the centre crop, 0 on the
    border frame, where clip clamped (0 <= srs <= 1 passes) and for a sample with k* = -1."""
    grad = torch.zeros(srs.shape, dtype=torch.float64)
    H, W = srs.shape[-2:]
    for b, s, g, m in _at_selected(srs.detach(), hrs, maps, border, clip, k):
        n = m.sum()
        e = s + (m * (g - s)).sum() / n - g
        d = drho(e, eps)
        inner = float(d_out[b]) * m / n * (d - (m * d).sum() / n)
        if clip:
            raw = srs.detach().double()[b, border:H - border, border:W - border]
            inner = inner * ((raw >= 0) & (raw <= 1))
        grad[b, border:H - border, border:W - border] = inner
    return grad


def offsets(k, border):
    """k* -> (B,2) (u - border, v - border)."""
    nb = 2 * border + 1
    return torch.stack([torch.div(k, nb, rounding_mode="floor") - border, k % nb - border], 1)


def top_two_gap(cl):
    """Relative difference of the two lowest cL1 per sample: how far the selection is from a tie."""
    two = torch.sort(cl, 1).values[:, :2]
    return ((two[:, 1] - two[:, 0]) / two[:, 0]) if cl.shape[1] > 1 else torch.full((cl.shape[0],), float("inf"), dtype=cl.dtype)


def min_abs_e(srs, hrs, maps, k, border=3, clip=False):
    """The smallest |e| over the weighted (m != 0) pixels at k*, over the batch: how far every sign of the L1 gradient is from a flip."""
    least = float("inf")
    for b, s, g, m in _at_selected(srs, hrs, maps, border, clip, k):
        e = s + (m * (g - s)).sum() / m.sum() - g
        least = min(least, float(e[m != 0].abs().min()))
    return least
