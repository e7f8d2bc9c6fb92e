"""The shift-searched loss restated in torch fp64, for the tests of hrnet_hip.losses.shift_loss: the search of
Evaluator.shift_cPSNR (src/Evaluator.py:52-73) over the brightness-corrected cMSE of get_loss (src/train.py:66-87).  Autograd gives the
gradient: the selected offset is picked on detached values, so the gradient flows through that offset alone.  No test logic here."""
import torch


def all_cmse(srs, hrs, maps, border, clip=False):
    """(B,H,W) x 3 -> (cMSE (B, (2 border + 1)^2) float64, differentiable in srs; n (B, K) clear pixels), k = u (2 border + 1) + v."""
    srs, hrs, maps = srs.double(), hrs.double(), maps.double()
    H, W = srs.shape[-2:]
    h, w = H - 2 * border, W - 2 * border
    s = srs[:, border:border + h, border:border + w]
    if clip:
        s = torch.clamp(s, 0.0, 1.0)
    cm, ns = [], []
    for u in range(2 * border + 1):
        for v in range(2 * border + 1):          # row-major, the order of itertools.product in Evaluator.py:66
            g, m = hrs[:, u:u + h, v:v + w], maps[:, u:u + h, v:v + w]
            n = m.sum((1, 2))
            bias = (m * (g - s)).sum((1, 2)) / n
            cm.append((m * (s + bias[:, None, None] - g) ** 2).sum((1, 2)) / n)
            ns.append(n)
    return torch.stack(cm, 1), torch.stack(ns, 1)


def select(cm, ns):
    """The lowest k of minimal cMSE among n_k > 0 (-1 without any), per sample."""
    c = torch.where(ns > 0, cm.detach(), torch.full_like(cm, float("inf")))
    k = torch.where((c == c.min(1, keepdim=True).values), torch.arange(c.shape[1])[None], c.shape[1]).min(1).values
    return torch.where((ns > 0).any(1), k, torch.full_like(k, -1))


def shift_loss(srs, hrs, maps, metric="cPSNR", border=3, clip=False):
    """-> (out (B,) float64 = cMSE_k* or -10 log10(cMSE_k*), NaN without a clear pixel; k* (B,) int64; cMSE (B, K))."""
    cm, ns = all_cmse(srs, hrs, maps, border, clip)
    k = select(cm, ns)
    best = cm.gather(1, k.clamp(min=0)[:, None])[:, 0]
    best = torch.where(k >= 0, best, torch.full_like(best, float("nan")))
    return (best if metric == "cMSE" else -10.0 * torch.log10(best)), k, cm.detach()


def offsets(k, border):
    """k* -> (B,2) (u - border, v - border)."""
    nb = 2 * border + 1
    return torch.stack([torch.div(k, nb, rounding_mode="floor") - border, k % nb - border], 1)


def top_two_gap(cm):
    """Relative difference of the two lowest cMSE per sample: how far the selection is from a tie."""
    two = torch.sort(cm, 1).values[:, :2]
    return ((two[:, 1] - two[:, 0]) / two[:, 0]) if cm.shape[1] > 1 else torch.full((cm.shape[0],), float("inf"), dtype=cm.dtype)
