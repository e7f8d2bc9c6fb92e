"""The shift-searched loss restated in torch fp64, for the tests of hrnet_hip.losses.shift_loss: the search of
Evaluator.shift_cPSNR (src/Evaluator.py:52-73) over the brightness-corrected cMSE of get_loss (src/train.py:66-87).  Autograd gives the
gradient: the selected offset is picked on detached values, so the gradient flows through that offset alone.  No test logic here."""
import torch

# the tolerances of tests/test_gpu_shift_loss.py (derived in its docstring): relative on the reductions; of the max-norm per element of d_srs
TOL = 1e-5
GRAD_TOL = 1e-6


def frame_of_row_ranges(rows_of, ranges, H, reach):
    """For maps that are zero outside the row ranges [(y0, y1)] of an (H, W) frame: the small frame whose searched loss is the big frame's -
    each range with `reach` real neighbour rows on either side (cut at the frame's edges, where the crop's own limits are the same),
    stacked.  A clear pixel meets only rows within 2 border (and, for cSSIM, a window) of itself, so with reach >= that every term of
    every sum of the big frame is a term of the small one and the rest of both is masked.  rows_of(a, b) -> a tuple of (b - a, W)
    tensors (srs, hrs, maps).  -> (the stacked tensors, each (1, rows, W); the windows [(a, b)])"""
    windows = [(max(0, y0 - reach), min(H, y1 + reach)) for y0, y1 in sorted(ranges)]
    assert all(b0 <= a1 for (_, b0), (a1, _) in zip(windows, windows[1:])), "ranges closer than their reach"
    parts = [rows_of(a, b) for a, b in windows]
    return tuple(torch.cat([p[i] for p in parts])[None] for i in range(len(parts[0]))), windows


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
