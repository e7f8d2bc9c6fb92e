"""The definition of hrn_masked_composite (include/hrnet_hip.h) restated in numpy, one pixel at a time with np.sort, and the sorting
networks of csrc/composite.hip restated as comparator lists.  Not a test module."""
import numpy as np


def masked_composite(views, masks=None, alphas=None, n_ref=9):
    """views (B,V,H,W) f32, masks (B,V,H,W) or None, alphas (B,V) or None -> (ref (B,H,W), count (B,H,W), filled (B,V,H,W)), f32."""
    views = np.asarray(views, np.float32)
    B, V, H, W = views.shape
    n = min(V, n_ref)
    real_all = np.ones((B, V), bool) if alphas is None else np.asarray(alphas) != 0
    clear_all = np.ones(views.shape, bool) if masks is None else np.asarray(masks) != 0
    ref = np.empty((B, H, W), np.float32)
    count = np.empty((B, H, W), np.float32)
    for b in range(B):
        real = real_all[b, :n]
        for y in range(H):
            for x in range(W):
                v = views[b, :n, y, x]
                cand = real & clear_all[b, :n, y, x]
                c = int(cand.sum())
                vote = cand if c else (real if real.any() else np.ones(n, bool))
                keys = np.sort(v[vote])
                ref[b, y, x] = keys[(len(keys) - 1) // 2]
                count[b, y, x] = c
    hole = real_all[:, :, None, None] & ~clear_all
    filled = np.where(hole, ref[:, None], views).astype(np.float32)
    return ref, count, filled


# the 25-exchange network for 9 keys (median_kernel of csrc/stem.hip, reused by csrc/composite.hip)
NET9 = [(0, 3), (1, 7), (2, 5), (4, 8), (0, 7), (2, 4), (3, 8), (5, 6), (0, 2), (1, 3), (4, 5), (7, 8), (1, 4), (3, 6), (5, 7),
        (0, 1), (2, 4), (3, 5), (6, 8), (2, 3), (4, 5), (6, 7), (1, 2), (3, 4), (5, 6)]


def batcher(n, p_from=1):
    """Batcher's odd-even merge sort for n = 2^k keys as a comparator list, the loops of csrc/composite.hip; p_from = n / 2: only its
    last stage, the merge of two sorted halves."""
    out = []
    p = 1
    while p < n:
        k = p
        while k >= 1:
            for j in range(k % p, n - k, 2 * k):
                for i in range(k):
                    if i + j + k < n and (i + j) // (2 * p) == (i + j + k) // (2 * p) and p >= p_from:
                        out.append((i + j, i + j + k))
            k //= 2
        p *= 2
    return out


def apply_network(net, keys):
    """keys (..., n): every comparator (i, j), i < j, puts the smaller at i - vectorised over the leading axes"""
    keys = np.array(keys, copy=True)
    for i, j in net:
        lo, hi = np.minimum(keys[..., i], keys[..., j]), np.maximum(keys[..., i], keys[..., j])
        keys[..., i], keys[..., j] = lo, hi
    return keys
