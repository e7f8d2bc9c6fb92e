"""CPU: the definition of the masked composite (tests/composite_ref.py, the numpy restatement the GPU tests compare the kernel with) on
hand-written cases, against the oracle's reference frame, and the kernel's sorting networks by the 0-1 principle."""
import numpy as np
import pytest

import composite_ref as R
from oracle import hrnet_np as O


def _px(values, masks=None, alphas=None, n_ref=9):
    """one sample, one pixel: lists over the views -> (ref, count, filled list)"""
    v = np.asarray(values, np.float32).reshape(1, -1, 1, 1)
    m = None if masks is None else np.asarray(masks, np.float32).reshape(1, -1, 1, 1)
    a = None if alphas is None else np.asarray(alphas, np.float32).reshape(1, -1)
    ref, count, filled = R.masked_composite(v, m, a, n_ref)
    return float(ref[0, 0, 0]), float(count[0, 0, 0]), filled[0, :, 0, 0].tolist()


@pytest.mark.parametrize("V", [1, 2, 5, 9, 12])
def test_unmasked_n9_is_the_oracles_reference_frame(V):
    rng = np.random.Generator(np.random.PCG64(V))
    lrs = np.floor(rng.random((2, V, 6, 7)) * 8).astype(np.float32) / 8          # ties
    ref, count, filled = R.masked_composite(lrs)
    assert np.array_equal(ref, O.reference_frame(lrs))
    assert np.array_equal(count, np.full_like(ref, min(V, 9))) and np.array_equal(filled, lrs)


def test_one_candidate():
    assert _px([5, 1, 9], [0, 0, 1]) == (9.0, 1.0, [9.0, 9.0, 9.0])


def test_even_count_takes_the_lower():
    assert _px([4, 2, 8, 6], [1, 1, 1, 1])[:2] == (4.0, 4.0)
    assert _px([4, 2, 8, 6], [1, 0, 1, 0]) == (4.0, 2.0, [4.0, 4.0, 8.0, 4.0])


def test_no_candidate_falls_back_to_the_real_views_with_count_zero():
    # masks ignored: lower median of {7, 3, 5} = 5; every real view is masked there, so every one is filled
    assert _px([7, 3, 5], [0, 0, 0]) == (5.0, 0.0, [5.0, 5.0, 5.0])
    # ... of the REAL views only: the padding view's 0 does not vote and stays as it is
    assert _px([7, 3, 0], [0, 0, 0], [1, 1, 0]) == (3.0, 0.0, [3.0, 3.0, 0.0])


def test_no_real_view_is_the_plain_median():
    assert _px([7, 3, 5], [1, 0, 1], [0, 0, 0]) == (5.0, 0.0, [7.0, 3.0, 5.0])


def test_padding_views_are_excluded_by_alphas():
    # the clear zeros of two padding views would drag the plain median to 0
    assert _px([6, 0, 0], None, [1, 0, 0]) == (6.0, 1.0, [6.0, 0.0, 0.0])
    assert _px([6, 8, 0, 0], [1, 1, 1, 1], [1, 1, 0, 0])[:2] == (6.0, 2.0)


def test_fewer_real_views_than_n_ref_and_views_beyond_it():
    # n_ref = 2: only the first two vote; the masked real view beyond them is filled, the clear one and the padding are not
    ref, count, filled = _px([2, 4, 100, 50, 0], [1, 1, 0, 1, 0], [1, 1, 1, 1, 0], n_ref=2)
    assert (ref, count, filled) == (2.0, 2.0, [2.0, 4.0, 2.0, 50.0, 0.0])
    # n_real = 1 < n_ref = 9
    assert _px([3, 0, 0], [1, 1, 1], [1, 0, 0], n_ref=9)[:2] == (3.0, 1.0)


def test_filled_leaves_padding_and_clear_pixels_untouched():
    ref, count, filled = _px([1, 2, 3, 0], [1, 0, 1, 0], [1, 1, 1, 0])
    assert (ref, count) == (1.0, 2.0) and filled == [1.0, 1.0, 3.0, 0.0]
    assert _px([1, 2, 3], None, [1, 1, 1])[2] == [1.0, 2.0, 3.0]


# ----------------------------------------------------------------------------- the sorting networks, by the 0-1 principle
def _all01(n):
    return ((np.arange(1 << n)[:, None] >> np.arange(n)) & 1).astype(np.int8)


def _sorted(keys):
    return bool((np.diff(keys.astype(np.int16), axis=-1) >= 0).all())


def test_net9_sorts_every_01_vector():
    assert len(R.NET9) == 25 and all(0 <= i < j < 9 for i, j in R.NET9)
    assert _sorted(R.apply_network(R.NET9, _all01(9)))


def test_net16_sorts_every_01_vector():
    net = R.batcher(16)
    assert len(net) == 63 and all(0 <= i < j < 16 for i, j in net)
    assert _sorted(R.apply_network(net, _all01(16)))


def test_net32_is_two_16_sorts_and_a_merge_of_sorted_halves():
    net, merge = R.batcher(32), R.batcher(32, p_from=16)
    assert len(net) == 191 and len(merge) == 65 and net[-65:] == merge and all(0 <= i < j < 32 for i, j in net)
    half = R.batcher(16)
    assert net[:-65] == [c for p in (1, 2, 4, 8) for c in sorted_stage(32, p)]
    # the stages before the merge never cross the halves, and restricted to one half they are the 16-key network, stage by stage
    lo = [c for c in net[:-65] if c[1] < 16]
    hi = [(i - 16, j - 16) for i, j in net[:-65] if i >= 16]
    assert len(lo) + len(hi) == 126 and lo == half and hi == half
    # the merge: all 17 x 17 pairs of sorted 0-1 halves
    pairs = np.array([[0] * (16 - a) + [1] * a + [0] * (16 - b) + [1] * b for a in range(17) for b in range(17)], np.int8)
    assert _sorted(R.apply_network(merge, pairs))


def sorted_stage(n, p):
    """the comparators of stage p of R.batcher(n), in its order"""
    out, k = [], p
    while k >= 1:
        for j in range(k % p, n - k, 2 * k):
            for i in range(k):
                if i + j + k < n and (i + j) // (2 * p) == (i + j + k) // (2 * p):
                    out.append((i + j, i + j + k))
        k //= 2
    return out


def test_networks_give_the_lower_median_with_inf_padding():
    """what the kernel does with them: +inf for a view that does not vote, then key (c - 1) // 2"""
    rng = np.random.Generator(np.random.PCG64(3))
    for n, net in ((9, R.NET9), (16, R.batcher(16)), (32, R.batcher(32))):
        keys = np.floor(rng.random((500, n)) * 6).astype(np.float32)
        vote = rng.random((500, n)) < 0.6
        vote[:, 0] |= ~vote.any(1)
        out = R.apply_network(net, np.where(vote, keys, np.inf))
        c = vote.sum(1)
        want = [np.sort(k[v])[(cc - 1) // 2] for k, v, cc in zip(keys, vote, c)]
        assert np.array_equal(out[np.arange(500), (c - 1) // 2], np.array(want, np.float32))
