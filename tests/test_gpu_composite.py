"""GPU (-m gpu): hrn_masked_composite (csrc/composite.hip) against its numpy restatement (tests/composite_ref.py), bit for bit: ref, count
and filled, over shapes that take each of the three sorting networks, partial blocks and several blocks per sample; against the
network's own median; reproducibility; independence of the batch; the dispatcher op."""
import numpy as np
import pytest
import torch

import composite_ref as R
import kt
import util

pytestmark = pytest.mark.gpu

# (1, 13, 5, 7) and (1, 24, 5, 7): n = min(V, n_ref) strictly inside 10..15 and 18..31, keys of the 16- and 32-key networks that are padding
SHAPES = [(2, 1, 5, 7), (2, 2, 5, 7), (1, 9, 16, 16), (2, 10, 9, 33), (1, 17, 8, 8), (2, 32, 16, 16), (1, 13, 5, 7), (1, 24, 5, 7)]
N_REFS = [1, 5, 9, 16, 17, 32]
_cases = {}


def _case(shape, family="eighths"):
    """(views, masks, alphas) of a shape, numpy f32; made once, shared, never modified.  Values, family "eighths": non-negative eighths
    (ties, no -0.0); family "signed": eighths in [-1.5, 1.5) (ties, both signs, no -0.0) with about 2 % of them +inf - a voter that is
    +inf sorts among the +inf keys of the views that do not vote, and the result is still the restatement's.
    Masks: ~60 % clear, with pixels forced to no candidate, exactly one, and all.  Alphas: trailing zeros; with B = 2 the second sample
    has no real view at all."""
    if (shape, family) not in _cases:
        B, V, H, W = shape
        rng = np.random.Generator(np.random.PCG64(sum(shape)))
        if family == "eighths":
            views = np.floor(rng.random(shape) * 24).astype(np.float32) / 8
        else:
            assert family == "signed", family
            views = (np.floor(rng.random(shape) * 24) - 12).astype(np.float32) / 8 + np.float32(0.0)
            views[rng.random(shape) < 0.02] = np.inf
            views[0, 0, H // 2, W // 2], views[0, 0, H // 2, W // 2 + 1] = -1.5, np.inf      # both ends present whatever the shape
            assert not np.signbit(views[views == 0]).any()
        masks = (rng.random(shape) < 0.6).astype(np.float32)
        masks[:, :, 0, 0] = 0                                    # no candidate
        masks[:, :, 0, 1] = 0
        masks[:, (V - 1) // 2, 0, 1] = 1                         # exactly one (where that view is real)
        masks[:, 0, 0, 2] = 1
        masks[:, 1:, 0, 2] = 0                                   # exactly one: the first view
        masks[:, :, 0, 3] = 1                                    # all
        masks[:, :, H - 1, W - 1] = 0
        masks = masks * np.float32(2.5)                          # "non-zero", not 1
        alphas = np.ones((B, V), np.float32)
        alphas[0, max(1, (2 * V) // 3):] = 0                     # n_real < V (and < n_ref for the larger n_ref)
        if B > 1:
            alphas[1] = 0                                        # n_real = 0
        _cases[(shape, family)] = (views, masks, alphas)
    return _cases[(shape, family)]


def _run(views, masks, alphas, n_ref, count=True, fill=True):
    from hrnet_hip import binding
    d = lambda t: None if t is None else util.dev(t)
    ref, filled, cnt = binding.masked_composite(d(views), d(masks), d(alphas), n_ref, count, fill)
    torch.cuda.synchronize()
    return ref, filled, cnt


def _same(t, want):
    return t.dtype == torch.float32 and np.array_equal(t.cpu().numpy().view(np.uint32), np.ascontiguousarray(want).view(np.uint32))


def _check_restatement(views, masks, alphas, n_ref):
    for m, a in ((masks, alphas), (masks, None), (None, alphas), (None, None)):
        want_ref, want_count, want_filled = R.masked_composite(views, m, a, n_ref)
        ref, filled, cnt = _run(views, m, a, n_ref)
        assert _same(ref, want_ref), ("ref", m is None, a is None)
        assert _same(cnt, want_count), ("count", m is None, a is None)
        assert _same(filled, want_filled), ("filled", m is None, a is None)
    # count / filled left out: the same ref, and nothing else comes back
    want_ref = R.masked_composite(views, masks, alphas, n_ref)[0]
    for count, fill in ((False, True), (True, False), (False, False)):
        ref, filled, cnt = _run(views, masks, alphas, n_ref, count, fill)
        assert _same(ref, want_ref) and (filled is None) == (not fill) and (cnt is None) == (not count)


@pytest.mark.parametrize("n_ref", N_REFS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_composite_equals_the_restatement(shape, n_ref):
    views, masks, alphas = _case(shape)
    _check_restatement(views, masks, alphas, n_ref)
    if shape == SHAPES[3]:                                       # the forced pixels are what they are meant to be (sample 0: real views)
        cnt = R.masked_composite(views, masks, alphas, 32)[1]
        n_real = int((alphas[0] != 0).sum())
        assert cnt[0, 0, 0] == 0 and cnt[0, 0, 1] == 1 and cnt[0, 0, 2] == 1 and cnt[0, 0, 3] == n_real and (cnt[1] == 0).all()


@pytest.mark.parametrize("n_ref", N_REFS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_composite_signed_values_and_inf_voters(shape, n_ref):
    """the second value family: negative values, and voters equal to the +inf key of a view that does not vote"""
    views, masks, alphas = _case(shape, "signed")
    _check_restatement(views, masks, alphas, n_ref)
    if shape == (2, 32, 16, 16) and n_ref == 32:                 # the family does what it is for: +inf among the voters of the 32-key sort
        n_real = int((alphas[0] != 0).sum())
        assert ((masks[0, :n_real] != 0) & np.isinf(views[0, :n_real])).any()
    if shape == (2, 10, 9, 33) and n_ref == 16:                  # ... and as the median itself
        assert np.isinf(R.masked_composite(views, masks, alphas, n_ref)[0]).any()


@pytest.mark.parametrize("shape", SHAPES + [(3, 12, 40, 56)], ids=lambda s: "x".join(map(str, s)))
def test_unmasked_n9_is_the_networks_median(shape):
    views = _case(shape)[0] if shape in SHAPES else np.floor(np.random.Generator(np.random.PCG64(1)).random(shape) * 24).astype(np.float32) / 8
    B, V, H, W = shape
    x = util.dev(views)
    med = torch.empty((B, H, W), dtype=torch.float32, device="cuda")
    assert kt.lib().hrn_kt_median(kt._p(x), kt._p(med), B, V, H, W, kt._stream()) == 0
    ref, filled, cnt = _run(views, None, None, 9)
    assert torch.equal(ref.view(torch.int32), med.view(torch.int32))
    assert torch.equal(filled, x) and bool((cnt == min(V, 9)).all())


def test_two_runs_are_bit_equal_and_a_sample_does_not_depend_on_its_batch():
    shape = (2, 32, 16, 16)
    views, masks, alphas = _case(shape)
    for n_ref in (9, 16, 32):
        a = _run(views, masks, alphas, n_ref)
        b = _run(views, masks, alphas, n_ref)
        assert all(torch.equal(s, t) for s, t in zip(a, b))
        for i in range(2):
            one = _run(views[i:i + 1], masks[i:i + 1], alphas[i:i + 1], n_ref)
            assert all(torch.equal(s[0], t[i]) for s, t in zip(one, a)), (n_ref, i)


def test_public_surface_and_opcheck():
    from hrnet_hip import composite
    views, masks, alphas = _case((2, 10, 9, 33))
    x, m, a = util.dev(views), util.dev(masks), util.dev(alphas)
    want = R.masked_composite(views, masks, alphas, 9)
    ref, filled = composite.masked_composite(x, m, a)
    assert _same(ref, want[0]) and _same(filled, want[2])
    ref, filled, cnt = composite.masked_composite(x.double(), m.bool(), a, n_ref=9, return_count=True, fill=False)
    assert _same(ref, want[0]) and filled is None and _same(cnt, want[1])
    ref, filled = composite.masked_composite(x.requires_grad_(True), m, a)
    assert not ref.requires_grad and not filled.requires_grad             # the frame is data
    ops = torch.ops.hrnet_hip
    x = x.detach()
    for args in ((x, m, a, 9, True, True), (x, None, None, 16, False, True), (x, m, None, 5, True, False)):
        torch.library.opcheck(ops.masked_composite.default, args, test_utils=("test_schema", "test_faketensor"))
