"""GPU (-m gpu): the HRNet backward at shapes where the persistent weight-gradient kernels walk MORE THAN ONE work item per workgroup.

The oracle tests of test_gpu_backward.py use shapes small enough that every workgroup of conv_wgrad_kernel, conv_wgrad_x3_kernel and
stem_wgrad_kernel handles a single tile / strip, and the unrolled main loops of the colsum / PReLU reductions never run.  From the
second item on these kernels run code the first never reaches (the fp32 wgrad's register prefetch of the next tile and its second
register -> LDS store; the bf16x3 wgrad's new buffer descriptors and the restart of its LDS-DMA ring), so here:

  * test_hrnet_backward_multi_tile_vs_autograd_oracle: B = 3, V = 32 (5 fusion levels), 64 x 64, against fp64 autograd on the port,
    both precisions with every PReLU slope at 1 (the network is linear in its activations, nothing can flip sign: the kernels are
    held to the bounds of test_hrnet_backward_vs_autograd_oracle);
  * test_bf16x3_vs_fp32_gradients_at_train_shape: B = 32, V = 32, 64 x 64 (the shape bench.py trains), the only shape at which the
    bf16x3 wgrad walks several strips per workgroup; an fp64 oracle would take minutes there, so the bf16x3 gradients are held to
    the fp32 path's, which the first test pins with several tiles per workgroup (the two wgrad kernels share no code, only the
    finish kernel).

Each test first asserts, from the launchers' own formulas and the device's CU count, that the loops it is meant to cover do run.
"""
import time

import numpy as np
import pytest
import torch

from oracle import synth
import util

pytestmark = pytest.mark.gpu

_ONES = {k: 1.0 for k in util._SLOPE_KEYS}
RED_BLOCKS = 512                        # csrc/backward.hip: RED_BLOCKS, the grid of colsum_kernel / prelu_bwd_bias_kernel


def _cdiv(a, b):
    return -(-a // b)


def _cus():
    # the CU count the library sizes its grids with (csrc/prof.hip, hrn_device_cus: hipDeviceAttributeMultiprocessorCount)
    return torch.cuda.get_device_properties(0).multi_processor_count


def _wgrad_work(M, H, W, cus):
    """(work items, grid) of the three persistent weight-gradient kernels for M images of H x W, restating their launchers:
        conv_wgrad_kernel     8 x 32 px tiles,         grid = min(CUs, tiles)       csrc/backward.hip, hrn_launch_conv_wgrad
        conv_wgrad_x3_kernel  32-px column strips,     grid = min(2 CUs, units)     csrc/wgrad_x3.hip, hrn_launch_conv_wgrad_x3
        stem_wgrad_kernel     8 x 32 px tiles,         grid = min(4 CUs, tiles)     csrc/backward.hip, hrn_launch_stem_wgrad_sub
    Each workgroup walks items blockIdx.x, blockIdx.x + grid, ..."""
    tiles = _cdiv(W, 32) * _cdiv(H, 8) * M
    units = _cdiv(W, 32) * M
    return {"fp32": (tiles, min(cus, tiles)), "bf16x3": (units, min(2 * cus, units)), "stem": (tiles, min(4 * cus, tiles))}


def _colsum_unrolled(rows, C):
    # colsum_kernel: thread row r = blockIdx.x * RP + rp, stride = grid * RP, RP = 1024 / C; the 4-way loop runs while r + 3 stride < rows
    return rows > 3 * RED_BLOCKS * (1024 // C)


def _prelu_unrolled(rows, C):
    # prelu_bwd_bias_kernel: the same mapping; its 2-way loop runs while r + stride < rows
    return rows > RED_BLOCKS * (1024 // C)


def _levels(V):
    # views entering each fusion level (csrc/train.hip, train_ws): n -> n / 2 while n / 2 > 0
    n, out = V, []
    while n // 2 > 0:
        out.append(n)
        n //= 2
    return out


# ----------------------------------------------------------------------------- fp64 oracle at B = 3, V = 32, 64 x 64
_MT = dict(B=3, V=32, S=64, n_real=[32, 29, 17])
_oracle_cache = {}                      # one oracle run serves both precisions (~16 s of fp64 autograd)


def _multi_tile_oracle():
    if not _oracle_cache:
        B, V, S = _MT["B"], _MT["V"], _MT["S"]
        lrs, alphas, _ = synth.make_batch(5, B, V, S, _MT["n_real"])
        cot = np.random.Generator(np.random.PCG64(77)).standard_normal((B, 1, 3 * S, 3 * S)).astype(np.float32)
        t0 = time.perf_counter()
        want_sr, want = util._oracle_grads(lrs, alphas, cot, True, slopes=_ONES)
        _oracle_cache.update(lrs=lrs, alphas=alphas, cot=cot, want_sr=want_sr, want=want, seconds=time.perf_counter() - t0)
    return _oracle_cache


@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
def test_hrnet_backward_multi_tile_vs_autograd_oracle(prec):
    """B = 3, V = 32 with 32 / 29 / 17 real views (padded views in a 5-level tree: G[0] / G[1] swap five times), 64 x 64, the alpha
    residual, every PReLU slope at 1; forward and every gradient against fp64 autograd, at the bounds of
    test_hrnet_backward_vs_autograd_oracle (tensors 2e-4 of their max-norm, single slopes and the final bias 2e-5 of the oracle's
    sum |terms|).  With 256 CUs the fp32 wgrad walks 6 tiles per workgroup in the encoder and 3 at fusion level 1, the stem wgrad's
    1536 tiles exceed its grid of 1024, and the colsum / PReLU reductions run their unrolled loops (asserted below for this device)."""
    B, V, S = _MT["B"], _MT["V"], _MT["S"]
    M, levels, cus = B * V, _levels(V), _cus()
    assert len(levels) == 5, levels
    enc, lvl1 = _wgrad_work(M, S, S, cus), _wgrad_work(B * (V // 2), S, S, cus)
    for name, (items, grid) in (("encoder", enc["fp32"]), ("fusion level 1", lvl1["fp32"])):
        assert items >= 2 * grid, f"fp32 wgrad, {name}: {items} tiles on a grid of {grid} (CUs {cus}): some workgroup walks one tile"
    assert enc["stem"][0] > enc["stem"][1], ("stem wgrad: no workgroup walks a second tile", enc["stem"], cus)
    assert _colsum_unrolled(M * S * S, 64)                                  # encoder.final bias
    assert _prelu_unrolled(M * S * S, 64)                                   # encoder PReLUs
    assert all(_prelu_unrolled(B * (n // 2) * S * S, 128) for n in levels)  # every fusion level's 128-channel PReLUs

    o = _multi_tile_oracle()
    lrs, alphas, cot, want = o["lrs"], o["alphas"], o["cot"], o["want"]
    m = util._fresh_model(True, precision=prec, slopes=_ONES)
    t0 = time.perf_counter()
    sr = m(util.dev(lrs), util.dev(alphas))
    (sr * util.dev(cot)).sum().backward()
    torch.cuda.synchronize()
    t_gpu = time.perf_counter() - t0
    fwd = util.rel_err(sr.detach().cpu().numpy(), o["want_sr"])
    abs_terms = want["__abs_terms__"]
    tens, scal = {}, {}
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        got = p.grad.cpu().numpy()
        if p.numel() == 1:
            scal[k] = abs(float(got.ravel()[0]) - float(want[k].ravel()[0])) / max(abs_terms.get(k, 0.0), 1e-30)
        else:
            tens[k] = util.rel_err(got, want[k])
    top = lambda d: sorted(d.items(), key=lambda kv: -kv[1])[:3]
    print(f"multi-tile {prec}: oracle {o['seconds']:.1f} s, HIP fwd+bwd {t_gpu:.2f} s; forward {fwd:.2e}; worst tensor errors "
          f"{top(tens)}; worst scalar errors / sum|terms| {top(scal)}")
    assert fwd <= (2e-5 if prec == "fp32" else 1e-4), fwd
    for k, e in tens.items():
        assert e <= 2e-4, (k, e)
    for k, e in scal.items():
        assert abs_terms.get(k, 0.0) > 0 and e <= 2e-5, (k, e, abs_terms.get(k))
    # a second backward pass accumulates into .grad
    sr2 = m(util.dev(lrs), util.dev(alphas))
    (sr2 * util.dev(cot)).sum().backward()
    for k, p in m.named_parameters():
        if p.numel() > 1:
            assert util.rel_err(p.grad.cpu().numpy(), 2 * want[k]) <= 2e-4, k


# ----------------------------------------------------------------------------- bf16x3 against fp32 at B = 32, V = 32, 64 x 64
def test_bf16x3_vs_fp32_gradients_at_train_shape():
    """The training shape (B = 32, V = 32, 64 x 64), every PReLU slope at 1, the same weights, inputs and cotangent through both HIP
    training precisions: every bf16x3 gradient against the fp32 path's.  Here the bf16x3 wgrad walks 4 strips per workgroup in the
    encoder (2048 units on 512 workgroups) and 2 at fusion level 1 (1024 units), against one at every oracle-checked shape.
    Bounds: forward 1.2e-4 of the fp32 output's max-norm (the two paths' fp64 bounds, 1e-4 + 2e-5; measured 4.2e-5); tensors 2e-4 of
    the fp32 tensor's max-norm (measured worst 1.25e-4, encode.res_layers.1.block.2.bias: a bias gradient sums 4M pixels of the
    propagated gradient, whose split-bf16 error grows with the batch - 6.6e-5 against fp64 at B = 3 in the test above); the
    single-slope gradients, which have no sum |terms| here, to 3e-4 of the largest |slope gradient| of the model (measured worst
    6.0e-5, fuse.fuse.2.weight: ~5x headroom; these sums cancel heavily, at B = 3 both paths are within 5e-8 of their sum |terms|),
    the final bias - the sum of the cotangent in both paths - along with them.  A wgrad that reads the wrong image for any later unit
    is off by O(1) here."""
    B, V, S = 32, 32, 64
    cus = _cus()
    enc, lvl1 = _wgrad_work(B * V, S, S, cus)["bf16x3"], _wgrad_work(B * (V // 2), S, S, cus)["bf16x3"]
    for name, (items, grid) in (("encoder", enc), ("fusion level 1", lvl1)):
        assert items >= 2 * grid, f"bf16x3 wgrad, {name}: {items} units on a grid of {grid} (CUs {cus}): some workgroup walks one unit"
    lrs, alphas, _ = synth.make_batch(9, B, V, S, [V - 3 * (i % 8) for i in range(B)])
    cot = np.random.Generator(np.random.PCG64(78)).standard_normal((B, 1, 3 * S, 3 * S)).astype(np.float32)
    out, grads = {}, {}
    for prec in ("fp32", "bf16x3"):
        m = util._fresh_model(True, precision=prec, slopes=_ONES)
        sr = m(util.dev(lrs), util.dev(alphas))
        (sr * util.dev(cot)).sum().backward()
        out[prec] = sr.detach().cpu().numpy()
        grads[prec] = {k: p.grad.cpu().numpy().astype(np.float64) for k, p in m.named_parameters()}
        del m, sr
        torch.cuda.empty_cache()
    ref, got = grads["fp32"], grads["bf16x3"]
    slope_scale = max(abs(float(v.ravel()[0])) for k, v in ref.items() if v.size == 1 and k != "decode.final.bias")
    fwd = util.rel_err(out["bf16x3"], out["fp32"])
    tens = {k: util.rel_err(got[k], v) for k, v in ref.items() if v.size > 1}
    scal = {k: abs(float(got[k].ravel()[0]) - float(v.ravel()[0])) / slope_scale for k, v in ref.items() if v.size == 1}
    top = lambda d: sorted(d.items(), key=lambda kv: -kv[1])[:3]
    print(f"bf16x3 vs fp32 at B={B}, V={V}, {S}x{S}: forward {fwd:.2e}; worst tensor errors {top(tens)}; worst scalar errors / "
          f"largest |slope gradient| ({slope_scale:.3e}) {top(scal)}")
    assert fwd <= 1.2e-4, fwd
    for k, e in tens.items():
        assert e <= 2e-4, (k, e)
    for k, e in scal.items():
        assert e <= 3e-4, (k, e)
