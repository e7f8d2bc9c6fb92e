"""conv3x3_r64 (bf16 64 -> 64, the encoder's kernel) on v_mfma_f32_16x16x32_bf16: the shapes at which its fragment and epilogue mapping
can go wrong, per element against fp64.

The kernel is launched on its own through hrn_kt_conv3x3_epi (route 0), without residual (conv3x3_r64<false>) and with res_mode 1 in
place, out == res (conv3x3_r64<true>).  Reference: kernel_refs.ref_conv_epi in fp64 on the exact values the kernel read; bound per
element: half a bf16 ulp of the output + C = 1e-5 times the sum of |terms| (kernel_bounds).  Every tensor sits in a sentinel-guarded
buffer, every launch runs twice on identical buffers and the two results are compared bit for bit, and every launch is checked to have
been the r64 family's (the profiler's launch count), not the general kernel's.

What each test is for (a wave's tile is 2 pixel rows x 32 pixels as 4 pixel blocks of 16; a lane pair exchanges so that a lane owns 16
bytes of one pixel; a store instruction covers 8 whole pixel rows; the kernel's tile is 8 x 32, its halo tile 10 x 34):
  test_block_edges      H in {7, 8, 9} x W in {15, 16, 17, 31, 32, 33, 47, 48, 49}: image edges on, one before and one behind every
                        16-pixel block edge and the tile's edge; both variants, the three activation paths
  test_halo_forms       3 images of 24 x 96: interior tiles (fast halo form), border tiles (fast form + fix_borders), the first and the
                        last tile of the tensor (general form) in one launch; every pixel compared, the rows next to each image
                        boundary among them
  test_many_tiles       M = 4 x CUs + 3 images of 8 x 32 (one tile each): every team walks two tiles at least, some a third, the last
                        round is ragged; both variants, the residual in place
  test_ragged_widths    widths 33, 34, 35 at H = 9: the per-lane guard of the whole-line stores
  test_lane_exchange    zero input, bias = channel (and a residual of 64 k, k from the pixel's position): the outputs are small
                        integers, exact in bf16, compared exactly - a wrong exchange or a wrong residual lane shows as a permuted
                        channel or pixel
"""
import functools

import pytest
import torch

import kernel_refs as K
from kernel_bounds import BF16, Ten, _assert_close, _nchw
from kt import _cus, _launches, _p, _stream, lib as _lib

pytestmark = pytest.mark.gpu

SLOPE_CLASSES = (K.SLOPES[0], K.SLOPES[1], K.SLOPES[4])       # no PReLU | 0 <= a <= 1 | the general path
assert SLOPE_CLASSES[0] is None and 0.0 <= SLOPE_CLASSES[1] <= 1.0 and SLOPE_CLASSES[2] < 0.0


@functools.lru_cache(maxsize=4)
def _operands(M, H, W, seed):
    """the fp32 CPU operands of a case (bf16-exact) and the fp64 pre-activation of the layer with its T: shared by every launch of the
    case and never modified"""
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn((64, 64, 3, 3), generator=g) * 0.05).to(torch.bfloat16).float()
    bias = (torch.randn(64, generator=g) * 0.1).to(torch.bfloat16).float()
    x = torch.randn((M, H, W, 64), generator=g).to(torch.bfloat16).float()
    res = torch.randn((M, H, W, 64), generator=g).to(torch.bfloat16).float()
    y, T = K.ref_conv_epi(x.double(), w.double(), bias.double(), None, 0)
    return w, bias, x, res, y, T


def _launch(w, bias, x, res, slope, M, H, W):
    """one launch -> (the output buffer, the input buffer).  res None: res_mode 0 into a sentinel-filled output; else in place"""
    lib = _lib()
    wd, bd = w.cuda(), bias.cuda()
    pk = torch.empty(64 * 64 * 9, dtype=torch.bfloat16, device="cuda")
    assert lib.hrn_kt_conv_pack(BF16, 64, 64, _p(wd), _p(pk), _stream()) == 0
    inp = Ten((M, H, W, 64), BF16, v=x)
    out = Ten((M, H, W, 64), BF16, v=res)
    sd = None if slope is None else torch.tensor([slope], dtype=torch.float32, device="cuda")
    res_mode = 0 if res is None else 1

    def go():
        return lib.hrn_kt_conv3x3_epi(BF16, 0, 64, 64, inp.ptr, None, 0, 0, 0, _p(pk), _p(bd), _p(sd), out.ptr if res_mode else None, res_mode,
                                      0, None, 0, out.ptr, 0, 0, 0, 0, 0, 0, M, H, W, _stream())

    counts, rc = _launches(go)
    assert rc == 0, rc
    fam = "prof:conv3x3_bf16_64x64+res" if res_mode else "prof:conv3x3_bf16_64x64"
    assert counts.get(fam) == 1 and counts["conv_general"] == 0, counts
    assert inp.unchanged(), "the launch wrote its input"
    assert out.guard_ok(), "a write past the output"
    return out


def _check(tag, M, H, W, seed, variants=(False, True), slopes=SLOPE_CLASSES):
    w, bias, x, res, y, T = _operands(M, H, W, seed)
    for with_res in variants:
        for slope in slopes:
            first = _launch(w, bias, x, res if with_res else None, slope, M, H, W)
            second = _launch(w, bias, x, res if with_res else None, slope, M, H, W)
            name = f"{tag} {'r64res' if with_res else 'r64'} M={M} {H}x{W} slope={slope}"
            assert torch.equal(first.raw, second.raw), f"{name}: two runs differ"
            want, Tw = K.ref_prelu_fwd(y, T, slope)
            if with_res:
                want, Tw = want + _nchw(res.double()), Tw + _nchw(res.double()).abs()
            _assert_close(name, "bf16", _nchw(first.value()), want, Tw)


@pytest.mark.parametrize("H", [7, 8, 9])
@pytest.mark.parametrize("W", [15, 16, 17, 31, 32, 33, 47, 48, 49])
def test_block_edges(H, W):
    _check("edges", 1, H, W, 1000 + 64 * H + W)


def test_halo_forms():
    _check("halo", 3, 24, 96, 2001, variants=(False,), slopes=(SLOPE_CLASSES[1],))


def test_many_tiles():
    M = 4 * _cus() + 3
    _check("tiles", M, 8, 32, 2002, slopes=(SLOPE_CLASSES[1],))


@pytest.mark.parametrize("W", [33, 34, 35])
def test_ragged_widths(W):
    _check("ragged", 2, 9, W, 2100 + W, slopes=(SLOPE_CLASSES[2],))


def test_lane_exchange():
    M, H, W = 2, 9, 35
    w = (torch.randn((64, 64, 3, 3), generator=torch.Generator().manual_seed(5)) * 0.05).to(torch.bfloat16).float()
    bias = torch.arange(64, dtype=torch.float32)
    x = torch.zeros((M, H, W, 64))
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    k = ((xx + 3 * yy) % 4).float()                                   # differs between the pixels a lane pair and a quad of lanes own
    res = (64.0 * k)[None, :, :, None].expand(M, H, W, 64).contiguous()
    for r in (None, res):
        out = _launch(w, bias, x, r, None, M, H, W)
        again = _launch(w, bias, x, r, None, M, H, W)
        assert torch.equal(out.raw, again.raw), "two runs differ"
        want = bias[None, None, None, :].expand(M, H, W, 64) + (0 if r is None else r)
        got = out.value().float()
        bad = torch.nonzero(got != want)
        assert bad.numel() == 0, (f"{'r64res' if r is not None else 'r64'}: {bad.shape[0]} elements differ; first (m, y, x, c) = {bad[0].tolist()}: "
                                  f"got {float(got[tuple(bad[0])])}, want {float(want[tuple(bad[0])])}")
