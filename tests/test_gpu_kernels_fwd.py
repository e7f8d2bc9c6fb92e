"""GPU (-m gpu): the bf16 and bf16x3 forward kernels, per element, against torch CPU float64.

Each kernel is launched on its own through the hooks of kernel_test.h, bound by tests/kt.py (hrn_kt_conv3x3_epi with the epilogue encoder_impl / fuse_impl set in ConvParams,
hrn_kt_stem, hrn_kt_decoder), with operands chosen so that the kernel's products are exact and only the accumulation order and the
rounding of the stored output remain:
  bf16     activations, weights, bias, slope and alpha bf16-representable;
  bf16x3   activations hi + lo planes of random fp32 values (the view stack, a residual, with 16 significant bits: hi + lo is then exact in
           fp32 and an alpha = 0 slot can be compared bit for bit), weights either bf16-exact (lo = 0: every product exact) or general
           fp32 (the W lo x X hi pass; the dropped lo x lo term is <= 2^-18 of |x w|);
  stem     inputs k / 2^16 (16 significant bits: hi + lo exact), bias of that form, weights bf16 (bf16) or general fp32 (bf16x3).
Bound per element, T = the same expression evaluated on absolute values (sum |terms| of the conv + |bias|, times max(1, |a|) through the
PReLU; with a residual |r| + |alpha| times that; torch_port.ABS_TERMS per element):
  bf16 storage     |got - want| <= 1/2 ulp_bf16(max(|got|, |want|)) + C T     (half an ulp: truncation and double rounding fail)
  bf16x3 (hi + lo) |got - want| <= 2^-16 |want| + C T
  decoder (fp32)   |got - want| <= C T
with one C (kernel_bounds.C) for the whole file and the two that follow it.  Every test prints its worst error / bound.

Template instance -> production call site -> tests
  stem_mfma_kernel<false> / <true>   encoder_impl (api.hip), bf16 / bf16x3          test_stem[bf16-*], test_stem[bf16x3-*]
  stem_kernel<BF16> (`sub`)          ShiftNet's bf16 training stem                   test_stem[bf16sub-*]
  conv3x3_r64<false> / <true>        encoder_impl: conv 1 / conv 2 (res_mode 1 in place), the encoder's final conv
                                                                                     test_conv[r64-*], test_conv[r64res-*]
  conv3x3_v6<128,128,0,true>         fuse_impl convA (pair gather in)                test_conv[v6pairin-*]
  conv3x3_v6<128,128,2,false>        fuse_impl convB (pair residual)                 test_conv[v6pairres-*]
  conv3x3_v6<128,64,3,false>         fuse_impl output conv, alpha residual           test_conv[v6alpha-*], test_conv[v6alphalast-*]
  conv3x3_v6<128,64,0,false>         fuse_impl output conv, alpha_residual False      test_conv[v6slot-*], test_conv[v6slotlast-*]
  conv3x3_v6x3 (same four, <64,64,0|1,false>)  the same call sites in bf16x3         test_conv[x3*-*]
  conv3x3_kernel<BF16, CI, CO>       the route HRN_CONV_R64=0 HRN_CONV_V6=0 select   test_conv[gen*-*]
  decoder_kernel<BF16, false, S>     decoder_impl, bf16                              test_decoder[bf16-S*]
  decoder_kernel<F32, true, S>       decoder_impl, bf16x3 (the split decoder)        test_decoder[bf16x3-S*]
Negative controls (test_negative_control) run on the CPU against the same GPU output and assert that the comparison FAILS.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from kernel_bounds import BF, GUARD, SENT, SHAPES, _assert_close, _grid, _nchw, _pair_gather, _ratio, _tiles, _ulp_bf16
from kt import BF16, BF16X3, _p, _stream, lib as _lib

pytestmark = pytest.mark.gpu

PAD = 1024                  # gap in front of a lo plane: its offset is never the plane's size (as fuse_impl's t1 / t2)
# slope classes: None (no PReLU), ACT 1 (0 <= a <= 1) and ACT 2 (a < 0 or a > 1) of conv3x3_r64, v6's act_pick for a > 1
SLOPES = [None, 0.25, 0.0, 1.0, BF(-0.3), 1.5]


# ----------------------------------------------------------------------------------------------------------- tensors and bounds
class Act:
    """an activation tensor in storage dt inside a sentinel-filled int16 device buffer: the hi plane [0, n), GUARD sentinels; bf16x3:
    PAD sentinels, the lo plane at lo_off bytes, GUARD sentinels.  val: the exact fp64 CPU value (hi + lo)."""

    def __init__(self, shape, dt, seed=None, scale=1.0, bits16=False):
        self.shape, self.dt = tuple(shape), dt
        self.n = int(np.prod(shape))
        self.lo_e = self.n + GUARD + PAD if dt == BF16X3 else 0
        total = self.lo_e + self.n + GUARD if dt == BF16X3 else self.n + GUARD
        self.raw = torch.full((total,), SENT, dtype=torch.int16, device="cuda")
        self.lo_off = 2 * self.lo_e
        self.val = None
        if seed is not None:
            v = torch.randn(self.shape, generator=torch.Generator().manual_seed(seed)) * scale
            if dt == BF16:
                hi, lo = v.to(torch.bfloat16), None
            else:
                if bits16:      # 16 significant bits: hi + lo == v exactly, in fp32 too
                    v = (v.view(torch.int32) & ~0xFF).view(torch.float32)
                hi = v.to(torch.bfloat16)
                lo = (v - hi.float()).to(torch.bfloat16)
            self.raw[:self.n] = hi.reshape(-1).view(torch.int16).cuda()
            if lo is not None:
                self.raw[self.lo_e:self.lo_e + self.n] = lo.reshape(-1).view(torch.int16).cuda()
            self.val = hi.double() + (lo.double() if lo is not None else 0)

    @property
    def ptr(self):
        return _p(self.raw)

    def planes(self):
        """-> (hi, lo or None) as int16 CPU tensors of self.shape"""
        raw = self.raw.cpu()
        hi = raw[:self.n].reshape(self.shape)
        lo = raw[self.lo_e:self.lo_e + self.n].reshape(self.shape) if self.dt == BF16X3 else None
        return hi, lo

    def value(self):
        hi, lo = self.planes()
        v = hi.view(torch.bfloat16).double()
        return v + lo.view(torch.bfloat16).double() if lo is not None else v

    def guards_intact(self):
        pieces = [self.raw[self.n:self.n + GUARD]]
        if self.dt == BF16X3:
            pieces += [self.raw[self.n + GUARD:self.lo_e], self.raw[self.lo_e + self.n:]]
        return all(bool((p == SENT).all()) for p in pieces)


def _prelu(x, T, a):
    if a is None:
        return x, T
    return torch.where(x >= 0, x, a * x), T * max(1.0, abs(a))


def _slope_dev(a):
    return None if a is None else torch.tensor([a], dtype=torch.float32, device="cuda")


# ----------------------------------------------------------------------------------------------------------- the convolutions
# instance: (dt, route, cin, cout, res_mode, in_pair, slot output)
INSTANCES = {
    "r64": (BF16, 0, 64, 64, 0, False, False),
    "r64res": (BF16, 0, 64, 64, 1, False, False),
    "v6pairin": (BF16, 0, 128, 128, 0, True, False),
    "v6pairres": (BF16, 0, 128, 128, 2, False, False),
    "v6alpha": (BF16, 0, 128, 64, 3, False, "stack"),
    "v6alphalast": (BF16, 0, 128, 64, 3, False, "fused"),
    "v6slot": (BF16, 0, 128, 64, 0, False, "stack"),
    "v6slotlast": (BF16, 0, 128, 64, 0, False, "fused"),
    "x3enc": (BF16X3, 0, 64, 64, 0, False, False),
    "x3encres": (BF16X3, 0, 64, 64, 1, False, False),
    "x3pairin": (BF16X3, 0, 128, 128, 0, True, False),
    "x3pairres": (BF16X3, 0, 128, 128, 2, False, False),
    "x3alpha": (BF16X3, 0, 128, 64, 3, False, "stack"),
    "x3alphalast": (BF16X3, 0, 128, 64, 3, False, "fused"),
    "x3slot": (BF16X3, 0, 128, 64, 0, False, "stack"),
    "x3slotlast": (BF16X3, 0, 128, 64, 0, False, "fused"),
    "gen64": (BF16, 1, 64, 64, 0, False, False),
    "gen64res": (BF16, 1, 64, 64, 1, False, False),
    "genpairin": (BF16, 1, 128, 128, 0, True, False),
    "genpairres": (BF16, 1, 128, 128, 2, False, False),
    "genalpha": (BF16, 1, 128, 64, 3, False, "stack"),
}


def _conv_case(name, shape, seed, slope=None, alphas="mix", wset="bf16", ctrl=None):
    """Launch instance `name` at `shape`; -> dict with the GPU output (fp64), the reference and T, plus what a control needs"""
    dt, route, cin, cout, res_mode, in_pair, slot = INSTANCES[name]
    lib = _lib()
    H, W = SHAPES[shape]
    uses_stack = in_pair or res_mode in (2, 3) or slot
    # view stack: B samples x V slots; a level of n views (pair_last = n - 2 for odd n) inside it, pair_vs = V > n
    n = 3 if slot == "fused" else 5
    V = n + 2
    half, pair_last = n // 2, n - (n & 1) - 1
    per = half if uses_stack else 1
    if shape == "multi":
        tiles = _tiles(dt, route, cin, cout, H, W)
        B = 1
        while (B * per * tiles) < 2 * _grid(route, cout, B * per * tiles):
            B += 1
        B += 1
    else:
        B = 2 if shape != "1x1" or uses_stack else 1
    M = B * per
    total = M * _tiles(dt, route, cin, cout, H, W)
    if shape == "multi":
        assert total >= 2 * _grid(route, cout, total), (total, _grid(route, cout, total))
    x3 = dt == BF16X3
    kind = "x3" if x3 else "bf16"

    # operands
    g = torch.Generator().manual_seed(seed)
    w = torch.randn((cout, cin, 3, 3), generator=g) * (0.05 if cin == 64 else 0.035)
    if not x3 or wset == "bf16":
        w = w.to(torch.bfloat16).float()
    bias = torch.randn(cout, generator=g) * 0.1
    if not x3:
        bias = bias.to(torch.bfloat16).float()
    w64, b64 = w.double(), bias.double()
    wd, bd = w.cuda(), bias.cuda()
    pk = torch.empty(cin * cout * 9 * (2 if x3 else 1), dtype=torch.bfloat16, device="cuda")
    assert lib.hrn_kt_conv_pack(dt, cin, cout, _p(wd), _p(pk), _stream()) == 0

    stack = Act((B, V, H, W, 64), dt, seed + 1, bits16=True) if uses_stack else None
    stack0 = stack.planes() if stack is not None else None
    inp = None if in_pair else Act((M, H, W, cin), dt, seed + 2)
    if in_pair:
        x64 = _pair_gather(stack.val[:, :n], half, pair_last)
    else:
        x64 = inp.val
    # alphas [B][V]: 0, 1, 0.75 mixed in the batch (the partner of slot i is pair_last - i)
    alph = None
    if res_mode == 3 and alphas == "mix":
        pattern = [0.0, 1.0, 0.75, 0.75, 1.0, 0.0, 0.75]
        alph = torch.tensor([[pattern[(b + j) % 7] for j in range(V)] for b in range(B)], dtype=torch.float32)
    out_vs = 1 if slot == "fused" else V
    if slot == "stack":
        out, out_h = stack, half                                  # res_mode 3: in place, out == res == stack
    elif slot == "fused":
        out, out_h = Act((B, H, W, 64), dt), half                 # the last level: fused [B][H][W][64], the residual from the stack
    elif res_mode == 1:
        out, out_h = Act((M, H, W, cout), dt, seed + 3), 0        # in place: out == res, as the encoder's second conv
    else:
        out, out_h = Act((M, H, W, cout), dt), 0
    res_ptr, res_lo, res_vs = None, 0, 0
    if res_mode == 1:
        res_ptr, res_lo = out.ptr, out.lo_off
        r64 = out.val
    elif res_mode == 3:
        res_ptr, res_lo, res_vs = stack.ptr, stack.lo_off, V
    ad = alph.cuda() if alph is not None else None
    sd = _slope_dev(slope)
    pair_h = half if (in_pair or res_mode == 2) else 0
    rc = lib.hrn_kt_conv3x3_epi(dt, route, cin, cout, None if in_pair else inp.ptr, stack.ptr if stack is not None else None, pair_h,
                                pair_last, V if uses_stack else 0, _p(pk), _p(bd), _p(sd), res_ptr, res_mode, res_vs, _p(ad),
                                V if ad is not None else 0, out.ptr, out_h, out_vs if slot else 0, 0 if in_pair else inp.lo_off,
                                stack.lo_off if stack is not None else 0, out.lo_off, res_lo, M, H, W, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()

    # reference
    def reference(w64=w64, own_alpha=False, swap_halves=False):
        z = _nchw(x64)
        y = F.conv2d(z, w64, b64, padding=1)
        T = F.conv2d(z.abs(), w64.abs(), b64.abs(), padding=1)
        y, T = _prelu(y, T, slope)
        if res_mode == 1:
            y, T = y + _nchw(r64), T + _nchw(r64).abs()
        elif res_mode == 2:
            st = stack.val[:, :n]
            if swap_halves:
                idx = torch.arange(half)
                zz = torch.cat([st[:, pair_last - idx], st[:, idx]], -1).reshape((M, H, W, 128))
            else:
                zz = _pair_gather(st, half, pair_last)
            y, T = y + _nchw(zz), T + _nchw(zz).abs()
        elif res_mode == 3:
            r = _nchw(stack.val[:, :half].reshape(M, H, W, 64))
            if alph is None:
                al = torch.ones(M, dtype=torch.float64)
            else:
                i = torch.arange(half)
                al = (alph[:, i] if own_alpha else alph[:, pair_last - i]).reshape(M).double()
            al = al[:, None, None, None]
            y, T = r + al * y, r.abs() + al.abs() * T
        return y, T

    if slot == "stack":
        got = _nchw(out.value()[:, :half].reshape(M, H, W, 64))
    else:
        got = _nchw(out.value())
    want, T = reference()
    return dict(got=got, want=want, T=T, kind=kind, reference=reference, w64=w64, stack=stack, stack0=stack0, half=half, V=V, out=out,
                inp=inp, alph=alph, slot=slot, M=M, res_mode=res_mode, pair_last=pair_last)


# the case matrix: every instance at every shape; the slope class, the alphas (mixed / NULL) and the weight set (bf16x3: bf16-exact or
# general fp32) rotate over the shapes instead of taking the full product
CASES = []
for ii, name in enumerate(INSTANCES):
    for si, shape in enumerate(SHAPES):
        CASES.append(pytest.param(name, shape, SLOPES[(ii + si) % len(SLOPES)], "null" if (ii + si) % 4 == 3 else "mix",
                                  "fp32" if (ii + si) % 2 else "bf16", id=f"{name}-{shape}"))


@pytest.mark.parametrize("name,shape,slope,alphas,wset", CASES)
def test_conv(name, shape, slope, alphas, wset):
    r = _conv_case(name, shape, 100 + 7 * list(SHAPES).index(shape), slope=slope, alphas=alphas, wset=wset)
    tag = f"{name} {shape} slope={slope} alphas={alphas} w={wset}"
    _assert_close(tag, r["kind"], r["got"], r["want"], r["T"])
    out = r["out"]
    assert out.guards_intact(), f"{tag}: a write past the output"
    if r["stack"] is not None:
        st = r["stack"]
        assert st.guards_intact(), f"{tag}: a write past the view stack"
        hi0, lo0 = r["stack0"]
        hi1, lo1 = st.planes()
        keep = slice(r["half"], None) if r["slot"] == "stack" else slice(None)     # slots i >= half (or the whole stack) untouched
        assert torch.equal(hi0[:, keep], hi1[:, keep]) and (lo0 is None or torch.equal(lo0[:, keep], lo1[:, keep])), \
            f"{tag}: the launch wrote view-stack slots it does not own"
    if r["res_mode"] == 3 and r["alph"] is not None:
        # where the partner's alpha is 0 the slot IS its residual, bit for bit (both planes in bf16x3)
        M, half, pl = r["M"], r["half"], r["pair_last"]
        i = torch.arange(half)
        zero = (r["alph"][:, pl - i] == 0).reshape(M)
        if bool(zero.any()):
            hi0, lo0 = r["stack0"]
            ghi, glo = out.planes()
            res_hi = hi0[:, :half].reshape((M,) + tuple(hi0.shape[2:]))
            got_hi = ghi[:, :half].reshape(res_hi.shape) if r["slot"] == "stack" else ghi.reshape(res_hi.shape)
            assert torch.equal(got_hi[zero], res_hi[zero]), f"{tag}: alpha = 0 slot differs from its residual (hi plane)"
            if lo0 is not None:
                res_lo = lo0[:, :half].reshape(res_hi.shape)
                got_lo = glo[:, :half].reshape(res_hi.shape) if r["slot"] == "stack" else glo.reshape(res_hi.shape)
                assert torch.equal(got_lo[zero], res_lo[zero]), f"{tag}: alpha = 0 slot differs from its residual (lo plane)"


# ----------------------------------------------------------------------------------------------------------- negative controls
def _rz_bf16(x):
    """fp64 -> the bf16 value toward zero"""
    u = _ulp_bf16(x)
    return torch.sign(x) * torch.floor(x.abs() / u) * u


@pytest.mark.parametrize("control,name", [("tap_swap", "v6pairres"), ("tap_swap", "x3alpha"), ("tap_swap", "r64res"),
                                          ("round_to_zero", "r64"), ("round_to_zero", "v6alpha"),
                                          ("own_alpha", "v6alpha"), ("own_alpha", "x3alpha"), ("own_alpha", "genalpha"),
                                          ("swap_halves", "v6pairres"), ("swap_halves", "x3pairres"), ("swap_halves", "genpairres")])
def test_negative_control(control, name):
    """The comparison against a reference that is wrong in one way must FAIL on the same GPU output that passes against the right one:
    one (co, ci) pair with two taps swapped; the reference rounded toward zero (bf16); the view's own alpha instead of its partner's
    (res_mode 3); the pair residual with its 64-channel halves swapped (res_mode 2)."""
    r = _conv_case(name, "15x33", 321, slope=0.25, alphas="mix", wset="fp32")
    got, kind = r["got"], r["kind"]
    ok = _assert_close(f"{name} (right reference)", kind, got, r["want"], r["T"])
    if control == "tap_swap":
        w = r["w64"].clone()
        w[5, 7, 0, 0], w[5, 7, 2, 2] = r["w64"][5, 7, 2, 2], r["w64"][5, 7, 0, 0]
        assert w[5, 7, 0, 0] != w[5, 7, 2, 2]
        bad, T = r["reference"](w64=w)
    elif control == "round_to_zero":
        bad, T = _rz_bf16(r["want"]), r["T"]
    elif control == "own_alpha":
        bad, T = r["reference"](own_alpha=True)
    else:
        bad, T = r["reference"](swap_halves=True)
    worst, idx = _ratio(kind, got, bad, T)
    print(f"{control} {name}: error / bound against the wrong reference {worst:.3e} (right one {ok:.3e})")
    assert worst > 1.0, f"{control} {name}: the comparison does not tell the wrong reference from the right one"


# ----------------------------------------------------------------------------------------------------------- the stem
STEM_SHAPES = {"1x1": (1, 1, 3), "2x3": (2, 3, 4), "9x27": (9, 27, 3), "15x33": (15, 33, 2), "17x50": (17, 50, 2), "9x63": (9, 63, 3),
               "16x64": (16, 64, 2), "multi": (5, 70, None)}


def _k16(shape, g):
    """values k / 2^16, 0 <= k < 2^16: 16 significant bits"""
    return torch.randint(0, 1 << 16, shape, generator=g).double() / 65536.0


@pytest.mark.parametrize("mode", ["bf16", "bf16x3", "bf16sub"])
@pytest.mark.parametrize("shape", list(STEM_SHAPES))
def test_stem(mode, shape):
    """stem_mfma_kernel<false> (bf16), <true> (bf16x3) and the VALU stem_kernel<BF16> (`sub`): 2 -> 64 conv + PReLU of (view m, frame m / rep1)"""
    lib = _lib()
    H, W, M = STEM_SHAPES[shape]
    segs_x = -(-W // 32)
    if M is None:       # every wave walks two segments at least: nseg >= 2 x 32,768 and all three carries of advance() occur
        M = -(-2 * 32768 // (H * segs_x)) + 1
        nseg = M * H * segs_x
        waves = 4 * min(-(-nseg // 4), 8192)
        assert nseg >= 2 * waves and segs_x % 2 == 1 and (waves // segs_x) % H != 0, (nseg, waves)
    rep1 = 3
    dt = BF16 if mode != "bf16x3" else BF16X3
    g = torch.Generator().manual_seed(17 + M + H)
    x0 = _k16((M, H, W), g)
    x1 = _k16((-(-M // rep1), H, W), g)
    w = torch.randn((64, 2, 3, 3), generator=g) * 0.3
    if mode == "bf16":
        w = w.to(torch.bfloat16).float()        # (bf16x3 and the VALU stem take general fp32 weights)
    bias = (torch.randint(-(1 << 14), 1 << 14, (64,), generator=g).double() / 65536.0).float()
    slope = [None, 0.25, BF(-0.3), 1.5][list(STEM_SHAPES).index(shape) % 4]
    sub = _k16((M, 2), g) if mode == "bf16sub" else None
    out = Act((M, H, W, 64), dt)
    d0, d1, dw, db, ds = x0.float().cuda(), x1.float().cuda(), w.cuda(), bias.cuda(), _slope_dev(slope)
    dsub = sub.float().cuda() if sub is not None else None
    rc = lib.hrn_kt_stem(dt, _p(d0), H * W, _p(d1), rep1, H * W, _p(dsub), _p(dw), _p(db), _p(ds), out.ptr, out.lo_off, M, H, W, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert out.guards_intact()
    hi, lo = out.planes()
    kind = "x3" if dt == BF16X3 else "bf16"
    worst = 0.0
    w64, b64 = w.double(), bias.double()
    step = 512
    for m0 in range(0, M, step):          # in chunks of images: host memory stays small at the multi-item shape
        m1 = min(M, m0 + step)
        idx = torch.arange(m0, m1)
        a, b = x0[m0:m1], x1[idx // rep1]
        if sub is not None:
            a, b = a - sub[m0:m1, 0, None, None], b - sub[m0:m1, 1, None, None]
        z = torch.stack([a, b], 1)
        y = F.conv2d(z, w64, b64, padding=1)
        T = F.conv2d(z.abs(), w64.abs(), b64.abs(), padding=1)
        y, T = _prelu(y, T, slope)
        got = hi[m0:m1].view(torch.bfloat16).double()
        if lo is not None:
            got = got + lo[m0:m1].view(torch.bfloat16).double()
        r = _assert_close(f"stem {mode} {shape} M={M} slope={slope} images {m0}..", kind, _nchw(got), y, T)
        worst = max(worst, r)
    print(f"stem {mode} {shape}: worst error / bound {worst:.3e}")


# ----------------------------------------------------------------------------------------------------------- the decoder
# (N, H, W): N H W not a multiple of 256 (blocks straddle images) except the whole-tile 16 x 64
DEC_SHAPES = {"1x1": (1, 1, 1), "2x3": (2, 2, 3), "9x27": (3, 9, 27), "17x50": (2, 17, 50), "16x64": (2, 16, 64), "straddle": (5, 7, 33)}


@pytest.mark.parametrize("scale", [2, 3, 4])
@pytest.mark.parametrize("mode", ["bf16", "bf16x3"])
@pytest.mark.parametrize("shape", list(DEC_SHAPES))
def test_decoder(shape, mode, scale):
    """decoder_kernel<BF16, false, S> and the split decoder <F32, true, S>: deconv S x S stride S + PReLU + 1 x 1 conv to one channel"""
    lib = _lib()
    N, H, W = DEC_SHAPES[shape]
    dt = BF16 if mode == "bf16" else BF16X3
    g = torch.Generator().manual_seed(1000 + 10 * scale + N)
    fused = Act((N, H, W, 64), dt, 5 + scale)
    wd = torch.randn((64, 64, scale, scale), generator=g) * 0.05
    if dt == BF16:
        wd = wd.to(torch.bfloat16).float()
    bd = torch.randn(64, generator=g) * 0.1
    wf = torch.randn(64, generator=g) * 0.2
    bf = torch.randn(1, generator=g) * 0.1
    slope = [0.25, BF(-0.3), 1.5, 0.0][(scale + list(DEC_SHAPES).index(shape)) % 4]
    wpk = torch.empty(64 * 64 * scale * scale, dtype=torch.float32, device="cuda")
    sr = torch.full((N + 1, scale * H, scale * W), float("nan"), device="cuda")        # image N: a guard that must stay untouched
    dev = [t.cuda() for t in (wd, bd, wf, bf)] + [_slope_dev(slope)]
    rc = lib.hrn_kt_decoder(dt, scale, fused.ptr, fused.lo_off, _p(dev[0]), _p(wpk), _p(dev[1]), _p(dev[4]), _p(dev[2]), _p(dev[3]), _p(sr),
                            N, H, W, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    got = sr.double().cpu()
    assert bool(torch.isnan(got[N]).all()), "a write past the SR output"
    z = _nchw(fused.val)
    y = F.conv_transpose2d(z, wd.double(), bd.double(), stride=scale)
    T = F.conv_transpose2d(z.abs(), wd.double().abs(), bd.double().abs(), stride=scale)
    y, T = _prelu(y, T, slope)
    want = F.conv2d(y, wf.double().view(1, 64, 1, 1), bf.double())[:, 0]
    T = F.conv2d(T, wf.double().abs().view(1, 64, 1, 1), bf.double().abs())[:, 0]
    _assert_close(f"decoder {mode} S={scale} {shape} slope={slope}", "f32", got[:N], want, T, layout="n y x")
