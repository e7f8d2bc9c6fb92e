"""GPU (-m gpu): the bf16, bf16x3 and fp32 forward kernels, per element, against torch CPU float64.

Each kernel is launched on its own through the hooks of kernel_test.h, bound by tests/kt.py (hrn_kt_conv3x3_epi with the epilogue encoder_impl / fuse_impl set in ConvParams,
hrn_kt_stem, hrn_kt_decoder), with operands chosen so that the kernel's products are exact and only the accumulation order and the
rounding of the stored output remain:
  bf16     activations, weights, bias, slope and alpha bf16-representable;
  bf16x3   activations hi + lo planes of random fp32 values (the view stack, a residual, with 16 significant bits: hi + lo is then exact in
           fp32 and an alpha = 0 slot can be compared bit for bit), weights either bf16-exact (lo = 0: every product exact) or general
           fp32 (the W lo x X hi pass; the dropped lo x lo term is <= 2^-18 of |x w|);
  stem     inputs k / 2^16 (16 significant bits: hi + lo exact), bias of that form, weights bf16 (bf16) or general fp32 (bf16x3).
  fp32     two operand sets (kernel_refs.f32_opset rotates them over the shapes; every lo offset handed to a hook is 0):
           exact   bf16-representable values stored as f32: every product exact, only the accumulation order remains;
           full    activations, view stack, residual, weights, bias, slope and alphas general fp32 with 24 significant bits (slope
                   fp32(0.3), alphas from {0, 1, fp32(0.7)}), the fp64 reference computed from exactly those values: a kernel that
                   loses operand bits (a bf16 staging buffer, a reduced-precision matrix instruction, a dropped lo term) passes
                   `exact` unchanged and fails `full`.  The fp32 stem and decoder run on general fp32 values only.
Bound per element, T = the same expression evaluated on absolute values (sum |terms| of the conv + |bias|, times max(1, |a|) through the
PReLU; with a residual |r| + |alpha| times that; torch_port.ABS_TERMS per element):
  bf16 storage     |got - want| <= 1/2 ulp_bf16(max(|got|, |want|)) + C T     (half an ulp: truncation and double rounding fail)
  bf16x3 (hi + lo) |got - want| <= 2^-16 |want| + C T
  decoder (fp32)   |got - want| <= C T
  fp32 kernels     |got - want| <= C_F32 T      (conv3x3_kernel<F32>, stem_kernel<F32>, decoder_kernel<F32, false, S>)
with one C (kernel_bounds.C) for the whole file and the two that follow it, and C_F32 = 2e-6 <= C (kernel_bounds.C_F32: four times the
largest "C needed" the fp32 cases measured on the MI355X, 4.02e-7).  On the `full` set an operand rounded to bf16 or to 10 mantissa bits
moves the worst element by 186 .. 265 / 24 .. 35 times C_F32 T; one rounded to 16 significant bits (the bf16x3 class) by 4 times in the
stem, but only by 0.7 .. 1.2 times in a convolution: those six controls are listed, not asserted (kernel_refs.F32_CONTROLS_UNASSERTED).
Every test prints its worst error / bound.

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
fp32 (for F32 route 0 and route 1 of the hook reach the same instance, conv3x3_kernel<F32, CI, CO> on 8 x 32 tiles: only route 0 runs)
  conv3x3_kernel<F32,64,64>          encoder_impl: conv 1 / the final conv, PReLU     test_conv[f32enc-*]
  conv3x3_kernel<F32,64,64>          encoder_impl: conv 2 (res_mode 1 in place)       test_conv[f32encres-*]
  conv3x3_kernel<F32,128,128>        fuse_impl convA (pair gather in)                 test_conv[f32pairin-*]
  conv3x3_kernel<F32,128,128>        fuse_impl convB (res_mode 2)                     test_conv[f32pairres-*]
  conv3x3_kernel<F32,128,64>         fuse_impl output conv, res_mode 3 in place with partner alphas / alphas NULL, stack slot and
                                     last level                                      test_conv[f32alpha-*], test_conv[f32alphalast-*]
  conv3x3_kernel<F32,128,64>         fuse_impl output conv, alpha_residual False      test_conv[f32slot-*], test_conv[f32slotlast-*]
  (conv3x3_kernel<F32> with ShiftNet's scale / relu epilogue: tests/test_gpu_kernels_shiftnet.py::test_conv_bn_relu)
  stem_kernel<F32>, sub NULL         encoder_impl, fp32 (rep1 = V)                    test_stem[f32-*]
  stem_kernel<F32>, `sub`            ShiftNet's eval stem (plane means, stride 2 HW)  test_stem[f32sub-*]
  decoder_kernel<F32, false, S>      decoder_impl, fp32                               test_decoder[f32-S*]
Negative controls (test_negative_control; the fp32 ones from kernel_refs.F32_CONTROLS) run on the CPU against the same GPU output and
assert that the comparison FAILS.
"""
import ctypes

import numpy as np
import pytest
import torch

import kernel_refs as K
from kernel_bounds import BF, C, C_F32, GUARD, SENT, SHAPES, Ten, _assert_close, _nchw, _pair_gather, _ratio, _ulp_bf16
from kernel_refs import SLOPES
from kt import BF16, BF16X3, F32, _p, _stream, lib as _lib

pytestmark = pytest.mark.gpu

PAD = 1024                  # gap in front of a lo plane: its offset is never the plane's size (as fuse_impl's t1 / t2)
# SLOPES (kernel_refs): None (no PReLU), ACT 1 (0 <= a <= 1) and ACT 2 (a < 0 or a > 1) of conv3x3_r64, v6's act_pick for a > 1


# ----------------------------------------------------------------------------------------------------------- tensors and bounds
class Act:
    """an activation tensor in storage dt inside a sentinel-filled int16 device buffer: the hi plane [0, n), GUARD sentinels; bf16x3:
    PAD sentinels, the lo plane at lo_off bytes, GUARD sentinels; f32: two words per element, GUARD sentinels, lo_off 0.  val: the exact
    fp64 CPU value (hi + lo).  F32 takes its values from v (fp32, CPU), the other storages draw theirs from seed."""

    def __init__(self, shape, dt, seed=None, scale=1.0, bits16=False, v=None):
        self.shape, self.dt = tuple(shape), dt
        self.n = int(np.prod(shape))
        self.words = self.n * (2 if dt == F32 else 1)           # int16 words of the first (f32: the only) plane
        self.lo_e = self.n + GUARD + PAD if dt == BF16X3 else 0
        total = self.lo_e + self.n + GUARD if dt == BF16X3 else self.words + GUARD
        self.raw = torch.full((total,), SENT, dtype=torch.int16, device="cuda")
        self.lo_off = 2 * self.lo_e
        self.val = None
        if dt == F32:
            assert seed is None
            if v is not None:
                assert v.dtype == torch.float32 and tuple(v.shape) == self.shape
                self.raw[:self.words] = v.contiguous().reshape(-1).view(torch.int16).cuda()
                self.val = v.double()
        elif seed is not None:
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
        """-> (hi, lo or None) as int16 CPU tensors of self.shape (f32: the bit patterns as one int32 tensor, None)"""
        raw = self.raw.cpu()
        if self.dt == F32:
            return raw[:self.words].view(torch.int32).reshape(self.shape), None
        hi = raw[:self.n].reshape(self.shape)
        lo = raw[self.lo_e:self.lo_e + self.n].reshape(self.shape) if self.dt == BF16X3 else None
        return hi, lo

    def value(self):
        hi, lo = self.planes()
        if self.dt == F32:
            return hi.view(torch.float32).double()
        v = hi.view(torch.bfloat16).double()
        return v + lo.view(torch.bfloat16).double() if lo is not None else v

    def guards_intact(self):
        pieces = [self.raw[self.words:self.words + GUARD]]
        if self.dt == BF16X3:
            pieces += [self.raw[self.n + GUARD:self.lo_e], self.raw[self.lo_e + self.n:]]
        return all(bool((p == SENT).all()) for p in pieces)


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
INSTANCES.update(K.F32_INSTANCES)       # f32enc .. f32slotlast: conv3x3_kernel<F32> at its HRNet call sites


def _conv_case(name, shape, seed, slope=None, alphas="mix", wset="bf16", ctrl=None):
    """Launch instance `name` at `shape`; -> dict with the GPU output (fp64), the reference and T, plus what a control needs.
    wset: bf16x3's weight set (bf16 / fp32); for an F32 instance the operand set (exact / full), which also picks slope and alphas"""
    dt, route, cin, cout, res_mode, in_pair, slot = INSTANCES[name]
    lib = _lib()
    H, W = SHAPES[shape]
    # view stack: B samples x V slots; a level of n views (pair_last = n - 2 for odd n) inside it, pair_vs = V > n
    geo = K.conv_geometry(INSTANCES[name], shape)
    uses_stack, n, V, half, pair_last, B, M = (geo[k] for k in ("uses_stack", "n", "V", "half", "pair_last", "B", "M"))
    x3, f32 = dt == BF16X3, dt == F32
    kind = "x3" if x3 else ("f32" if f32 else "bf16")
    opset = wset if f32 else None
    assert (opset in ("exact", "full")) == f32, (name, wset)

    # operands
    if f32:
        ops = K.f32_conv_operands(INSTANCES[name], geo, seed, opset)
        w, bias = ops["w"], ops["bias"]
        slope = K.f32_slope(slope, opset)
    else:
        g = torch.Generator().manual_seed(seed)
        w = torch.randn((cout, cin, 3, 3), generator=g) * (0.05 if cin == 64 else 0.035)
        if not x3 or wset == "bf16":
            w = w.to(torch.bfloat16).float()
        bias = torch.randn(cout, generator=g) * 0.1
        if not x3:
            bias = bias.to(torch.bfloat16).float()
    w64, b64 = w.double(), bias.double()
    wd, bd = w.cuda(), bias.cuda()
    pk = torch.empty(cin * cout * 9 * (2 if x3 or f32 else 1), dtype=torch.bfloat16, device="cuda")
    assert lib.hrn_kt_conv_pack(dt, cin, cout, _p(wd), _p(pk), _stream()) == 0

    def act(key, shp, sd, **kw):          # an operand tensor: F32 from the builder's values, bf16 / bf16x3 drawn from the seed
        return Act(shp, dt, v=ops[key]) if f32 else Act(shp, dt, sd, **kw)

    stack = act("stack", (B, V, H, W, 64), seed + 1, bits16=True) if uses_stack else None
    stack0 = stack.planes() if stack is not None else None
    inp = None if in_pair else act("inp", (M, H, W, cin), seed + 2)
    if in_pair:
        x64 = _pair_gather(stack.val[:, :n], half, pair_last)
    else:
        x64 = inp.val
    # alphas [B][V]: 0, 1, 0.75 (the full set: fp32(0.7)) mixed in the batch (the partner of slot i is pair_last - i)
    alph = None
    if res_mode == 3 and alphas == "mix":
        alph = K.conv_alphas(B, V, opset or "exact")
    out_vs = 1 if slot == "fused" else V
    if slot == "stack":
        out, out_h = stack, half                                  # res_mode 3: in place, out == res == stack
    elif slot == "fused":
        out, out_h = Act((B, H, W, 64), dt), half                 # the last level: fused [B][H][W][64], the residual from the stack
    elif res_mode == 1:
        out, out_h = act("res", (M, H, W, cout), seed + 3), 0     # in place: out == res, as the encoder's second conv
    else:
        out, out_h = Act((M, H, W, cout), dt), 0
    res_ptr, res_lo, res_vs = None, 0, 0
    r64 = None
    if res_mode == 1:
        res_ptr, res_lo = out.ptr, out.lo_off
        r64 = out.val
    elif res_mode == 3:
        res_ptr, res_lo, res_vs = stack.ptr, stack.lo_off, V
    ad = alph.cuda() if alph is not None else None
    sd = _slope_dev(slope)
    pair_h = half if (in_pair or res_mode == 2) else 0
    lo_offs = (0 if in_pair else inp.lo_off, stack.lo_off if stack is not None else 0, out.lo_off, res_lo)
    assert not f32 or lo_offs == (0, 0, 0, 0)
    rc = lib.hrn_kt_conv3x3_epi(dt, route, cin, cout, None if in_pair else inp.ptr, stack.ptr if stack is not None else None, pair_h,
                                pair_last, V if uses_stack else 0, _p(pk), _p(bd), _p(sd), res_ptr, res_mode, res_vs, _p(ad),
                                V if ad is not None else 0, out.ptr, out_h, out_vs if slot else 0, *lo_offs, M, H, W, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()

    # reference (kernel_refs.ref_conv_epi), in fp64 on the exact values the kernel read
    args = dict(x=x64, w=w64, b=b64, slope=slope, res_mode=res_mode, res=r64, stack=stack.val if stack is not None else None, geo=geo,
                alph=alph)

    def reference(w64=w64, own_alpha=False, swap_halves=False):
        return K.ref_conv_epi(**dict(args, w=w64, own_alpha=own_alpha, swap_halves=swap_halves))

    if slot == "stack":
        got = _nchw(out.value()[:, :half].reshape(M, H, W, 64))
    else:
        got = _nchw(out.value())
    want, T = reference()
    return dict(got=got, want=want, T=T, kind=kind, reference=reference, w64=w64, stack=stack, stack0=stack0, half=half, V=V, out=out,
                inp=inp, alph=alph, slot=slot, M=M, res_mode=res_mode, pair_last=pair_last, args=args, c=C_F32 if f32 else None)


# the case matrix: every instance at every shape; the slope class, the alphas (mixed / NULL) and the weight set (bf16x3: bf16-exact or
# general fp32; F32: the operand set exact / full of kernel_refs.f32_opset - every F32 instance meets `full` at 2x3, 15x33, 9x63 and
# multi) rotate over the shapes instead of taking the full product
CASES = []
for ii, name in enumerate(INSTANCES):
    for si, shape in enumerate(SHAPES):
        wset = K.f32_opset(ii, si) if INSTANCES[name][0] == F32 else ("fp32" if (ii + si) % 2 else "bf16")
        CASES.append(pytest.param(name, shape, SLOPES[(ii + si) % len(SLOPES)], "null" if (ii + si) % 4 == 3 else "mix", wset,
                                  id=f"{name}-{shape}"))


@pytest.mark.parametrize("name,shape,slope,alphas,wset", CASES)
def test_conv(name, shape, slope, alphas, wset):
    r = _conv_case(name, shape, 100 + 7 * list(SHAPES).index(shape), slope=slope, alphas=alphas, wset=wset)
    shown = K.f32_slope(slope, wset) if INSTANCES[name][0] == F32 else slope       # (the full set runs its own value of the slope's class)
    tag = f"{name} {shape} slope={shown} alphas={alphas} w={wset}"
    _assert_close(tag, r["kind"], r["got"], r["want"], r["T"], c=r["c"] or C)
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


def _f32_control_case(target):
    """the GPU output a fp32 control is judged on: target an F32 conv instance, "stem" or "decoder", at the case kernel_refs names"""
    if target == "stem":
        r = _stem_case("f32", K.F32_CONTROL_SHAPE)
        return dict(kind="stem", got=_nchw(r["out"].value()), args=dict(r["args"], m0=0, m1=r["M"]), layout="m c y x")
    if target == "decoder":
        r = _decoder_case(K.F32_CONTROL_DECODER[0], "f32", K.F32_CONTROL_DECODER[1])
        return dict(kind="decoder", got=r["got"], args=r["args"], layout="n y x")
    r = _conv_case(target, K.F32_CONTROL_SHAPE, K.F32_CONTROL_SEED, slope=K.F32_CONTROL_SLOPE, alphas="mix", wset="full")
    return dict(kind="conv", got=r["got"], args=r["args"], layout="m c y x")


@pytest.mark.parametrize("control,name", [("tap_swap", "v6pairres"), ("tap_swap", "x3alpha"), ("tap_swap", "r64res"),
                                          ("round_to_zero", "r64"), ("round_to_zero", "v6alpha"),
                                          ("own_alpha", "v6alpha"), ("own_alpha", "x3alpha"), ("own_alpha", "genalpha"),
                                          ("swap_halves", "v6pairres"), ("swap_halves", "x3pairres"), ("swap_halves", "genpairres")] +
                         K.F32_CONTROLS)
def test_negative_control(control, name):
    """The comparison against a reference that is wrong in one way must FAIL on the same GPU output that passes against the right one:
    one (co, ci) pair with two taps swapped; the reference rounded toward zero (bf16); the view's own alpha instead of its partner's
    (res_mode 3); the pair residual with its 64-channel halves swapped (res_mode 2).
    fp32 (kernel_refs.F32_CONTROLS: the f32* instances, "stem", "decoder"), all on the `full` operand set under C_F32: the structural
    controls above plus swap_in (the pair-gather input's halves exchanged: the chunk -> src0 / src1 selection), and the operand-rounding
    controls round<bits>_x / round<bits>_w - the reference computed from activations (stem: inputs; decoder: `fused`) or weights rounded
    to 8 (bf16), 11 (10 mantissa bits) or 16 significant bits (the bf16x3 class: what stem_mfma_kernel keeps of an input).  On the
    `exact` operand set the rounding controls are no-ops - rounding a bf16-representable value changes nothing, so a kernel that drops
    operand bits passes there: the gap the `full` set closes.  tests/test_kernels_fwd_f32_host.py asserts on the CPU that each of these
    wrong references is at least twice the bound from the right one, which the kernel's own error (at most once the bound) cannot hide."""
    if (control, name) in K.F32_CONTROLS:
        case = _f32_control_case(name)
        got = case["got"]
        want, T = K.f32_control_reference(None, case)
        ok = _assert_close(f"{name} (right reference)", "f32", got, want, T, layout=case["layout"], c=C_F32)
        bad, Tb = K.f32_control_reference(control, case)
        worst, idx = _ratio("f32", got, bad, Tb, C_F32)
        print(f"{control} {name}: error / bound against the wrong reference {worst:.3e} (right one {ok:.3e})")
        assert worst > 1.0, f"{control} {name}: the comparison does not tell the wrong reference from the right one"
        return
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


def _stem_case(mode, shape):
    """Launch the stem in `mode` at `shape` -> dict: the output tensor, the fp64 operands (args of kernel_refs.ref_stem_fwd), kind, c"""
    lib = _lib()
    H, W, M = STEM_SHAPES[shape]
    segs_x = -(-W // 32)
    if M is None:       # every wave walks two segments at least: nseg >= 2 x 32,768 and all three carries of advance() occur
        M = -(-2 * 32768 // (H * segs_x)) + 1
        nseg = M * H * segs_x
        waves = 4 * min(-(-nseg // 4), 8192)
        assert nseg >= 2 * waves and segs_x % 2 == 1 and (waves // segs_x) % H != 0, (nseg, waves)
        # (the VALU stem_kernel of bf16sub / f32 / f32sub: more 4 x 32 patches than its 16,384 blocks, so blocks walk a second patch)
        assert M * -(-H // 4) * segs_x > 16384
    slope = [None, 0.25, BF(-0.3), 1.5][list(STEM_SHAPES).index(shape) % 4]
    if mode in ("f32", "f32sub"):
        # general fp32 inputs, weights and bias (kernel_refs.f32_stem_operands); the inputs sit in guarded buffers that must stay unchanged
        dt, kind, c = F32, "f32", C_F32
        slope = K.f32_slope(slope, "full")
        ops = K.f32_stem_operands(mode, M, H, W, 17 + M + H)
        rep1, sub, w, bias = ops["rep1"], ops["sub"], ops["w"], ops["bias"]
        x0, x1 = ops["x0"].double(), ops["x1"].double()
        if mode == "f32sub":        # as ShiftNet's eval pass: one tensor [M][2][H][W], in1 = in0 + plane, both 2 planes apart, rep1 = 1
            held = [Ten(ops["x"].shape, F32, ops["x"])]
            p0, p1, stride = held[0].ptr, ctypes.c_void_p(held[0].raw.data_ptr() + 4 * H * W), 2 * H * W
        else:
            held = [Ten(ops["x0"].shape, F32, ops["x0"]), Ten(ops["x1"].shape, F32, ops["x1"])]
            p0, p1, stride = held[0].ptr, held[1].ptr, H * W
        held += [Ten(w.shape, F32, w), Ten(bias.shape, F32, bias)] + ([Ten(sub.shape, F32, sub)] if sub is not None else [])
        dw, db, dsub = held[2 if mode == "f32" else 1].ptr, held[3 if mode == "f32" else 2].ptr, held[-1].ptr if sub is not None else None
        sub = sub.double() if sub is not None else None
    else:
        rep1, held, c = 3, [], C
        dt = BF16 if mode != "bf16x3" else BF16X3
        kind = "x3" if dt == BF16X3 else "bf16"
        g = torch.Generator().manual_seed(17 + M + H)
        x0 = _k16((M, H, W), g)
        x1 = _k16((-(-M // rep1), H, W), g)
        w = torch.randn((64, 2, 3, 3), generator=g) * 0.3
        if mode == "bf16":
            w = w.to(torch.bfloat16).float()        # (bf16x3 and the VALU stem take general fp32 weights)
        bias = (torch.randint(-(1 << 14), 1 << 14, (64,), generator=g).double() / 65536.0).float()
        sub = _k16((M, 2), g) if mode == "bf16sub" else None
        keep = [x0.float().cuda(), x1.float().cuda(), w.cuda(), bias.cuda(), sub.float().cuda() if sub is not None else None]
        p0, p1, dw, db, dsub = (_p(t) for t in keep)
        stride = H * W
    out = Act((M, H, W, 64), dt)
    ds = _slope_dev(slope)
    rc = lib.hrn_kt_stem(dt, p0, stride, p1, rep1, stride, dsub, dw, db, _p(ds), out.ptr, out.lo_off, M, H, W, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert out.guards_intact()
    assert all(t.unchanged() for t in held), "the stem wrote one of its inputs"
    return dict(out=out, M=M, kind=kind, c=c, slope=slope,
                args=dict(x0=x0, x1=x1, rep1=rep1, sub=sub, w=w.double(), b=bias.double(), slope=slope))


@pytest.mark.parametrize("mode", ["bf16", "bf16x3", "bf16sub", "f32", "f32sub"])
@pytest.mark.parametrize("shape", list(STEM_SHAPES))
def test_stem(mode, shape):
    """stem_mfma_kernel<false> (bf16), <true> (bf16x3) and the VALU stem_kernel<BF16> (`sub`): 2 -> 64 conv + PReLU of (view m, frame m / rep1);
    stem_kernel<F32> as encoder_impl calls it (f32: sub NULL, rep1 = V) and as ShiftNet's eval pass does (f32sub: in1 = in0 + plane, image
    stride 2 planes, rep1 = 1, sub = the plane means), on general fp32 inputs and weights"""
    r = _stem_case(mode, shape)
    M, kind, slope = r["M"], r["kind"], r["slope"]
    hi, lo = r["out"].planes()
    worst = 0.0
    step = 512
    for m0 in range(0, M, step):          # in chunks of images: host memory stays small at the multi-item shape
        m1 = min(M, m0 + step)
        y, T = K.ref_stem_fwd(m0=m0, m1=m1, **r["args"])
        if kind == "f32":
            got = hi[m0:m1].view(torch.float32).double()
        else:
            got = hi[m0:m1].view(torch.bfloat16).double()
        if lo is not None:
            got = got + lo[m0:m1].view(torch.bfloat16).double()
        e = _assert_close(f"stem {mode} {shape} M={M} slope={slope} images {m0}..", kind, _nchw(got), y, T, c=r["c"])
        worst = max(worst, e)
    print(f"stem {mode} {shape}: worst error / bound {worst:.3e}")


# ----------------------------------------------------------------------------------------------------------- the decoder
# (N, H, W): N H W not a multiple of 256 (blocks straddle images) except the whole-tile 16 x 64
DEC_SHAPES = {"1x1": (1, 1, 1), "2x3": (2, 2, 3), "9x27": (3, 9, 27), "17x50": (2, 17, 50), "16x64": (2, 16, 64), "straddle": (5, 7, 33)}


def _decoder_case(shape, mode, scale):
    """Launch the decoder -> dict: sr (fp64, N images; the guard image checked), the fp64 args of kernel_refs.ref_decoder_fwd, c"""
    lib = _lib()
    N, H, W = DEC_SHAPES[shape]
    dt = {"bf16": BF16, "bf16x3": BF16X3, "f32": F32}[mode]
    slope = [0.25, BF(-0.3), 1.5, 0.0][(scale + list(DEC_SHAPES).index(shape)) % 4]
    if dt == F32:       # `fused` stored as f32, general fp32 values like the weights (kernel_refs.f32_decoder_operands)
        slope = K.f32_slope(slope, "full")
        ops = K.f32_decoder_operands(N, H, W, scale, 1000 + 10 * scale + N)
        fused = Act((N, H, W, 64), dt, v=ops["fused"])
        wd, bd, wf, bf = (ops[k] for k in ("wd", "bd", "wf", "bf"))
    else:
        g = torch.Generator().manual_seed(1000 + 10 * scale + N)
        fused = Act((N, H, W, 64), dt, 5 + scale)
        wd = torch.randn((64, 64, scale, scale), generator=g) * 0.05
        if dt == BF16:
            wd = wd.to(torch.bfloat16).float()
        bd = torch.randn(64, generator=g) * 0.1
        wf = torch.randn(64, generator=g) * 0.2
        bf = torch.randn(1, generator=g) * 0.1
    wpk = torch.empty(64 * 64 * scale * scale, dtype=torch.float32, device="cuda")
    sr = torch.full((N + 1, scale * H, scale * W), float("nan"), device="cuda")        # image N: a guard that must stay untouched
    dev = [t.cuda() for t in (wd, bd, wf, bf)] + [_slope_dev(slope)]
    rc = lib.hrn_kt_decoder(dt, scale, fused.ptr, fused.lo_off, _p(dev[0]), _p(wpk), _p(dev[1]), _p(dev[4]), _p(dev[2]), _p(dev[3]), _p(sr),
                            N, H, W, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    got = sr.double().cpu()
    assert bool(torch.isnan(got[N]).all()), "a write past the SR output"
    assert fused.guards_intact() and torch.equal(fused.value(), fused.val), "the decoder wrote its input"
    return dict(got=got[:N], slope=slope, c=C_F32 if dt == F32 else C,
                args=dict(fused=fused.val, wd=wd.double(), bd=bd.double(), slope=slope, wf=wf.double(), bf=bf.double(), S=scale))


@pytest.mark.parametrize("scale", [2, 3, 4])
@pytest.mark.parametrize("mode", ["bf16", "bf16x3", "f32"])
@pytest.mark.parametrize("shape", list(DEC_SHAPES))
def test_decoder(shape, mode, scale):
    """decoder_kernel<BF16, false, S>, the split decoder <F32, true, S> and the fp32 decoder <F32, false, S> (`fused` stored as f32, general
    fp32 values): deconv S x S stride S + PReLU + 1 x 1 conv to one channel"""
    r = _decoder_case(shape, mode, scale)
    want, T = K.ref_decoder_fwd(**r["args"])
    _assert_close(f"decoder {mode} S={scale} {shape} slope={r['slope']}", "f32", r["got"], want, T, layout="n y x", c=r["c"])
