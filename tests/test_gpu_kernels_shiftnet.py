"""GPU (-m gpu): ShiftNet's own kernels (shiftnet.hip, shiftnet_bwd.hip, the per-plane mean of stem.hip, the f32 convolution's folded
BatchNorm epilogue) and the fused Adam, per element, against torch CPU float64.

Each launcher is called on its own through the hooks of kernel_test.h (hrn_kt_sn_*, bound by tests/kt.py), exactly as api.hip / shiftnet_bwd.hip call it, on the stored
tensors it would see in production; Adam through the public hrn_adam_step.  The reference (the ref_* functions of tests/kernel_refs.py, checked against
torch autograd / torch.optim.Adam by tests/test_kernels_shiftnet_host.py) is the same operation in fp64 on the exact values the kernel
reads.  A kernel fed its stored tensors has no ReLU / max-pool flip to excuse: where a gate depends on computed values the inputs make
them exact (quantised x with a power-of-two scale and a coarse shift), and one test holds the forward's and the backward's gate to each
other with general values.  Operands are chosen so that the products a kernel forms in fp32 are exact (bf16-representable values, or 16
significant bits against 8): only the accumulation order and one rounding of the stored output remain.
Bound per element, T = the same expression on absolute values, C = kernel_bounds.C = 1e-5:
  bf16 output                          |got - want| <= 1/2 ulp_bf16(max(|got|, |want|)) + c T
  f32 output, every parameter gradient |got - want| <= c T       (accumulated gradients: want = start + sum, T = |start| + sum |terms|)
c = C, except where an fp32 chain is longer than 128 terms by construction: c = max(C, n_seq 2^-24), n_seq computed from the kernel's
constants and printed (stem_dgrad 9 x 64; fc1 16 stages x 64 k + 32 slabs + 1; fc1_bwd_x 256 + 3).  No element is masked or excluded.
Outputs start as sentinels, accumulated gradients from random values with NaN behind; every test asserts that its inputs are
bit-identical afterwards and that the guards behind every output are intact, and prints its worst error / bound.
Bit for bit: bn_act_pool with an exact affine, sub_plane_mean, fc_to_ref, fc_from_ref (bf16: one round to nearest even).

Template instance -> production call site -> tests
  bn_partial_kernel<F32|BF16> + bn_finish_kernel        BatchNorm statistics, training forward (both), train-mode forward of api.hip (f32)
                                                                                                 test_bn_stats[f32|bf16-C*-*]
  bn_save_stats_kernel                                  mean / invstd kept for the backward      test_bn_stats[*]
  bn_fold_kernel                                        eval mode (api.hip), with / without conv_bias   test_bn_fold[C*-*]
  bn_act_pool_kernel<1|2, F32|BF16>                     BN + ReLU (+ pool) of every layer; scale NULL: eval's pool-only pass
                                                        test_bn_act_pool[f32|bf16-pool*-C*-exact|general|null], test_bn_act_pool_grid_stride[*]
  bn_bwd_reduce / apply_kernel<1|2, F32|BF16> + bn_bwd_finish_kernel
                                                        the BatchNorm backward of every layer    test_bn_bwd[f32|bf16-pool*-C*], test_bn_bwd_grid_cap[*]
  (forward / backward gate)                             bn_act_pool and bn_dv on the same tensors test_bn_gate_agreement[f32|bf16-pool*]
  conv3x3_kernel<F32, 64|128, 64|128> (scale, relu)     eval mode: conv + folded BN + ReLU        test_conv_bn_relu[*-*]
  plane_mean_kernel                                     the input's plane means, forward and backward   test_plane_mean[hw*]
  sub_plane_mean_kernel                                 d_x = g - mean(g)                         test_sub_plane_mean[hw*|cap]
  stem_dgrad_kernel<F32|BF16>                           the stem's input gradient                test_stem_dgrad[f32|bf16-*]
  fc_to_ref_kernel<F32|BF16>                            fc1's input, dropout folded in            test_fc_to_ref[f32|bf16-B*-*]
  fc_from_ref_kernel<F32|BF16>                          its gradient back to NHWC                 test_fc_from_ref[f32|bf16-B*-*]
  fc1_mfma_kernel + fc1_finish_kernel                   fc1 + ReLU, groups of 32 samples          test_fc1[B*], test_fc_to_ref_fc1_chain
  fc2_kernel                                            fc2                                       test_fc2[B*]
  fc2_bwd_kernel                                        dz1, d fc2.weight, d fc1.bias             test_fc2_bwd[*-B*]
  fc1_bwd_w_kernel                                      d fc1.weight                              test_fc1_bwd_w[B*]
  fc1_bwd_x_kernel                                      d fc1 input                               test_fc1_bwd_x[B*]
  adam_kernel (adam.hip)                                hrn_adam_step, FusedAdam.step             test_adam[n*-s*]
Negative controls (test_negative_control) run on the CPU against the GPU output that passed and assert that the comparison FAILS.
"""
import functools

import numpy as np
import pytest
import torch

from kernel_bounds import NAN16, SENT, SHAPES, Acc, C, Ten, _assert_close, _exact_affine, _grid, _nchw, _quantised, _ratio, _tiles, rnd
from kernel_refs import (ADAM_EPS, ADAM_SETTINGS, BN_NPIX, D, FC1_NSEQ, FCK, FCX_NSEQ, HIGH, MOM, _adam_p_ratio, _mask, _stem_dgrad_w,
                         _window_counts, adam_inputs, bn_stats_inputs, ref_adam, ref_bn_act_pool, ref_bn_bwd, ref_bn_fold, ref_bn_stats,
                         ref_conv_bn_relu, ref_fc1, ref_fc1_bwd_w, ref_fc1_bwd_x, ref_fc2, ref_fc2_bwd, ref_fc_from_ref, ref_fc_to_ref,
                         ref_stem_dgrad)
from kt import BF16, F32, _p, _stream, lib as _lib

pytestmark = pytest.mark.gpu

DTS = [pytest.param(F32, id="f32"), pytest.param(BF16, id="bf16")]
KIND = {F32: "f32", BF16: "bf16"}


# ----------------------------------------------------------------------------------------------------------- helpers
class NanTen(Ten):
    """a Ten with NaN instead of the finite sentinel behind the payload: a read past the tensor poisons what is computed from it"""

    def __init__(self, shape, dt, v=None, fill=SENT):
        super().__init__(shape, dt, v, fill)
        self.bits0 = self.bits0.clone()
        self.bits0[self.words:] = NAN16
        self.raw = self.bits0.cuda()

    def guard_ok(self):
        return bool((self.raw[self.words:] == NAN16).all())


def V(v, cls=Ten):
    """an f32 device tensor (with guards) of the fp32 CPU values v"""
    return cls(tuple(v.shape), F32, v.float())


def _close(tag, kind, got, want, T, c=C, layout="i"):
    return _assert_close(tag, kind, got, want, T * (c / C), layout=layout)


def _assert_bound(tag, got, want, bound, layout="i"):
    """|got - want| <= bound per element, with the worst error / bound printed"""
    r = (got - want).abs() / (bound + 1e-300)
    i = int(torch.argmax(r))
    idx = np.unravel_index(i, tuple(r.shape))
    worst = float(r.reshape(-1)[i])
    print(f"{tag}: max error / bound {worst:.3e} at ({layout}) = {tuple(int(k) for k in idx)}")
    assert worst <= 1.0, f"{tag}: element {idx}: got {float(got[idx]):.9g}, want {float(want[idx]):.9g}, bound {float(bound[idx]):.3g}"
    return worst


def _bits_equal(tag, got, want):
    """bit for bit up to the sign of a zero"""
    bad = int((got != want).sum()) if got.dtype == want.dtype else -1
    print(f"{tag}: {bad} of {got.numel()} elements differ")
    assert bad == 0, tag
    return float(bad)


def _seq_const(tag, n_seq):
    c = C if n_seq <= 128 else max(C, n_seq * 2.0 ** -24)
    print(f"{tag}: n_seq = {n_seq}, constant = {c:.3e}")
    return c


def _stored(v, dt):
    """fp64 exact value -> what a store in dt keeps of it (f32: the value must be representable; bf16: one round to nearest even)"""
    f = v.float()
    assert torch.equal(f.double(), v), "not representable in fp32"
    return f if dt == F32 else f.to(torch.bfloat16)


def _payload(t):
    """the payload of a Ten as a typed CPU tensor (f32 or bf16)"""
    return t.planes()[0]


# ----------------------------------------------------------------------------------------------------------- BatchNorm statistics, fold
def _bn_stats_case(dt, Cc, npix, running=True):
    lib = _lib()
    xv, gamma, beta, rm0, rv0 = bn_stats_inputs(npix, Cc, dt, 7 + Cc + npix % 1000)
    x, ga, be = Ten((npix, Cc), dt, xv), V(gamma), V(beta)
    rm, rv = (V(rm0), V(rv0)) if running else (None, None)
    outs = {k: Ten((Cc,), F32) for k in ("scale", "shift", "mean", "invstd")}
    npart = 256 * 128 * 2
    part = torch.full((npart + 64,), float("nan"), dtype=D, device="cuda")
    assert lib.hrn_kt_sn_bn_stats(dt, x.ptr, npix, Cc, ga.ptr, be.ptr, outs["scale"].ptr, outs["shift"].ptr, rm.ptr if running else None,
                                  rv.ptr if running else None, MOM, _p(part), _stream()) == 0
    assert lib.hrn_kt_sn_bn_save_stats(_p(part), npix, Cc, outs["mean"].ptr, outs["invstd"].ptr, _stream()) == 0
    torch.cuda.synchronize()
    assert x.unchanged() and ga.unchanged() and be.unchanged(), "an input was written"
    assert all(t.guard_ok() for t in outs.values()) and bool(torch.isnan(part[npart:]).all()), "a write past an output"
    got = {k: t.value() for k, t in outs.items()}
    if running:
        assert rm.guard_ok() and rv.guard_ok()
        got["running_mean"], got["running_var"] = rm.value(), rv.value()
    return dict(got=got, x=x.val, gamma=ga.val, beta=be.val, rm0=rm0.double() if running else None, rv0=rv0.double() if running else None)


BN_STATS_CASES = []
for _di, _dt in enumerate((F32, BF16)):
    for _ci, _Cc in enumerate((64, 128)):
        for _ni, _nn in enumerate(BN_NPIX):
            BN_STATS_CASES.append(pytest.param(_dt, _Cc, _nn, (_di + _ci + _ni) % 4 != 3, id=f"{KIND[_dt]}-C{_Cc}-{_nn}"))


@pytest.mark.parametrize("dt,Cc,npix_name,running", BN_STATS_CASES)
def test_bn_stats(dt, Cc, npix_name, running):
    """bn_partial_kernel<ST> + bn_finish_kernel, then bn_save_stats_kernel on the same partial sums: six vectors per channel (running_*
    NULL in a quarter of the cases).  npix 257: blocks 129.. of the 256 get no pixel; 255 x 256 + 1: one pixel in the last block"""
    npix = BN_NPIX[npix_name]
    r = _bn_stats_case(dt, Cc, npix, running)
    x = r["x"]
    mean, var = x.mean(0), x.var(0, unbiased=False)
    ratio = float((mean[3:5] ** 2 / var[3:5]).max())
    print(f"bn_stats: mean^2 / var up to {ratio:.3e}; variance of the constant channels {[float(v) for v in var[5:8]]}")
    assert ratio >= HIGH[dt] and float(var[5:8].max()) <= 1e-30
    assert all(bool((x[:, 5 + k] == x[0, 5 + k]).all()) for k in range(3)) and float(x[0, 5]) == 0.0
    want = ref_bn_stats(x, r["gamma"], r["beta"], r["rm0"], r["rv0"])
    assert set(want) == set(r["got"])
    for k, (w, T) in want.items():
        _close(f"bn_stats {KIND[dt]} C={Cc} npix={npix} {k}", "f32", r["got"][k], w, T, layout="c")


@pytest.mark.parametrize("bias", [True, False], ids=["convbias", "nobias"])
@pytest.mark.parametrize("Cc", [64, 128], ids=["C64", "C128"])
def test_bn_fold(Cc, bias):
    """bn_fold_kernel: scale = gamma / sqrt(running_var + eps), shift = beta + (conv_bias - running_mean) scale"""
    lib = _lib()
    g = torch.Generator().manual_seed(Cc)
    vals = [torch.randn(Cc, generator=g), torch.randn(Cc, generator=g) * 0.1, torch.randn(Cc, generator=g), torch.rand(Cc, generator=g) * 2 + 1e-3,
            torch.randn(Cc, generator=g)]
    vals[3][:3] = torch.tensor([0.0, 1e-7, 1e4])                   # running_var: zero, far below eps, large
    ins = [V(v) for v in vals]
    sc, sh = Ten((Cc,), F32), Ten((Cc,), F32)
    assert lib.hrn_kt_sn_bn_fold(ins[0].ptr, ins[1].ptr, ins[2].ptr, ins[3].ptr, ins[4].ptr if bias else None, sc.ptr, sh.ptr, Cc, _stream()) == 0
    torch.cuda.synchronize()
    assert all(t.unchanged() for t in ins) and sc.guard_ok() and sh.guard_ok()
    (wsc, Tsc), (wsh, Tsh) = ref_bn_fold(*[t.val for t in ins[:4]], ins[4].val if bias else None)
    _close(f"bn_fold C={Cc} bias={bias} scale", "f32", sc.value(), wsc, Tsc, layout="c")
    _close(f"bn_fold C={Cc} bias={bias} shift", "f32", sh.value(), wsh, Tsh, layout="c")


# ----------------------------------------------------------------------------------------------------------- BN + ReLU (+ pool), forward
def general_affine(Cc, seed):
    """scale of both signs in 0.5 .. 1.5, shift ~ 0.3 N(0, 1): general fp32 values"""
    g = torch.Generator().manual_seed(seed)
    sc = torch.rand(Cc, generator=g) + 0.5
    sc[2::5] *= -1
    return sc, torch.randn(Cc, generator=g) * 0.3


def _act_pool_case(dt, pool, N, H, Cc, mode, seed):
    """mode "exact": quantised x, power-of-two scale, coarse shift (x scale + shift exact in fp32: the output is the fp64 result, stored);
    "general": random x, scale, shift; "null": scale = shift = NULL, the pool (+ ReLU) only pass of eval mode"""
    lib = _lib()
    p = 2 if pool else 1
    if mode == "general":
        xv, (sc, sh) = rnd((N, H, H, Cc), seed, dt), general_affine(Cc, seed + 1)
    else:
        xv, (sc, sh) = _quantised((N, H, H, Cc), seed).float(), _exact_affine(Cc, seed + 1)
    x = Ten((N, H, H, Cc), dt, xv)
    assert torch.equal(x.val, xv.double())
    scd, shd = (None, None) if mode == "null" else (V(sc), V(sh))
    out = Ten((N, H // p, H // p, Cc), dt)
    assert lib.hrn_kt_sn_bn_act_pool(dt, x.ptr, scd.ptr if scd else None, shd.ptr if shd else None, out.ptr, N, H, H, Cc, pool, _stream()) == 0
    torch.cuda.synchronize()
    assert x.unchanged() and out.guard_ok() and (mode == "null" or (scd.unchanged() and shd.unchanged()))
    return dict(x=x, out=out, sc=None if mode == "null" else sc.double(), sh=None if mode == "null" else sh.double())


def _act_pool_check(tag, dt, pool, mode, r):
    want, T = ref_bn_act_pool(r["x"].val, r["sc"], r["sh"], pool)
    if mode == "general":
        return _close(tag, KIND[dt], r["out"].value(), want, T, layout="n y x c")
    if pool:
        tied, dead = _window_counts(ref_bn_act_pool(r["x"].val, r["sc"], r["sh"], 0)[0])
        print(f"{tag}: {tied} tied windows, {dead} windows all <= 0")
        assert tied > 100 and dead > 100
    assert bool((want == 0).any()) and bool((want > 0).any())
    return _bits_equal(tag, _payload(r["out"]), _stored(want, dt))


@pytest.mark.parametrize("mode", ["exact", "general", "null"])
@pytest.mark.parametrize("Cc,H", [(64, 32), (128, 16)], ids=["C64", "C128"])
@pytest.mark.parametrize("pool", [0, 1], ids=["pool0", "pool1"])
@pytest.mark.parametrize("dt", DTS)
def test_bn_act_pool(dt, pool, Cc, H, mode):
    """bn_act_pool_kernel<POOL, ST>: bit for bit with an exact affine and in the pool-only pass, the bound with a general one"""
    r = _act_pool_case(dt, pool, 3, H, Cc, mode, 7 + Cc + pool)
    _act_pool_check(f"bn_act_pool {KIND[dt]} pool={pool} C={Cc} {mode}", dt, pool, mode, r)


@pytest.mark.parametrize("dt", DTS)
def test_bn_act_pool_grid_stride(dt):
    """N Ho Wo C / 4 above the grid of 8192 x 256 threads, as at layer 1 of every production batch: the grid-stride loop runs twice"""
    N, H, Cc = 9, 128, 64
    assert N * H * H * Cc // 4 > 8192 * 256
    r = _act_pool_case(dt, 0, N, H, Cc, "exact", 5)
    _act_pool_check(f"bn_act_pool {KIND[dt]} grid-stride", dt, 0, "exact", r)


# ----------------------------------------------------------------------------------------------------------- BN + ReLU (+ pool), backward
def _bn_bwd_case(dt, pool, N, H, Cc, null=None, general=False, seed=11, dbeta_zero=False, x_ten=None):
    """stats hand-made: mean, invstd general, scale / shift exact (general=True: general too, with random x)"""
    lib = _lib()
    p = 2 if pool else 1
    g = torch.Generator().manual_seed(seed + 2)
    if general:
        xv, (sc, sh) = rnd((N, H, H, Cc), seed, dt), general_affine(Cc, seed + 1)
    else:
        xv, (sc, sh) = _quantised((N, H, H, Cc), seed).float(), _exact_affine(Cc, seed + 1)
    x = x_ten if x_ten is not None else Ten((N, H, H, Cc), dt, xv)
    dy = Ten((N, H // p, H // p, Cc), dt, rnd((N, H // p, H // p, Cc), seed + 3, dt))
    mean, istd = torch.randn(Cc, generator=g) * 0.05, torch.rand(Cc, generator=g) + 0.5
    gamma = torch.rand(Cc, generator=g) + 0.5
    gamma[::3] *= -1
    sv = torch.zeros(512)
    sv[:Cc], sv[128:128 + Cc], sv[256:256 + Cc], sv[384:384 + Cc] = mean, istd, sc, sh
    stats, ga = V(sv), V(gamma)
    dx = Ten((N, H, H, Cc), dt)
    dg, db = Acc((Cc,), seed + 4, none=null == "dgamma"), Acc((Cc,), seed + 5, none=null == "dbeta")
    if dbeta_zero:
        db.start = torch.zeros(Cc)
        db.buf = torch.cat([db.start, torch.full((64,), float("nan"))]).cuda()
    part = torch.full((256 * 128 * 2 + 64,), float("nan"), dtype=D, device="cuda")
    sums = torch.full((256 + 64,), float("nan"), dtype=D, device="cuda")
    assert lib.hrn_kt_sn_bn_bwd(dt, x.ptr, dy.ptr, stats.ptr, ga.ptr, dx.ptr, dg.ptr, db.ptr, N, H, H, Cc, pool, _p(part), _p(sums), _stream()) == 0
    torch.cuda.synchronize()
    assert x.unchanged() and dy.unchanged() and stats.unchanged() and ga.unchanged(), "an input was written"
    assert dx.guard_ok() and bool(torch.isnan(part[256 * 128 * 2:]).all()) and bool(torch.isnan(sums[256:]).all()), "a write past an output"
    args = [x.val, dy.val] + [t.double() for t in (mean, istd, sc, sh, gamma)] + [pool]
    return dict(dx=dx.value(), dg=dg, db=db, args=args, x=x, dy=dy, sc=sc, sh=sh, kind=KIND[dt])


def _bn_bwd_check(tag, r):
    ref = ref_bn_bwd(*r["args"])
    x, _, _, _, sc, sh, _, pool = r["args"]
    v = torch.relu(x * sc + sh)
    if pool:
        tied, dead = _window_counts(v)
        print(f"{tag}: {tied} tied windows, {dead} windows all <= 0")
        assert tied > 100 and dead > 100
    assert bool((v == 0).any()) and bool((v > 0).any())
    _close(tag + " dx", r["kind"], r["dx"], *ref["dx"], layout="n y x c")
    r["db"].check(tag + " dbeta", *ref["dbeta"], layout="c")
    r["dg"].check(tag + " dgamma", *ref["dgamma"], layout="c")


BN_BWD_CASES = []
for _di, _dt in enumerate((F32, BF16)):
    for _pool in (0, 1):
        for _ci, (_Cc, _H) in enumerate(((64, 32), (128, 16))):
            for _ni, _null in enumerate((None, "dgamma", "dbeta")):
                BN_BWD_CASES.append(pytest.param(_dt, _pool, _Cc, _H, _null, id=f"{KIND[_dt]}-pool{_pool}-C{_Cc}-{_null or 'all'}"))


@pytest.mark.parametrize("dt,pool,Cc,H,null", BN_BWD_CASES)
def test_bn_bwd(dt, pool, Cc, H, null):
    """bn_bwd_reduce / finish / apply: dx per element, dgamma / dbeta accumulated (each NULL in turn).  Exact affine: the ReLU / arg-max gate
    is the fp64 one; ties go to the first maximum, windows that are all <= 0 get nothing"""
    _bn_bwd_check(f"bn_bwd {KIND[dt]} pool={pool} C={Cc} null={null}", _bn_bwd_case(dt, pool, 3, H, Cc, null, seed=11 + Cc + pool))


@pytest.mark.parametrize("dt", DTS)
def test_bn_bwd_grid_cap(dt):
    """N H W C / 4 above ew_grid's cap of 4096 x 256 threads (N H W > 65,536 at C = 64 without pool): bn_bwd_apply's loop runs twice"""
    N, H, Cc = 5, 128, 64
    assert N * H * H > 65536
    _bn_bwd_check(f"bn_bwd {KIND[dt]} grid cap", _bn_bwd_case(dt, 0, N, H, Cc, seed=19))


@pytest.mark.parametrize("pool", [0, 1], ids=["pool0", "pool1"])
@pytest.mark.parametrize("dt", DTS)
def test_bn_gate_agreement(dt, pool):
    """General scale / shift: bn_dv must recompute v = x scale + shift with the arithmetic of bn_act_pool_kernel.  dbeta (start 0) of the
    backward equals the fp64 sum of dy over the outputs the forward launch of the same x, scale, shift stored as > 0, within C T"""
    N, H, Cc = 3, 32, 64
    fw = _act_pool_case(dt, pool, N, H, Cc, "general", 40 + pool)
    r = _bn_bwd_case(dt, pool, N, H, Cc, general=True, seed=40 + pool, dbeta_zero=True, x_ten=fw["x"])
    assert torch.equal(r["sc"], fw["sc"].float()) and torch.equal(r["sh"], fw["sh"].float())
    out = fw["out"].value()
    live = out != 0
    tiny = float(out[live].abs().min())
    print(f"bn_gate_agreement: {int(live.sum())} of {out.numel()} outputs > 0, the smallest {tiny:.3e}")
    assert bool((out >= 0).all()) and tiny >= 2.0 ** -126 and 0.05 < float(live.double().mean()) < 0.99
    dy = r["dy"].val
    r["db"].check(f"bn_gate_agreement {KIND[dt]} pool={pool} dbeta", (dy * live).sum((0, 1, 2)), (dy.abs() * live).sum((0, 1, 2)), layout="c")


# ----------------------------------------------------------------------------------------------------------- f32 conv + folded BN + ReLU
def _conv_bn_case(cin, cout, shape, seed):
    lib = _lib()
    H, W = SHAPES[shape]
    tiles = _tiles(F32, 1, cin, cout, H, W)
    M = 2
    if shape == "multi":        # at least twice as many tiles as the persistent grid, and not a multiple of it
        M = -(-2 * _grid(1, cout, 1 << 30) // tiles) + 3
        assert M * tiles >= 2 * _grid(1, cout, M * tiles)
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn((cout, cin, 3, 3), generator=g) * (0.05 if cin == 64 else 0.035)).to(torch.bfloat16).float()
    sc, sh = general_affine(cout, seed + 1)
    x = Ten((M, H, W, cin), F32, rnd((M, H, W, cin), seed + 2, BF16))
    wd, scd, shd = V(w.reshape(-1)), V(sc), V(sh)
    pk = torch.empty(cin * cout * 9, dtype=torch.float32, device="cuda")
    assert lib.hrn_kt_conv_pack(F32, cin, cout, wd.ptr, _p(pk), _stream()) == 0
    out = Ten((M, H, W, cout), F32)
    assert lib.hrn_kt_sn_conv_bn_relu(cin, cout, x.ptr, _p(pk), scd.ptr, shd.ptr, out.ptr, M, H, W, _stream()) == 0
    torch.cuda.synchronize()
    assert x.unchanged() and wd.unchanged() and scd.unchanged() and shd.unchanged() and out.guard_ok()
    return dict(got=_nchw(out.value()), x=x.val, w=w.double(), sc=sc.double(), sh=sh.double())


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("cin,cout", [(64, 64), (64, 128), (128, 128)], ids=["64x64", "64x128", "128x128"])
def test_conv_bn_relu(cin, cout, shape):
    """conv3x3_kernel<F32> with ConvParams::scale / bias (= shift) / relu as api.hip sets them for eval: ReLU(conv(x) scale + shift)"""
    r = _conv_bn_case(cin, cout, shape, 300 + cin + list(SHAPES).index(shape))
    want, T = ref_conv_bn_relu(r["x"], r["w"], r["sc"], r["sh"])
    assert bool((want == 0).any()) and bool((want > 0).any())
    _close(f"conv_bn_relu {cin}->{cout} {shape}", "f32", r["got"], want, T, layout="m c y x")


# ----------------------------------------------------------------------------------------------------------- plane mean
@pytest.mark.parametrize("hw", [1, 255, 257, 16384], ids=lambda v: f"hw{v}")
def test_plane_mean(hw):
    """plane_mean_kernel: the mean of each of B x 2 planes, summed in fp64"""
    lib = _lib()
    planes = 6
    x = V(torch.randn((planes, hw), generator=torch.Generator().manual_seed(hw)) + 0.5)
    mean = Ten((planes,), F32)
    assert lib.hrn_kt_sn_plane_mean(x.ptr, mean.ptr, planes, hw, _stream()) == 0
    torch.cuda.synchronize()
    assert x.unchanged() and mean.guard_ok()
    _close(f"plane_mean hw={hw}", "f32", mean.value(), x.val.mean(1), x.val.abs().mean(1), layout="plane")


@pytest.mark.parametrize("hw,planes", [(1, 6), (255, 6), (257, 6), (16384, 6), (16384, 65)], ids=["hw1", "hw255", "hw257", "hw16384", "cap"])
def test_sub_plane_mean(hw, planes):
    """sub_plane_mean_kernel: out = g - means[plane], bit for bit against float32 torch; "cap": above 4096 x 256 elements"""
    lib = _lib()
    if planes == 65:
        assert planes * hw > 4096 * 256
    gen = torch.Generator().manual_seed(hw + planes)
    g, means = V(torch.randn((planes, hw), generator=gen)), V(torch.randn(planes, generator=gen) * 0.1)
    out = Ten((planes, hw), F32)
    assert lib.hrn_kt_sn_sub_plane_mean(g.ptr, means.ptr, out.ptr, planes, hw, _stream()) == 0
    torch.cuda.synchronize()
    assert g.unchanged() and means.unchanged() and out.guard_ok()
    _bits_equal(f"sub_plane_mean hw={hw} planes={planes}", _payload(out), _payload(g) - _payload(means)[:, None])


# ----------------------------------------------------------------------------------------------------------- the stem's data gradient
STEM_DGRAD_SHAPES = {"1x1": (3, 1, 1), "2x3": (4, 2, 3), "17x50": (2, 17, 50)}


@pytest.mark.parametrize("shape", list(STEM_DGRAD_SHAPES))
@pytest.mark.parametrize("dt", DTS)
def test_stem_dgrad(dt, shape):
    """stem_dgrad_kernel<ST>: din (M, 2, H, W) f32 per element; a chain of 9 x 64 fused multiply-adds per output"""
    lib = _lib()
    M, H, W = STEM_DGRAD_SHAPES[shape]
    c = _seq_const(f"stem_dgrad {shape}", 9 * 64)
    g, w = Ten((M, H, W, 64), dt, rnd((M, H, W, 64), 50 + H, dt)), V(_stem_dgrad_w(51))
    din = Ten((M, 2, H, W), F32)
    assert lib.hrn_kt_sn_stem_dgrad(dt, g.ptr, w.ptr, din.ptr, M, H, W, _stream()) == 0
    torch.cuda.synchronize()
    assert g.unchanged() and w.unchanged() and din.guard_ok()
    want, T = ref_stem_dgrad(g.val, w.val.reshape(64, 2, 3, 3))
    _close(f"stem_dgrad {KIND[dt]} {shape}", "f32", din.value(), want, T, c=c, layout="m c y x")


@pytest.mark.parametrize("dt", DTS)
def test_stem_dgrad_grid_cap(dt):
    """M H W above ew_grid's cap of 4096 x 256 pixels with small images: the grid-stride loop runs twice.  g is built on the device from
    small integers (k / 4, |k| <= 8: bf16-representable) and the reference goes in chunks of images, to keep host memory down"""
    lib = _lib()
    H, W = 3, 5
    M = 4096 * 256 // (H * W) + 3
    assert M * H * W > 4096 * 256
    c = _seq_const("stem_dgrad grid cap", 9 * 64)
    k = torch.randint(-8, 9, (M, H, W, 64), generator=torch.Generator().manual_seed(52), dtype=torch.int8)
    tdt = torch.float32 if dt == F32 else torch.bfloat16
    gd = torch.cat([(k.cuda().float() / 4).to(tdt).reshape(-1), torch.full((64,), float("nan"), dtype=tdt, device="cuda")])
    w = V(_stem_dgrad_w(53))
    din = Ten((M, 2, H, W), F32)
    assert lib.hrn_kt_sn_stem_dgrad(dt, _p(gd), w.ptr, din.ptr, M, H, W, _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(gd[:k.numel()].float(), k.cuda().reshape(-1).float() / 4) and w.unchanged() and din.guard_ok()
    got, w64 = din.value(), w.val.reshape(64, 2, 3, 3)
    worst, step = 0.0, 8192
    for m0 in range(0, M, step):
        want, T = ref_stem_dgrad(k[m0:m0 + step].to(D) / 4, w64)
        worst = max(worst, _ratio("f32", got[m0:m0 + step], want, T * (c / C))[0])
    print(f"stem_dgrad {KIND[dt]} grid cap M={M}: max error / bound {worst:.3e}")
    assert worst <= 1.0


# ----------------------------------------------------------------------------------------------------------- fc1's input adapters
def _fc_to_ref_case(dt, B, masked, seed=60):
    lib = _lib()
    y = Ten((B, 256, 128), dt, rnd((B, 256, 128), seed + B, dt))
    mask = _mask(B, seed + 1) if masked else None
    md = mask.cuda() if masked else None
    xr = Ten((B, FCK), F32)
    assert lib.hrn_kt_sn_fc_to_ref(dt, y.ptr, _p(md), xr.ptr, B, _stream()) == 0
    torch.cuda.synchronize()
    assert y.unchanged() and xr.guard_ok() and (not masked or torch.equal(md.cpu(), mask))
    return y, mask, xr


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("B", [1, 3, 33], ids=lambda v: f"B{v}")
@pytest.mark.parametrize("dt", DTS)
def test_fc_to_ref(dt, B, masked):
    """fc_to_ref_kernel<ST>: xr[b][c 256 + hw] = y[b][hw][c] (x 2 where the mask keeps it, 0 where not), bit for bit"""
    y, mask, xr = _fc_to_ref_case(dt, B, masked)
    _bits_equal(f"fc_to_ref {KIND[dt]} B={B} masked={masked}", _payload(xr), _stored(ref_fc_to_ref(y.val, mask), F32))


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("B", [1, 3, 33], ids=lambda v: f"B{v}")
@pytest.mark.parametrize("dt", DTS)
def test_fc_from_ref(dt, B, masked):
    """fc_from_ref_kernel<ST>: dy[b][hw][c] = dxr[b][c 256 + hw] (x 2 / 0), f32 bit for bit, bf16 one round to nearest even.  B = 33 is above
    ew_grid's cap (33 x 32768 > 4096 x 256 elements)"""
    lib = _lib()
    if B == 33:
        assert B * FCK > 4096 * 256
    dxr = V(torch.randn((B, FCK), generator=torch.Generator().manual_seed(70 + B)))
    mask = _mask(B, 71) if masked else None
    md = mask.cuda() if masked else None
    dy = Ten((B, 256, 128), dt)
    assert lib.hrn_kt_sn_fc_from_ref(dt, dxr.ptr, _p(md), dy.ptr, B, _stream()) == 0
    torch.cuda.synchronize()
    assert dxr.unchanged() and dy.guard_ok() and (not masked or torch.equal(md.cpu(), mask))
    _bits_equal(f"fc_from_ref {KIND[dt]} B={B} masked={masked}", _payload(dy), _stored(ref_fc_from_ref(dxr.val, mask).contiguous(), dt))


# ----------------------------------------------------------------------------------------------------------- the fully connected tail
FC_B = [1, 2, 31, 32, 33, 64, 65]


@functools.lru_cache(maxsize=1)
def _fc1_weight():
    """fc1.weight (1024, 32768), bf16-representable: (CPU f32, device f32).  134 MB each, made once for the file"""
    w = (torch.randn((1024, FCK), generator=torch.Generator().manual_seed(80)) * 0.01).to(torch.bfloat16).float()
    return w, w.cuda()


def _fc1_weight_unchanged():
    w, wd = _fc1_weight()
    return bool((wd == w.cuda()).all())


def _fc1_run(xr, bias):
    """hrn_launch_fc1 on xr (a Ten (B, 32768)) -> y (B, 1024) fp64; NaN behind xr and behind y"""
    lib = _lib()
    B = xr.shape[0]
    _, wd = _fc1_weight()
    y = NanTen((B, 1024), F32)
    nbytes = lib.hrn_kt_sn_fc1_partial_bytes()
    assert nbytes == 32 * 32 * 1024 * 4
    part = torch.full((nbytes // 4 + 64,), float("nan"), device="cuda")
    assert lib.hrn_kt_sn_fc1(xr.ptr, _p(wd), bias.ptr, y.ptr, B, _p(part), _stream()) == 0
    torch.cuda.synchronize()
    assert xr.unchanged() and bias.unchanged() and _fc1_weight_unchanged(), "an input was written"
    assert y.guard_ok() and bool(torch.isnan(part[nbytes // 4:]).all()), "a write past an output"
    return y.value()


def _fc1_case(B):
    xr = V(rnd((B, FCK), 81 + B, BF16), NanTen)
    bias = V(rnd((1024,), 82, BF16) * 0.5)
    assert len({tuple(row[:4].tolist()) for row in xr.val}) == B          # every sample distinct
    return dict(got=_fc1_run(xr, bias), xr=xr.val, bias=bias.val)


@pytest.mark.parametrize("B", FC_B, ids=lambda v: f"B{v}")
def test_fc1(B):
    """fc1_mfma_kernel + fc1_finish_kernel through hrn_launch_fc1 (groups of 32 samples): ReLU(b + xr W^T) per element"""
    r = _fc1_case(B)
    c = _seq_const(f"fc1 B={B}", FC1_NSEQ)
    want, T = ref_fc1(r["xr"], _fc1_weight()[0], r["bias"])
    assert bool((want == 0).any()) and bool((want > 0).any())
    _close(f"fc1 B={B}", "f32", r["got"], want, T, c=c, layout="b j")


def _fc_chain_case():
    """fc_to_ref (bf16-representable y, dropout mask) -> fc1, B = 3"""
    y, mask, xr = _fc_to_ref_case(F32, 3, True, seed=83)
    xr.bits0 = xr.raw.cpu()                     # what fc_to_ref left: fc1's input from here on
    bias = V(rnd((1024,), 82, BF16) * 0.5)
    return dict(got=_fc1_run(xr, bias), y=y.val, mask=mask, bias=bias.val)


def test_fc_to_ref_fc1_chain():
    """the two launches as the forward chains them: ReLU(F.linear(dropout(flatten_CHW(y)), W, b))"""
    r = _fc_chain_case()
    c = _seq_const("fc_to_ref + fc1", FC1_NSEQ)
    want, T = ref_fc1(ref_fc_to_ref(r["y"], r["mask"]), _fc1_weight()[0], r["bias"])
    _close("fc_to_ref + fc1", "f32", r["got"], want, T, c=c, layout="b j")


@pytest.mark.parametrize("B", FC_B, ids=lambda v: f"B{v}")
def test_fc2(B):
    """fc2_kernel: theta (B, 2) = y w2^T; four products per thread, then the shuffle tree"""
    lib = _lib()
    y, w2 = V(rnd((B, 1024), 90 + B, BF16), NanTen), V(rnd((2, 1024), 91, BF16) * 0.125)
    theta = NanTen((B, 2), F32)
    assert lib.hrn_kt_sn_fc2(y.ptr, w2.ptr, theta.ptr, B, _stream()) == 0
    torch.cuda.synchronize()
    assert y.unchanged() and w2.unchanged() and theta.guard_ok()
    want, T = ref_fc2(y.val, w2.val)
    _close(f"fc2 B={B}", "f32", theta.value(), want, T, layout="b o")


def _fc2_bwd_case(B, null=None):
    lib = _lib()
    dth, w2 = V(rnd((B, 2), 100 + B, BF16)), V(rnd((2, 1024), 101, BF16) * 0.125)
    y1 = V(torch.relu(rnd((B, 1024), 102 + B, BF16)))                       # the stored ReLU output: exact zeros at about half
    dz1 = NanTen((B, 1024), F32)
    dw2, db1 = Acc((2, 1024), 103, none=null == "dw2"), Acc((1024,), 104, none=null == "db1")
    assert lib.hrn_kt_sn_fc2_bwd(dth.ptr, y1.ptr, w2.ptr, dz1.ptr, dw2.ptr, db1.ptr, B, _stream()) == 0
    torch.cuda.synchronize()
    assert dth.unchanged() and y1.unchanged() and w2.unchanged() and dz1.guard_ok()
    return dict(dz1=dz1.value(), dw2=dw2, db1=db1, args=(dth.val, y1.val, w2.val))


@pytest.mark.parametrize("B", FC_B, ids=lambda v: f"B{v}")
@pytest.mark.parametrize("null", [None, "dw2", "db1"], ids=["all", "no-dw2", "no-db1"])
def test_fc2_bwd(null, B):
    """fc2_bwd_kernel: dz1 written (gate y1 > 0 on the stored y1), dw2 and db1 accumulated, each NULL in turn; chains of B <= 65 terms"""
    r = _fc2_bwd_case(B, null)
    y1 = r["args"][1]
    assert 0.3 < float((y1 == 0).double().mean()) < 0.7
    ref = ref_fc2_bwd(*r["args"])
    _close(f"fc2_bwd B={B} null={null} dz1", "f32", r["dz1"], *ref["dz1"], layout="b j")
    r["dw2"].check(f"fc2_bwd B={B} dw2", *ref["dw2"], layout="o j")
    r["db1"].check(f"fc2_bwd B={B} db1", *ref["db1"], layout="j")


@pytest.mark.parametrize("B", [1, 31, 32, 33], ids=lambda v: f"B{v}")
def test_fc1_bwd_w(B):
    """fc1_bwd_w_kernel through hrn_launch_sn_fc1_bwd_w: dw1 (1024, 32768) += dz1^T xr over all 33.5 M elements, 32 products per launch
    and one addition per group; compared in blocks of 128 rows"""
    lib = _lib()
    dz1, xr = V(rnd((B, 1024), 110 + B, BF16)), V(rnd((B, FCK), 111 + B, BF16))
    dw1 = Acc((1024, FCK), 112)
    assert lib.hrn_kt_sn_fc1_bwd_w(dz1.ptr, xr.ptr, dw1.ptr, B, _stream()) == 0
    torch.cuda.synchronize()
    assert dz1.unchanged() and xr.unchanged()
    assert bool(torch.isnan(dw1.buf[dw1.n:]).all()), "a write past the gradient"
    worst, rows = (0.0, None), 128
    for j0 in range(0, 1024, rows):
        got = dw1.buf[j0 * FCK:(j0 + rows) * FCK].double().cpu().reshape(rows, FCK)
        s0 = dw1.start[j0 * FCK:(j0 + rows) * FCK].double().reshape(rows, FCK)
        want, T = ref_fc1_bwd_w(dz1.val, xr.val, j0, j0 + rows)
        r, idx = _ratio("f32", got, s0 + want, s0.abs() + T)
        if r >= worst[0]:
            worst = (r, (j0 + int(idx[0]), int(idx[1])))
    del dw1
    print(f"fc1_bwd_w B={B}: max error / bound {worst[0]:.3e} at (j k) = {worst[1]}")
    assert worst[0] <= 1.0


@pytest.mark.parametrize("B", [1, 31, 32, 33, 65], ids=lambda v: f"B{v}")
def test_fc1_bwd_x(B):
    """fc1_bwd_x_kernel through hrn_launch_sn_fc1_bwd_x: dxr (B, 32768) = dz1 W per element; the rows behind the batch stay untouched"""
    lib = _lib()
    c = _seq_const(f"fc1_bwd_x B={B}", FCX_NSEQ)
    w, wd = _fc1_weight()
    dz1 = V(rnd((B, 1024), 120 + B, BF16), NanTen)
    dxr = Ten((B + 2, FCK), F32)
    assert lib.hrn_kt_sn_fc1_bwd_x(dz1.ptr, _p(wd), dxr.ptr, B, _stream()) == 0
    torch.cuda.synchronize()
    assert dz1.unchanged() and _fc1_weight_unchanged() and dxr.guard_ok()
    assert bool((dxr.raw[B * FCK * 2:dxr.words] == SENT).all()), "rows >= B of dxr were written"
    want, T = ref_fc1_bwd_x(dz1.val, w)
    _close(f"fc1_bwd_x B={B}", "f32", dxr.value()[:B], want, T, c=c, layout="b k")


# ----------------------------------------------------------------------------------------------------------- fused Adam
ADAM_N = [1, 3, 4, 5, 1027, 4096 * 256 * 4 + 7]          # the last: above the grid of 4096 x 256 threads x 4 elements, with a scalar tail


def _adam_case(n, setting):
    from hrnet_hip import binding
    lib = binding.load_library()
    lr, b1, b2, wd, step = setting
    nan = torch.full((64,), float("nan"))
    cpu = adam_inputs(n, 130 + n % 1000)
    dev = [torch.cat([t, nan]).cuda() for t in cpu]
    assert lib.hrn_adam_step(_p(dev[0]), _p(dev[1]), _p(dev[2]), _p(dev[3]), n, lr, b1, b2, ADAM_EPS, wd, step, _stream()) == 0
    torch.cuda.synchronize()
    got = [t.cpu() for t in dev]
    assert all(bool(torch.isnan(t[n:]).all()) for t in got), "a write past a buffer"
    assert torch.equal(got[1][:n].view(torch.int32), cpu[1].view(torch.int32)), "the gradient was written"
    hyper = [float(np.float32(h)) for h in (lr, b1, b2, ADAM_EPS, wd)] + [step]          # as the ABI receives them
    return dict(p=got[0][:n].double(), m=got[2][:n].double(), v=got[3][:n].double(), ins=[t.double() for t in cpu], hyper=hyper)


@pytest.mark.parametrize("si", range(len(ADAM_SETTINGS)), ids=lambda v: f"s{v}")
@pytest.mark.parametrize("n", ADAM_N, ids=lambda v: f"n{v}")
def test_adam(n, si):
    """adam_kernel through hrn_adam_step: m', v' within C T (v': + 2^-126, where g^2 underflows), p' from the stored m', v'"""
    r = _adam_case(n, ADAM_SETTINGS[si])
    tag = f"adam n={n} setting {ADAM_SETTINGS[si]}"
    if n >= 1027:
        p, g, m, v = r["ins"]
        assert bool((g == 0).any()) and bool((v == 0).any()) and bool((m == 0).any()) and bool((g == float(np.float32(1e-30))).any())
    m1, Tm, v1, Tv, _, _ = ref_adam(*r["ins"], *r["hyper"])
    _close(tag + " m'", "f32", r["m"], m1, Tm)
    _assert_bound(tag + " v'", r["v"], v1, C * Tv + 2.0 ** -126)
    ratio = _adam_p_ratio(r)
    print(f"{tag} p': max error / bound {float(ratio.max()):.3e} at {int(ratio.argmax())}")
    assert float(ratio.max()) <= 1.0


# ----------------------------------------------------------------------------------------------------------- negative controls
CONTROLS = ["pool_last_maximum", "scale_unbiased_variance", "running_var_biased", "fc1_hwc_flatten", "dropout_keep_scale_1", "fc1_group_shift",
            "fc2_bwd_gate_ge", "adam_no_bias_correction_v", "adam_eps_inside_sqrt"]


@pytest.mark.parametrize("control", CONTROLS)
def test_negative_control(control):
    """The comparison against a reference that is wrong in one way must FAIL on the same GPU output that passes against the right one."""
    if control == "pool_last_maximum":
        r = _bn_bwd_case(BF16, 1, 3, 32, 64, seed=11)
        ok = _close("bn_bwd dx (right reference)", "bf16", r["dx"], *ref_bn_bwd(*r["args"])["dx"], layout="n y x c")
        worst, _ = _ratio("bf16", r["dx"], *ref_bn_bwd(*r["args"], last_max=True)["dx"])
    elif control in ("scale_unbiased_variance", "running_var_biased"):
        r = _bn_stats_case(F32, 64, 257)
        key = "scale" if control == "scale_unbiased_variance" else "running_var"
        args = (r["x"], r["gamma"], r["beta"], r["rm0"], r["rv0"])
        ok = _close(f"bn_stats {key} (right reference)", "f32", r["got"][key], *ref_bn_stats(*args)[key], layout="c")
        bad = ref_bn_stats(*args, unbiased_scale=control == "scale_unbiased_variance", biased_running=control == "running_var_biased")
        worst, _ = _ratio("f32", r["got"][key], *bad[key])
    elif control in ("fc1_hwc_flatten", "dropout_keep_scale_1"):
        r = _fc_chain_case()
        c = max(C, FC1_NSEQ * 2.0 ** -24)
        w = _fc1_weight()[0]
        want, T = ref_fc1(ref_fc_to_ref(r["y"], r["mask"]), w, r["bias"])
        ok = _close("fc_to_ref + fc1 (right reference)", "f32", r["got"], want, T, c=c, layout="b j")
        xr = ref_fc_to_ref(r["y"], r["mask"], hwc=True) if control == "fc1_hwc_flatten" else ref_fc_to_ref(r["y"], r["mask"], keep=1.0)
        bad, T = ref_fc1(xr, w, r["bias"])
        worst, _ = _ratio("f32", r["got"], bad, T * (c / C))
    elif control == "fc1_group_shift":
        r = _fc1_case(33)
        c = max(C, FC1_NSEQ * 2.0 ** -24)
        w = _fc1_weight()[0]
        want, T = ref_fc1(r["xr"], w, r["bias"])
        ok = _close("fc1 B=33 (right reference)", "f32", r["got"], want, T, c=c, layout="b j")
        bad, T = ref_fc1(r["xr"], w, r["bias"], shift_group=True)
        worst, _ = _ratio("f32", r["got"], bad, T * (c / C))
    elif control == "fc2_bwd_gate_ge":
        r = _fc2_bwd_case(33)
        ok = _close("fc2_bwd dz1 (right reference)", "f32", r["dz1"], *ref_fc2_bwd(*r["args"])["dz1"], layout="b j")
        worst, _ = _ratio("f32", r["dz1"], *ref_fc2_bwd(*r["args"], gate_ge=True)["dz1"])
    else:
        r = _adam_case(1027, ADAM_SETTINGS[1])
        ok = float(_adam_p_ratio(r).max())
        assert ok <= 1.0
        wrong = dict(no_bc2=True) if control == "adam_no_bias_correction_v" else dict(eps_inside=True)
        worst = float(_adam_p_ratio(r, **wrong).max())
    print(f"{control}: error / bound against the wrong reference {worst:.3e} (right one {ok:.3e})")
    assert ok <= 1.0 < worst, f"{control}: the comparison does not tell the wrong reference from the right one"
