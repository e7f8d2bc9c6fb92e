"""GPU (-m gpu): the non-convolution kernels of HRNet's backward, per element, against torch CPU float64.

Each launcher is called on its own through the hooks of kernel_test.h (hrn_kt_*, bound by tests/kt.py), exactly as train.hip / api.hip call it, on the stored tensors it
would see in production; the reference (the ref_* functions of tests/kernel_refs.py, checked against torch autograd by tests/test_kernels_bwd_host.py) is
the same operation in fp64 on the exact values the kernel reads (hi + lo for bf16x3), so no PReLU sign can differ between the two.
Operands are chosen so that the products a kernel forms in fp32 are exact (dy / dsn of at most 16 significant bits, slopes 0.25, 1,
BF(-0.3), 1.5, 2^-20, 0; alphas 0, 1, 0.75): only the accumulation order and one rounding of the stored output remain.
Bound per element, T = the same expression on absolute values, C = kernel_bounds.C = 1e-5 (168 fp32 roundings):
  bf16 output                          |got - want| <= 1/2 ulp_bf16(max(|got|, |want|)) + C T
  bf16x3 output (hi + lo)              |got - want| <= 2^-16 |want| + C T
  f32 output, every parameter gradient |got - want| <= C T       (accumulated gradients: want = start + sum, T = |start| + sum |terms|)
Kernels that add in fp32 along a chain keep it at <= 128 terms by the choice of shape; where a case cannot (stem_wgrad's many-tile case,
stem_dgrad_route's and stem_dgrad_ref's 9 x 64 taps per view) its constant is max(C, n_seq 2^-24) with n_seq computed from the shape, and printed.
bf16x3 tensors lie as the backward lays them out (the lo plane directly behind the hi plane) in a buffer with sentinels behind; outputs
start as sentinels, accumulated gradients from random values; every test asserts that the guards and the inputs are bit-identical after.
Bit-exact: planes_to_f32 / f32_to_planes and the median.

Template instance -> production call site (train.hip unless noted) -> tests
  prelu_bwd_bias_kernel<64|128, F32|BF16|BF16X3> + colsum_finish / scalar_finish
                                        every PReLU of encoder (C 64) and fusion (C 128, 64)   test_prelu_bwd_bias[f32|bf16|bf16x3-C*-*-a*]
  colsum_kernel<64|128, *>              the encoder's final bias; ShiftNet's conv biases       test_colsum[*-C*-*]
  add_kernel<*>                         residual sums of the training forward                    test_add[*]
  fuse_update_kernel<*>                 the fusion levels, forward for training                  test_fuse_update[*-n*-B*-*]
  pair_add_kernel<*>                    t2 = z + u of a fusion level, forward for training       test_pair_add[*-n*-B*-*]
  fuse_df_kernel<*>                     d f of a level                                           test_fuse_df[*-n*-B*-*]
  fuse_scatter_kernel<*>                d views of a level                                       test_fuse_scatter[*-n*-B*-*]
  alpha_grad_partial_kernel<*> + finish d alphas per level                                       test_alpha_grad[*-*]
  stem_wgrad_kernel<*> + finish         HRNet's stem (sub NULL), ShiftNet's stem (`sub`, strides 2 plane)
                                                                                                 test_stem_wgrad[*-*-*]
  stem_dgrad_route_kernel<*>            d lrs with the median routing                            test_stem_dgrad_route[*-V*-B*-*]
  stem_dgrad_ref_kernel<*>              d lrs and d ref with the frame given from outside (hrn_hrnet_backward_ref)
                                                                                                 test_stem_dgrad_ref[*-V*-B*-*], test_stem_dgrad_ref_agrees_with_route[*-V*]
  stem_kernel<*> (only_if_nonpos)       the gated recompute of the stem's pre-activation         test_stem_pre[*-*-*]
  decoder_bwd_kernel<2,4|3,9|4,8> + decoder_bwd_finish_kernel<S>   (f32)
                                        the decoder's backward, every mode                       test_decoder_bwd[S*-*], test_decoder_bwd_null[S*-*]
  planes_to_f32_kernel<true|false>      the fused state in front of the f32 decoder backward     test_planes_to_f32[two|one-*]
  f32_to_planes_kernel<true|false>      its gradient behind it                                   test_f32_to_planes[two|one-*]
  median_kernel                         the reference frame, inference and training (api.hip)    test_median[V*], test_median_grid_cap
Negative controls (test_negative_control) run on the CPU against the GPU output that passed and assert that the comparison FAILS.
"""
import ctypes

import pytest
import torch

from kernel_bounds import BF, C, GUARD, NAN16, SENT, Acc, Ten, _assert_close, _nchw, _ratio, rnd
from kernel_refs import (DEC_SLOPES, LEVELS, PRELU_SLOPES, _alphas, decoder_inputs, prelu_inputs, ref_alpha_grad, ref_decoder_bwd, ref_decoder_up,
                         ref_fuse_df, ref_fuse_scatter, ref_fuse_update, ref_median, ref_pair_add, ref_prelu_bwd, ref_route_index, ref_split_planes,
                         ref_stem_dgrad_ref, ref_stem_dgrad_route, ref_stem_pre, ref_stem_wgrad, route_inputs, split_inputs)
from kt import BF16, BF16X3, F32, _cus, _p, _stream, lib as _lib

pytestmark = pytest.mark.gpu

DTS = [pytest.param(F32, id="f32"), pytest.param(BF16, id="bf16"), pytest.param(BF16X3, id="bf16x3")]
KIND = {F32: "f32", BF16: "bf16", BF16X3: "x3"}


# ----------------------------------------------------------------------------------------------------------- the test inputs
def k16(shape, g):
    """values k / 2^16, 0 <= k < 2^16"""
    return (torch.randint(0, 1 << 16, shape, generator=g).double() / 65536.0).float()


def _scratch(lib):
    return torch.empty(lib.hrn_kt_wgrad_scratch_bytes(), dtype=torch.uint8, device="cuda")


def _dev1(a):
    return torch.tensor([a], dtype=torch.float32, device="cuda")


# ----------------------------------------------------------------------------------------------------------- prelu_bwd_bias, colsum
ROWS = ["1", "RP-1", "S-1", "S", "S+1", "2S+1", "4S+3", "5S+RP+1"]


def _rows(name, Cc):
    """512 workgroups x RP = 1024 / C row phases: one sweep covers S = 512 RP rows; the main loops are unrolled by 2 (prelu) and 4 (colsum)"""
    RP = 1024 // Cc
    S = 512 * RP
    return {"1": 1, "RP-1": RP - 1, "S-1": S - 1, "S": S, "S+1": S + 1, "2S+1": 2 * S + 1, "4S+3": 4 * S + 3, "5S+RP+1": 5 * S + RP + 1}[name]


def _prelu_case(dt, Cc, rows, a, alias, null, seed):
    lib = _lib()
    dyv, srcv = prelu_inputs(rows, Cc, dt, seed)
    from_y = a > 0
    dy = Ten((rows, Cc), dt, dyv)
    src = Ten((rows, Cc), dt, srcv)
    other = Ten((rows, Cc), dt, None, fill=NAN16)       # the tensor the kernel must not read: NaN
    y, xpre = (src, other) if from_y else (other, src)
    g = dy if alias else Ten((rows, Cc), dt)
    db, dsl = Acc((Cc,), seed + 2, none=null == "db"), Acc((), seed + 3, none=null == "dslope")
    sc, sl = _scratch(lib), _dev1(a)
    rc = lib.hrn_kt_prelu_bwd_bias(dt, dy.ptr, y.ptr, xpre.ptr, _p(sl), g.ptr, rows, Cc, dsl.ptr, db.ptr, _p(sc), _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert y.unchanged() and xpre.unchanged() and (alias or dy.unchanged()), "an input was written"
    assert g.guard_ok() and y.guard_ok(), "a write past a tensor"
    return dict(g=g.value(), dy=dy.val, src=src.val, a=a, db=db, dsl=dsl, kind=KIND[dt])


# every (storage, C, rows, slope); g aliasing dy or apart and the NULL (frozen) db / dslope rotate over them
PRELU_CASES = []
for _di, _dt in enumerate((F32, BF16, BF16X3)):
    for _ci, _Cc in enumerate((64, 128)):
        for _ri, _rn in enumerate(ROWS):
            for _ai, _a in enumerate(PRELU_SLOPES):
                _k = _di + _ci + _ri + _ai
                PRELU_CASES.append(pytest.param(_dt, _Cc, _rn, _a, _k % 2 == 0, [None, "db", None, "dslope"][(_k // 2 + _ai) % 4],
                                                id=f"{KIND[_dt].replace('x3', 'bf16x3')}-C{_Cc}-{_rn}-a{_ai}"))


@pytest.mark.parametrize("dt,Cc,rows_name,a,alias,null", PRELU_CASES)
def test_prelu_bwd_bias(dt, Cc, rows_name, a, alias, null):
    """prelu_bwd_bias_kernel<C, ST> + colsum_finish + scalar_finish: g per element, db per channel, dslope (fp64 accumulation: C)"""
    rows = _rows(rows_name, Cc)
    r = _prelu_case(dt, Cc, rows, a, alias, null, 1000 + rows % 977)
    tag = f"prelu_bwd_bias {r['kind']} C={Cc} rows={rows} a={a} alias={alias} null={null}"
    g, dslope, Ts, dbw, Tb = ref_prelu_bwd(r["dy"], r["src"], a)
    assert bool((r["src"] == 0).any()) and bool((r["src"] < 0).any()) and bool((r["src"] > 0).any())
    _assert_close(tag + " g", r["kind"], r["g"], g, g.abs(), layout="row c")
    r["db"].check(tag + " db", dbw, Tb, layout="c")
    r["dsl"].check(tag + " dslope", dslope, Ts, layout="")


@pytest.mark.parametrize("rows_name", ROWS)
@pytest.mark.parametrize("Cc", [64, 128], ids=["C64", "C128"])
@pytest.mark.parametrize("dt", DTS)
def test_colsum(dt, Cc, rows_name):
    """colsum_kernel<C, ST> + colsum_finish: db[c] += sum over rows"""
    lib = _lib()
    rows = _rows(rows_name, Cc)
    g = Ten((rows, Cc), dt, rnd((rows, Cc), 77 + rows % 991, dt))
    db = Acc((Cc,), 5)
    sc = _scratch(lib)
    assert lib.hrn_kt_colsum(dt, g.ptr, rows, Cc, db.ptr, _p(sc), _stream()) == 0
    torch.cuda.synchronize()
    assert g.unchanged()
    db.check(f"colsum {KIND[dt]} C={Cc} rows={rows}", g.val.sum(0), g.val.abs().sum(0), layout="c")


# ----------------------------------------------------------------------------------------------------------- the fusion level helpers
LEVEL_SIZES = [(1, "1"), (3, "1"), (1, "33x33"), (3, "33x33"), (1, "cap"), (3, "cap")]
LEVEL_CASES = []
for _dt in (F32, BF16, BF16X3):
    for _n in LEVELS:
        for _B, _hw in LEVEL_SIZES:
            for _ar in (0, 1):
                LEVEL_CASES.append(pytest.param(_dt, _n, _B, _hw, _ar, id=f"{KIND[_dt].replace('x3', 'bf16x3')}-n{_n}-B{_B}-{_hw}-ar{_ar}"))


def _level(n, B, hw_name):
    """-> half, pair_last, V (alphas per sample, > n), hw; "cap": B half hw just above 32768 pixels = the launchers' grid cap of 2048 x 256
    float4 units, so that the grid-stride loops of all three kernels run twice"""
    half, pair_last = n // 2, n - (n & 1) - 1
    hw = {"1": 1, "33x33": 33 * 33}.get(hw_name) or 32768 // (B * half) + 37
    if hw_name == "cap":
        assert B * half * hw > 32768
    return half, pair_last, n + 2, hw


def _fuse_update_case(dt, n, B, hw_name, ar):
    lib = _lib()
    half, pair_last, V, hw = _level(n, B, hw_name)
    stack = Ten((B, n, hw, 64), dt, rnd((B, n, hw, 64), 11 + n, dt))
    f = Ten((B, half, hw, 64), dt, rnd((B, half, hw, 64), 12 + n, dt))
    out = Ten((B, half, hw, 64), dt)
    al = _alphas(B, V, zero_at=pair_last)
    ad = al.cuda()
    assert lib.hrn_kt_fuse_update(dt, stack.ptr, n, f.ptr, _p(ad), V, pair_last, half, ar, out.ptr, hw, B, _stream()) == 0
    torch.cuda.synchronize()
    assert stack.unchanged() and f.unchanged() and out.guard_ok() and torch.equal(ad.cpu(), al)
    return dict(stack=stack, f=f, out=out, al=al, half=half, pair_last=pair_last)


@pytest.mark.parametrize("dt,n,B,hw_name,ar", LEVEL_CASES)
def test_fuse_update(dt, n, B, hw_name, ar):
    """fuse_update_kernel<ST>: s'[b][i] = s[b][i] + alpha[b][pair_last - i] f[b][i] (or f)"""
    r = _fuse_update_case(dt, n, B, hw_name, ar)
    want, T = ref_fuse_update(r["stack"].val, r["f"].val, r["al"], r["pair_last"], ar)
    _assert_close(f"fuse_update {KIND[dt]} n={n} B={B} hw={hw_name} ar={ar}", KIND[dt], r["out"].value(), want, T, layout="b v p c")
    if ar:      # where the partner's alpha is 0 the output IS its stack slot, bit for bit (both planes in bf16x3)
        zero = r["al"][:, r["pair_last"] - torch.arange(r["half"])] == 0
        assert bool(zero.any())
        for po, ps in zip(r["out"].planes(), r["stack"].planes()):
            assert torch.equal(po[zero].view(torch.int16 if dt != F32 else torch.int32), ps[:, :r["half"]][zero].view(torch.int16 if dt != F32 else torch.int32))


PAIR_ADD_CASES = [c for c in LEVEL_CASES if c.values[4] == 0]          # (no alpha residual in this kernel: one case per level and size)


@pytest.mark.parametrize("dt,n,B,hw_name,ar", PAIR_ADD_CASES)
def test_pair_add(dt, n, B, hw_name, ar):
    """pair_add_kernel<ST>: t2[b * half + v] = cat(s[b][v], s[b][pair_last - v]) + u, the unpaired view of an odd level unread; "cap": the
    grid-stride loop of its 4096 x 256 threads runs twice (B half hw 32 float4 units)"""
    lib = _lib()
    half, pair_last, _, hw = _level(n, B, hw_name)
    if hw_name == "cap":
        assert B * half * hw * 32 > 4096 * 256
    v = rnd((B, n, hw, 64), 14 + n, dt)
    if n & 1:
        v[:, n - 1] = float("nan")          # takes no part in any pair
    stack = Ten((B, n, hw, 64), dt, v)
    u = Ten((B, half, hw, 128), dt, rnd((B, half, hw, 128), 15 + n, dt))
    t2 = Ten((B, half, hw, 128), dt)
    assert lib.hrn_kt_pair_add(dt, stack.ptr, n, half, pair_last, u.ptr, t2.ptr, hw, B, _stream()) == 0
    torch.cuda.synchronize()
    assert stack.unchanged() and u.unchanged() and t2.guard_ok()
    want, T = ref_pair_add(stack.val, u.val, pair_last)
    assert bool(torch.isfinite(want).all())
    _assert_close(f"pair_add {KIND[dt]} n={n} B={B} hw={hw_name}", KIND[dt], t2.value(), want, T, layout="b v p c")


def _fuse_df_case(dt, n, B, hw_name, ar):
    lib = _lib()
    half, pair_last, V, hw = _level(n, B, hw_name)
    dsn = Ten((B, half, hw, 64), dt, rnd((B, half, hw, 64), 21 + n, dt))
    df = Ten((B, half, hw, 64), dt)
    al = _alphas(B, V)
    ad = al.cuda()
    assert lib.hrn_kt_fuse_df(dt, dsn.ptr, _p(ad), V, pair_last, half, ar, df.ptr, hw, B, _stream()) == 0
    torch.cuda.synchronize()
    assert dsn.unchanged() and df.guard_ok() and torch.equal(ad.cpu(), al)
    return dict(dsn=dsn, df=df, al=al, pair_last=pair_last, kind=KIND[dt])


@pytest.mark.parametrize("dt,n,B,hw_name,ar", LEVEL_CASES)
def test_fuse_df(dt, n, B, hw_name, ar):
    """fuse_df_kernel<ST>: df[b][i] = alpha[b][pair_last - i] ds'[b][i] (or ds')"""
    r = _fuse_df_case(dt, n, B, hw_name, ar)
    want, T = ref_fuse_df(r["dsn"].val, r["al"], r["pair_last"], ar)
    _assert_close(f"fuse_df {KIND[dt]} n={n} B={B} hw={hw_name} ar={ar}", KIND[dt], r["df"].value(), want, T, layout="b v p c")


def _fuse_scatter_case(dt, n, B, hw_name, ar):
    lib = _lib()
    half, pair_last, V, hw = _level(n, B, hw_name)
    dsn = Ten((B, half, hw, 64), dt, rnd((B, half, hw, 64), 31 + n, dt))
    dz = Ten((B, half, hw, 128), dt, rnd((B, half, hw, 128), 32 + n, dt))
    ds = Ten((B, n, hw, 64), dt)
    assert lib.hrn_kt_fuse_scatter(dt, dsn.ptr, dz.ptr, n, half, pair_last, ar, ds.ptr, hw, B, _stream()) == 0
    torch.cuda.synchronize()
    assert dsn.unchanged() and dz.unchanged() and ds.guard_ok()
    return dict(dsn=dsn, dz=dz, ds=ds, pair_last=pair_last, kind=KIND[dt])


@pytest.mark.parametrize("dt,n,B,hw_name,ar", LEVEL_CASES)
def test_fuse_scatter(dt, n, B, hw_name, ar):
    """fuse_scatter_kernel<ST>: dz and the pass-through to the level's input views; the unpaired view of an odd level gets exact zeros"""
    r = _fuse_scatter_case(dt, n, B, hw_name, ar)
    want, T = ref_fuse_scatter(r["dsn"].val, r["dz"].val, n, r["pair_last"], ar)
    got = r["ds"].value()
    _assert_close(f"fuse_scatter {KIND[dt]} n={n} B={B} hw={hw_name} ar={ar}", KIND[dt], got, want, T, layout="b v p c")
    if n & 1:
        for p in r["ds"].planes():
            assert bool((p[:, n - 1].view(torch.int16 if dt != F32 else torch.int32) == 0).all()), "the unpaired view is not exact +0"


@pytest.mark.parametrize("dt", DTS)
def test_add(dt):
    """add_kernel<ST>: o = a + b, below and above the grid cap (2048 x 256 float4 units)"""
    lib = _lib()
    for n in (4, 4 * 1089, 4 * (2048 * 256 + 77)):
        a, b, o = Ten((n,), dt, rnd((n,), 41, dt)), Ten((n,), dt, rnd((n,), 42, dt)), Ten((n,), dt)
        assert lib.hrn_kt_add(dt, a.ptr, b.ptr, o.ptr, n, _stream()) == 0
        torch.cuda.synchronize()
        assert a.unchanged() and b.unchanged() and o.guard_ok()
        _assert_close(f"add {KIND[dt]} n={n}", KIND[dt], o.value(), a.val + b.val, a.val.abs() + b.val.abs(), layout="i")


# ----------------------------------------------------------------------------------------------------------- alpha_grad
# name -> (B, n of the level, hw): nimg = B half images, P = clamp(ceil(2048 / nimg), 1, 64) parts per image
ALPHA_CASES = {"nimg1": (1, 2, 1089), "nimg3": (1, 6, 1089), "nimg3b": (3, 3, 200), "nimg40": (10, 9, 1089), "nimg2049-hw1": (683, 7, 1),
               "nimg1-hw1": (1, 2, 1)}


def _alpha_parts(nimg):
    return max(1, min(64, -(-2048 // nimg)))


@pytest.mark.parametrize("case", list(ALPHA_CASES))
@pytest.mark.parametrize("dt", DTS)
def test_alpha_grad(dt, case):
    """alpha_grad_partial_kernel<ST> + finish: d_alphas[b][pair_last - v] = sum dsn f, written; the other entries untouched"""
    lib = _lib()
    B, n, hw = ALPHA_CASES[case]
    half, pair_last, V = n // 2, n - (n & 1) - 1, n + 2
    nimg = B * half
    P = _alpha_parts(nimg)
    per = -(-16 * hw // P)
    n_seq = 4 * -(-per // 256)           # fused multiply-adds per thread, in fp32
    assert n_seq <= 128
    if case == "nimg40":
        assert P == 52 and per * P != 16 * hw
    if case == "nimg1-hw1":
        assert P > 16 * hw                # more parts than float4 units: empty parts
    dsn = Ten((B, half, hw, 64), dt, rnd((B, half, hw, 64), 51 + n, dt))
    f = Ten((B, half, hw, 64), dt, rnd((B, half, hw, 64), 52 + n, dt))
    da0 = torch.randn((B, V), generator=torch.Generator().manual_seed(53))
    da = torch.cat([da0.reshape(-1), torch.full((64,), float("nan"))]).cuda()
    nbytes = lib.hrn_kt_alpha_grad_scratch_bytes(nimg)
    assert nbytes == nimg * P * 8
    sc = torch.empty(nbytes + 64, dtype=torch.uint8, device="cuda")
    assert lib.hrn_kt_alpha_grad(dt, dsn.ptr, f.ptr, half, pair_last, _p(da), B, V, hw, _p(sc), nbytes, _stream()) == 0
    torch.cuda.synchronize()
    assert dsn.unchanged() and f.unchanged()
    got = da.cpu()
    assert bool(torch.isnan(got[B * V:]).all())
    got = got[:B * V].reshape(B, V)
    own = pair_last - torch.arange(half)
    rest = torch.ones(V, dtype=torch.bool)
    rest[own] = False
    assert torch.equal(got[:, rest].view(torch.int32), da0[:, rest].contiguous().view(torch.int32)), "an entry outside the level was written"
    want, T = ref_alpha_grad(dsn.val, f.val)
    print(f"alpha_grad {case}: P = {P}, per = {per}, n_seq = {n_seq}")
    _assert_close(f"alpha_grad {KIND[dt]} {case}", "f32", got[:, own].double(), want, T, layout="b v")


# ----------------------------------------------------------------------------------------------------------- the stem
STEM_SHAPES = {"1x1": (1, 1, 3), "2x3": (2, 3, 4), "9x27": (9, 27, 3), "15x33": (15, 33, 2), "17x50": (17, 50, 2), "9x63": (9, 63, 3),
               "16x64": (16, 64, 2), "multi": (3, 33, None)}
STEM_MODES = ["rep1", "rep3", "sub", "shiftnet"]      # HRNet (rep1 = 1, 3), `sub` given (rep1 = 3), ShiftNet's stride pattern with `sub`


@pytest.mark.parametrize("shape", list(STEM_SHAPES))
@pytest.mark.parametrize("mode", STEM_MODES)
@pytest.mark.parametrize("dt", DTS)
def test_stem_wgrad(dt, mode, shape):
    """stem_wgrad_kernel<ST> + finish through hrn_launch_stem_wgrad (sub NULL) / hrn_launch_stem_wgrad_sub: dw [64][2][3][3] +="""
    lib = _lib()
    H, W, M = STEM_SHAPES[shape]
    tiles_img = -(-W // 32) * -(-H // 8)
    if M is None:       # at least twice as many tiles as the grid of 4 CUs workgroups, and not a multiple of it
        M = -(-2 * 4 * _cus() // tiles_img) + 3
    tiles = M * tiles_img
    grid = min(4 * _cus(), tiles)
    n_seq = 64 * -(-tiles // grid)          # 64 pixels per thread per tile, in fp32, over the tiles of a workgroup
    c = C if n_seq <= 128 else max(C, n_seq * 2.0 ** -24)
    if shape == "multi":
        assert tiles >= 2 * grid
    else:
        assert n_seq <= 128
    gen = torch.Generator().manual_seed(61 + H + W)
    plane = H * W
    if mode == "shiftnet":      # x [M][2][H][W]: in0 = x (image stride 2 planes), in1 = x + plane, rep1 = 1
        x = k16((M, 2, H, W), gen)
        x0, x1, rep1, s0, s1 = x[:, 0], x[:, 1], 1, 2 * plane, 2 * plane
        xd = x.cuda()
        p0, p1 = _p(xd), ctypes.c_void_p(xd.data_ptr() + 4 * plane)
    else:
        rep1 = 1 if mode == "rep1" else 3
        x0, x1 = k16((M, H, W), gen), k16((-(-M // rep1), H, W), gen)
        d0, d1 = x0.cuda(), x1.cuda()
        p0, p1, s0, s1 = _p(d0), _p(d1), plane, plane
    sub = k16((M, 2), gen) if mode in ("sub", "shiftnet") else None
    subd = sub.cuda() if sub is not None else None
    g = Ten((M, H, W, 64), dt, rnd((M, H, W, 64), 62 + H, dt))
    dw = Acc((64, 2, 3, 3), 63)
    sc = _scratch(lib)
    assert lib.hrn_kt_stem_wgrad(dt, p0, s0, p1, rep1, s1, _p(subd), g.ptr, M, H, W, dw.ptr, _p(sc), _stream()) == 0
    torch.cuda.synchronize()
    assert g.unchanged()
    want, T = ref_stem_wgrad(x0.double(), x1.double(), rep1, sub.double() if sub is not None else None, g.val)
    print(f"stem_wgrad {shape}: M = {M}, tiles = {tiles}, grid = {grid}, n_seq = {n_seq}, constant = {c:.3e}")
    dw.check(f"stem_wgrad {KIND[dt]} {mode} {shape}", want, T, c=c, layout="co c ky kx")


ROUTE_SHAPES = {"2x3": (2, 3), "9x27": (9, 27), "15x33": (15, 33), "17x50": (17, 50)}
ROUTE_CASES = []
for _dt in (F32, BF16, BF16X3):
    for _V in (1, 2, 3, 8, 9, 10, 12):
        for _B in (1, 2):
            for _sh in ROUTE_SHAPES:
                ROUTE_CASES.append(pytest.param(_dt, _V, _B, _sh, id=f"{KIND[_dt].replace('x3', 'bf16x3')}-V{_V}-B{_B}-{_sh}"))


def _route_case(dt, V, B, shape):
    lib = _lib()
    H, W = ROUTE_SHAPES[shape]
    lrs, ref = route_inputs(B, V, H, W, 71 + V)
    dA = Ten((B * V, H, W, 64), dt, rnd((B * V, H, W, 64), 72 + V, dt))
    w = torch.randn((64, 2, 3, 3), generator=torch.Generator().manual_seed(73)) * 0.3
    d_lrs = torch.full((B * V * H * W + 64,), float("nan"), device="cuda")
    ld, rd, wd_, wt = lrs.cuda(), ref.cuda(), w.cuda(), torch.empty(64 * 18, device="cuda")
    assert lib.hrn_kt_stem_dgrad_route(dt, dA.ptr, _p(wd_), _p(wt), _p(ld), _p(rd), _p(d_lrs), B, V, H, W, _stream()) == 0
    torch.cuda.synchronize()
    assert dA.unchanged() and torch.equal(ld.cpu(), lrs) and torch.equal(rd.cpu(), ref) and torch.equal(wd_.cpu(), w)
    got = d_lrs.cpu()
    assert bool(torch.isnan(got[B * V * H * W:]).all())
    return dict(got=got[:B * V * H * W].reshape(B, V, H, W).double(), dA=dA.val, w=w.double(), lrs=lrs, ref=ref)


@pytest.mark.parametrize("dt,V,B,shape", ROUTE_CASES)
def test_stem_dgrad_route(dt, V, B, shape):
    """stem_dgrad_route_kernel<ST>: d_lrs per element, no element excluded.  Each view's two outputs are chains of 9 x 64 fused
    multiply-adds in fp32 and channel 1 is then summed over the V views: n_seq = 9 * 64 + V"""
    r = _route_case(dt, V, B, shape)
    n_seq = 9 * 64 + V
    c = max(C, n_seq * 2.0 ** -24)
    want, T = ref_stem_dgrad_route(r["dA"], r["w"], r["lrs"], r["ref"])
    print(f"stem_dgrad_route V={V}: n_seq = {n_seq}, constant = {c:.3e}")
    _assert_close(f"stem_dgrad_route {KIND[dt]} V={V} B={B} {shape}", "f32", r["got"], want, T * (c / C), layout="b v y x")


# the frame given from outside: the routed kernel's shapes and 16 x 64, whose 8 x 32 tiles divide the image exactly (every halo column of a
# tile seam is an image column, every halo column past the last tile lies outside); 17 x 50 has two tile columns and three tile rows
REF_SHAPES = dict(ROUTE_SHAPES, **{"16x64": (16, 64)})
REF_VS = (1, 2, 3, 9, 10, 12)
REF_CASES = []
for _dt in (F32, BF16, BF16X3):
    for _V in REF_VS:
        for _B in (1, 2):
            for _sh in REF_SHAPES:
                REF_CASES.append(pytest.param(_dt, _V, _B, _sh, id=f"{KIND[_dt].replace('x3', 'bf16x3')}-V{_V}-B{_B}-{_sh}"))


def _nan_tailed(n):
    return torch.full((n + 64,), float("nan"), device="cuda")


def _ref_case(dt, V, B, shape, every_variant=True):
    """hrn_kt_stem_dgrad_ref on _route_case's dA and w.  every_variant: three launches - both outputs, d_lrs alone (d_ref NULL), d_ref
    alone (d_lrs NULL) - and both NULL, which is refused; otherwise the both-outputs launch only.  -> the both-outputs run (the fp32
    outputs as the kernel wrote them, on the CPU), after the single-output runs were held to it bit for bit"""
    lib = _lib()
    H, W = REF_SHAPES[shape]
    nl, nr = B * V * H * W, B * H * W
    dA = Ten((B * V, H, W, 64), dt, rnd((B * V, H, W, 64), 72 + V, dt))
    w = torch.randn((64, 2, 3, 3), generator=torch.Generator().manual_seed(73)) * 0.3
    wd_, wt = w.cuda(), torch.empty(64 * 18, device="cuda")
    runs = []
    for want_lrs, want_ref in ((True, True), (True, False), (False, True))[:3 if every_variant else 1]:
        dl, dr = _nan_tailed(nl) if want_lrs else None, _nan_tailed(nr) if want_ref else None
        rc = lib.hrn_kt_stem_dgrad_ref(dt, dA.ptr, _p(wd_), _p(wt), _p(dl), _p(dr), B, V, H, W, _stream())
        assert rc == 0, (rc, lib.hrn_last_error())
        torch.cuda.synchronize()
        runs.append((None if dl is None else dl.cpu(), None if dr is None else dr.cpu()))
    assert dA.unchanged() and dA.guard_ok() and torch.equal(wd_.cpu(), w), "an input was written"
    dl0, dr0 = runs[0]
    out = dict(d_lrs=dl0[:nl].reshape(B, V, H, W), d_ref=dr0[:nr].reshape(B, H, W), dA=dA, w=w, wd=wd_)
    for t, n in ((dl0, nl), (dr0, nr)):
        assert bool(torch.isnan(t[n:]).all()), "a write past an output"
        assert not bool(torch.isnan(t[:n]).any()), "an element was not written"
    if not every_variant:
        return out
    dl1, dr2 = runs[1][0], runs[2][1]
    for t, n in ((dl1, nl), (dr2, nr)):
        assert bool(torch.isnan(t[n:]).all()), "a write past an output"
        assert not bool(torch.isnan(t[:n]).any()), "an element was not written"
    assert torch.equal(dl1[:nl].view(torch.int32), dl0[:nl].view(torch.int32)), "d_lrs alone differs from d_lrs of the both-outputs run"
    assert torch.equal(dr2[:nr].view(torch.int32), dr0[:nr].view(torch.int32)), "d_ref alone differs from d_ref of the both-outputs run"
    # neither output: refused before any launch (wt, the one buffer a launch could still write, stays as it was)
    wt_nan = torch.full((64 * 18,), float("nan"), device="cuda")
    rc = lib.hrn_kt_stem_dgrad_ref(dt, dA.ptr, _p(wd_), _p(wt_nan), None, None, B, V, H, W, _stream())
    msg = lib.hrn_last_error()
    torch.cuda.synchronize()
    assert rc == -2 and b"stem dgrad: neither d_lrs nor d_ref is wanted" in msg, (rc, msg)
    assert bool(torch.isnan(wt_nan).all()) and dA.unchanged()
    return out


def _ref_check(tag, r, B, V, **wrong):
    """both outputs of _ref_case against ref_stem_dgrad_ref under test_stem_dgrad_route's bound -> (error / bound of d_lrs, of d_ref)"""
    c = max(C, (9 * 64 + V) * 2.0 ** -24)
    d_lrs, T_lrs, d_ref, T_ref = ref_stem_dgrad_ref(r["dA"].val, r["w"].double(), B, V, **wrong)
    if wrong:
        return (_ratio("f32", r["d_lrs"].double(), d_lrs, T_lrs * (c / C))[0], _ratio("f32", r["d_ref"].double(), d_ref, T_ref * (c / C))[0])
    return (_assert_close(f"{tag} d_lrs", "f32", r["d_lrs"].double(), d_lrs, T_lrs * (c / C), layout="b v y x"),
            _assert_close(f"{tag} d_ref", "f32", r["d_ref"].double(), d_ref, T_ref * (c / C), layout="b y x"))


@pytest.mark.parametrize("dt,V,B,shape", REF_CASES)
def test_stem_dgrad_ref(dt, V, B, shape):
    """stem_dgrad_ref_kernel<ST>: d_lrs and d_ref per element, no element excluded, with test_stem_dgrad_route's bound for its reason: each
    view's two outputs are chains of 9 x 64 fused multiply-adds in fp32, and d_ref then adds the V views' channel 1: n_seq = 9 * 64 + V.
    The single-output launches are bit-equal to the both-outputs launch; no output wanted is -2"""
    r = _ref_case(dt, V, B, shape)
    n_seq = 9 * 64 + V
    print(f"stem_dgrad_ref V={V}: n_seq = {n_seq}, constant = {max(C, n_seq * 2.0 ** -24):.3e}")
    _ref_check(f"stem_dgrad_ref {KIND[dt]} V={V} B={B} {shape}", r, B, V)


@pytest.mark.parametrize("V", [9, 10], ids=["V9", "V10"])
@pytest.mark.parametrize("dt", DTS)
def test_stem_dgrad_ref_agrees_with_route(dt, V):
    """The copy against the original, bit for bit, on one dA and w: away from the routed view the routed kernel's d_lrs is the copy's, at
    the routed view it is float32(d_lrs + d_ref) - both kernels run the same fmaf chains in the same order, acc1 adds the views' channel 1
    in view order in both, and the routed kernel's last store is the one fp32 add keep + acc1"""
    lib = _lib()
    B, shape = 2, "15x33"
    H, W = REF_SHAPES[shape]
    r = _ref_case(dt, V, B, shape, every_variant=False)
    lrs, ref = route_inputs(B, V, H, W, 71 + V)
    ld, rd, wt = lrs.cuda(), ref.cuda(), torch.empty(64 * 18, device="cuda")
    routed = _nan_tailed(B * V * H * W)
    assert lib.hrn_kt_stem_dgrad_route(dt, r["dA"].ptr, _p(r["wd"]), _p(wt), _p(ld), _p(rd), _p(routed), B, V, H, W, _stream()) == 0
    torch.cuda.synchronize()
    got = routed.cpu()
    assert bool(torch.isnan(got[B * V * H * W:]).all()) and r["dA"].unchanged()
    got = got[:B * V * H * W].reshape(B, V, H, W)
    sel = ref_route_index(lrs, ref)[:, None]
    want = r["d_lrs"].scatter_add(1, sel, r["d_ref"][:, None])         # one fp32 add per pixel, at the routed view
    at_sel = torch.zeros((B, V, H, W), dtype=torch.bool).scatter_(1, sel, True)
    diff = got.view(torch.int32) != want.view(torch.int32)
    print(f"stem_dgrad_ref against stem_dgrad_route {KIND[dt]} V={V}: {int((diff & ~at_sel).sum())} of {int((~at_sel).sum())} elements differ away "
          f"from the routed view, {int((diff & at_sel).sum())} of {int(at_sel.sum())} at it; max |difference| {float((got - want).abs().max()):.3e}")
    assert int(sel.max()) > 0 and float(r["d_ref"].abs().max()) > 0
    assert not bool(diff.any())


@pytest.mark.parametrize("shape", ["2x3", "15x33", "17x50"])
@pytest.mark.parametrize("a", [0.25, 0.0, BF(-0.3)], ids=["pos", "zero", "neg"])
@pytest.mark.parametrize("dt", DTS)
def test_stem_pre(dt, a, shape):
    """stem_kernel<ST> through hrn_launch_stem_pre: nothing written with a positive slope (the launch is gated on the device), else the
    pre-activation in the storage of dt"""
    lib = _lib()
    H, W, M = STEM_SHAPES[shape]
    V = 3
    gen = torch.Generator().manual_seed(81 + H)
    x0, x1 = k16((M, H, W), gen), k16((-(-M // V), H, W), gen)
    w = torch.randn((64, 2, 3, 3), generator=gen) * 0.3
    b = (torch.randint(-(1 << 14), 1 << 14, (64,), generator=gen).double() / 65536.0).float()
    out = Ten((M, H, W, 64), dt)
    dev = [t.cuda() for t in (x0, x1, w, b)]
    sl = _dev1(a)
    assert lib.hrn_kt_stem_pre(dt, _p(dev[0]), H * W, _p(dev[1]), V, H * W, _p(dev[2]), _p(dev[3]), out.ptr, M, H, W, _p(sl), _stream()) == 0
    torch.cuda.synchronize()
    assert out.guard_ok() and all(torch.equal(d.cpu(), t) for d, t in zip(dev, (x0, x1, w, b)))
    if a > 0:
        assert out.unchanged(), "the gated launch wrote its output"
        return
    want, T = ref_stem_pre(x0.double(), x1.double(), V, w.double(), b.double())
    _assert_close(f"stem_pre {KIND[dt]} a={a} {shape}", KIND[dt], _nchw(out.value()), want, T)


# ----------------------------------------------------------------------------------------------------------- the decoder's backward
DEC_SHAPES = {"1x1": (1, 1, 1), "2x3": (2, 2, 3), "9x27": (3, 9, 27), "straddle": (5, 7, 33), "2.5cus": None}
DEC_GRADS = ["dwd", "dbd", "dad", "dwf", "dbf"]


def _dec_shape(shape):
    if DEC_SHAPES[shape] is not None:
        return DEC_SHAPES[shape]
    cus = _cus()
    W = 2 * cus + cus // 2 + 1          # between 2 and 3 times the CU count, not a multiple of it
    assert 2 * cus < W < 3 * cus and W % cus
    return 1, 1, W


def _decoder_case(S, shape, a, null=()):
    lib = _lib()
    N, H, W = _dec_shape(shape)
    fused, d_sr, wd, bd, wf = decoder_inputs(N, H, W, S, 900 + 10 * S + N)
    n_seq = S * S * -(-N * H * W // min(_cus(), N * H * W))       # the longest fp32 chain: dbd, S^2 positions per pixel of a workgroup
    assert n_seq <= 128, n_seq
    P = N * H * W * 64
    d_fused = torch.full((P + 64,), float("nan"), device="cuda")
    shapes = {"dwd": (64, 64, S, S), "dbd": (64,), "dad": (), "dwf": (64,), "dbf": ()}
    acc = {k: Acc(shapes[k], 90 + i, none=k in null) for i, k in enumerate(DEC_GRADS)}
    ins = [fused, d_sr, wd, bd, torch.tensor([a]), wf]
    dev = [t.cuda() for t in ins]
    sc = _scratch(lib)
    rc = lib.hrn_kt_decoder_bwd(S, *[_p(t) for t in dev], _p(d_fused), *[acc[k].ptr for k in DEC_GRADS], N, H, W, _p(sc), _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert all(torch.equal(d.cpu(), t) for d, t in zip(dev, ins)), "an input was written"
    got = d_fused.cpu()
    assert bool(torch.isnan(got[P:]).all()), "a write past d_fused"
    args = [t.double() for t in (fused, d_sr, wd, bd)] + [a, wf.double(), S]
    return dict(d_fused=got[:P].reshape(N, H, W, 64).double(), acc=acc, args=args)


def _decoder_check(tag, r):
    ref = ref_decoder_bwd(*r["args"])
    _assert_close(tag + " d_fused", "f32", r["d_fused"], *ref["d_fused"], layout="n y x c")
    for k in DEC_GRADS:
        r["acc"][k].check(f"{tag} {k}", *ref[k], layout="ci co ky kx" if k == "dwd" else "i")


@pytest.mark.parametrize("shape", list(DEC_SHAPES))
@pytest.mark.parametrize("S", [2, 3, 4], ids=["S2", "S3", "S4"])
def test_decoder_bwd(S, shape):
    """decoder_bwd_kernel<S, NP> (S = 4: two launches, the second adds) + finish: d_fused written, the five gradients accumulated.  The
    kernel branches on `up > 0` recomputed in fp32: the inputs make `up` exact (decoder_inputs), zeros included, so no element is masked"""
    a = DEC_SLOPES[(S + list(DEC_SHAPES).index(shape)) % 5]
    r = _decoder_case(S, shape, a)
    up = ref_decoder_up(*r["args"][:1], r["args"][2], r["args"][3], S)
    assert bool((up == 0).any()) and bool((up > 0).any()) and bool((up < 0).any())
    _decoder_check(f"decoder_bwd S={S} {shape} a={a}", r)


NULLS = {"no-dwd": ("dwd",), "no-dbd": ("dbd",), "no-dad": ("dad",), "no-dwf": ("dwf",), "no-dbf": ("dbf",), "no-dwd-dad": ("dwd", "dad"),
         "none": tuple(DEC_GRADS)}


@pytest.mark.parametrize("null", list(NULLS))
@pytest.mark.parametrize("S", [2, 3, 4], ids=["S2", "S3", "S4"])
def test_decoder_bwd_null(S, null):
    """the NULL gradients hrn_hrnet_backward_sel can hand over (frozen parameters): the others and d_fused still right"""
    a = DEC_SLOPES[(S + len(null)) % 5]
    _decoder_check(f"decoder_bwd S={S} {null} a={a}", _decoder_case(S, "straddle", a, null=NULLS[null]))


# ----------------------------------------------------------------------------------------------------------- planes <-> f32, bit-exact
PLANE_SIZES = {"8": 8, "8x257": 8 * 257, "cap": 8 * (8192 * 256 + 301)}        # "cap": n / 8 above the grid of 8192 x 256 threads


def _planes_case(two, n, v):
    """f32_to_planes of v -> (hi, lo or None) as int16, with the guards checked"""
    lib = _lib()
    src = v.cuda()
    out = torch.full((2 * n + GUARD,), SENT, dtype=torch.int16, device="cuda")
    assert lib.hrn_kt_f32_to_planes(_p(src), _p(out), 2 * n if two else 0, n, _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(src.cpu().view(torch.int32), v.view(torch.int32))
    o = out.cpu()
    assert bool((o[2 * n if two else n:] == SENT).all()), "a write past the planes (the one-plane form must not touch a second plane)"
    return o[:n], (o[n:2 * n] if two else None)


@pytest.mark.parametrize("size", list(PLANE_SIZES))
@pytest.mark.parametrize("two", [True, False], ids=["two", "one"])
def test_f32_to_planes(two, size):
    """f32_to_planes_kernel<LO>: hi = bf16(v) round to nearest even, lo = bf16(v - hi), bit for bit against torch"""
    n = PLANE_SIZES[size]
    v = split_inputs(n, 5 + n % 13)
    hi, lo = _planes_case(two, n, v)
    whi, wlo = ref_split_planes(v)
    bad = int((hi != whi.view(torch.int16)).sum())
    print(f"f32_to_planes {size}: {bad} hi words differ")
    assert bad == 0
    if two:
        bad = int((lo != wlo.view(torch.int16)).sum())
        print(f"f32_to_planes {size}: {bad} lo words differ")
        assert bad == 0


@pytest.mark.parametrize("size", list(PLANE_SIZES))
@pytest.mark.parametrize("two", [True, False], ids=["two", "one"])
def test_planes_to_f32(two, size):
    """planes_to_f32_kernel<LO>: out = float(hi) + float(lo) (one plane: float(hi)), bit for bit"""
    lib = _lib()
    n = PLANE_SIZES[size]
    g = torch.Generator().manual_seed(7 + n % 11)
    bits = torch.randint(-32768, 32768, (2 * n,), generator=g, dtype=torch.int32).to(torch.int16)
    expo = (bits.to(torch.int32) >> 7) & 0xFF
    bits[expo == 0xFF] = 0x3F80                 # no Inf / NaN
    bits[:8:3] = 0                              # +0 hi, and -0 below
    bits[1] = -32768
    planes = torch.cat([bits, torch.full((GUARD,), SENT, dtype=torch.int16)]).cuda()
    out = torch.full((n + 64,), float("nan"), device="cuda")
    assert lib.hrn_kt_planes_to_f32(_p(planes), 2 * n if two else 0, _p(out), n, _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(planes.cpu()[:2 * n], bits)
    got = out.cpu()
    assert bool(torch.isnan(got[n:]).all())
    hi, lo = bits[:n].view(torch.bfloat16).float(), bits[n:].view(torch.bfloat16).float()
    want = hi + lo if two else hi
    bad = int((got[:n].view(torch.int32) != want.view(torch.int32)).sum())
    print(f"planes_to_f32 {size} two={two}: {bad} words differ")
    assert bad == 0


# ----------------------------------------------------------------------------------------------------------- the median
def _median_case(B, V, H, W, seed):
    lib = _lib()
    lrs = torch.randint(-3, 4, (B, V, H, W), generator=torch.Generator().manual_seed(seed)).float()
    lrs[0, 0].view(-1)[::5] += 0.5              # not only integers
    ld = lrs.cuda()
    ref = torch.full((B * H * W + 64,), float("nan"), device="cuda")
    assert lib.hrn_kt_median(_p(ld), _p(ref), B, V, H, W, _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(ld.cpu(), lrs)
    got = ref.cpu()
    assert bool(torch.isnan(got[B * H * W:]).all())
    return lrs, got[:B * H * W].reshape(B, H, W)


@pytest.mark.parametrize("V", list(range(1, 13)), ids=[f"V{v}" for v in range(1, 13)])
def test_median(V):
    """median_kernel: the lower median of the first min(V, 9) views, ties and negative values, == torch.median"""
    lrs, got = _median_case(3, V, 17, 50, 100 + V)
    want = ref_median(lrs)
    bad = int((got != want).sum())
    print(f"median V={V}: {bad} pixels differ")
    assert bad == 0


def test_median_grid_cap():
    """B H W above the grid of 4096 x 256 threads: the grid-stride loop runs twice"""
    B, V, H, W = 2, 9, 725, 727
    assert B * H * W > 4096 * 256
    lrs, got = _median_case(B, V, H, W, 99)
    assert int((got != ref_median(lrs)).sum()) == 0


# ----------------------------------------------------------------------------------------------------------- negative controls
CONTROLS = ["prelu_zero_positive", "dslope_no_inv", "fuse_df_own_alpha", "fuse_scatter_swap_halves", "median_upper", "route_highest",
            "decoder_taps_transposed", "f32_to_planes_truncate", "ref_drops_last_view", "ref_channels_swapped"]


@pytest.mark.parametrize("control", CONTROLS)
def test_negative_control(control):
    """The comparison against a reference that is wrong in one way must FAIL on the same GPU output that passes against the right one."""
    if control in ("prelu_zero_positive", "dslope_no_inv"):
        a = 0.25
        r = _prelu_case(BF16, 64, 8193, a, False, None, 4321)
        g, dslope, Ts, _, _ = ref_prelu_bwd(r["dy"], r["src"], a)
        if control == "prelu_zero_positive":
            ok = _assert_close("prelu g (right reference)", "bf16", r["g"], g, g.abs(), layout="row c")
            bad = ref_prelu_bwd(r["dy"], r["src"], a, zero_is_positive=True)[0]
            worst, _ = _ratio("bf16", r["g"], bad, bad.abs())
        else:
            ok = r["dsl"].check("prelu dslope (right reference)", dslope, Ts, layout="")
            _, bad, Tb, _, _ = ref_prelu_bwd(r["dy"], r["src"], a, no_inv=True)
            s0 = r["dsl"].start.double().reshape(())
            worst, _ = _ratio("f32", r["dsl"].buf.double().cpu()[:1].reshape(()), s0 + bad, s0.abs() + Tb)
    elif control == "fuse_df_own_alpha":
        r = _fuse_df_case(BF16X3, 5, 3, "33x33", 1)
        want, T = ref_fuse_df(r["dsn"].val, r["al"], r["pair_last"], 1)
        ok = _assert_close("fuse_df (right reference)", "x3", r["df"].value(), want, T, layout="b v p c")
        bad, T = ref_fuse_df(r["dsn"].val, r["al"], r["pair_last"], 1, own_alpha=True)
        worst, _ = _ratio("x3", r["df"].value(), bad, T)
    elif control == "fuse_scatter_swap_halves":
        r = _fuse_scatter_case(BF16, 5, 3, "33x33", 1)
        want, T = ref_fuse_scatter(r["dsn"].val, r["dz"].val, 5, r["pair_last"], 1)
        ok = _assert_close("fuse_scatter (right reference)", "bf16", r["ds"].value(), want, T, layout="b v p c")
        bad, T = ref_fuse_scatter(r["dsn"].val, r["dz"].val, 5, r["pair_last"], 1, swap_halves=True)
        worst, _ = _ratio("bf16", r["ds"].value(), bad, T)
    elif control == "median_upper":
        lrs, got = _median_case(3, 8, 17, 50, 108)
        ok = float((got != ref_median(lrs)).sum())
        assert ok == 0
        worst = 1.0 + float((got != ref_median(lrs, upper=True)).sum())
    elif control == "route_highest":
        r = _route_case(BF16, 9, 2, "15x33")
        c = max(C, (9 * 64 + 9) * 2.0 ** -24)
        want, T = ref_stem_dgrad_route(r["dA"], r["w"], r["lrs"], r["ref"])
        ok = _assert_close("stem_dgrad_route (right reference)", "f32", r["got"], want, T * (c / C), layout="b v y x")
        bad, T = ref_stem_dgrad_route(r["dA"], r["w"], r["lrs"], r["ref"], highest=True)
        worst, _ = _ratio("f32", r["got"], bad, T * (c / C))
    elif control in ("ref_drops_last_view", "ref_channels_swapped"):
        B, V = 2, 10
        r = _ref_case(BF16, V, B, "15x33", every_variant=False)
        ok = max(_ref_check("stem_dgrad_ref (right reference)", r, B, V))
        if control == "ref_drops_last_view":        # the window of nine the median has and this sum has not: only d_ref can tell
            worst = _ref_check("", r, B, V, drop_last_view=True)[1]
        else:                                       # both outputs must tell
            worst = min(_ref_check("", r, B, V, swap_channels=True))
    elif control == "decoder_taps_transposed":
        r = _decoder_case(3, "9x27", 0.25)
        ref = ref_decoder_bwd(*r["args"])
        ok = _assert_close("decoder_bwd d_fused (right reference)", "f32", r["d_fused"], *ref["d_fused"], layout="n y x c")
        bad = ref_decoder_bwd(*r["args"], transpose_taps=True)
        worst, _ = _ratio("f32", r["d_fused"], *bad["d_fused"])
    else:
        n = 8 * 257
        v = split_inputs(n, 3)
        hi, _ = _planes_case(True, n, v)
        ok = float((hi != ref_split_planes(v)[0].view(torch.int16)).sum())
        assert ok == 0
        worst = 1.0 + float((hi != ref_split_planes(v, truncate_hi=True)[0].view(torch.int16)).sum())
    print(f"{control}: error / bound against the wrong reference {worst:.3e} (right one {ok:.3e})")
    assert worst > 1.0, f"{control}: the comparison does not tell the wrong reference from the right one"
