"""GPU (-m gpu): HRNet's kernels where offsets pass 2^31 bytes, 2^32 bytes and 2^31 elements, per element against torch CPU float64.

Every other per-element test stays below about 1 GiB per tensor.  Here the production launchers run, through the same hooks (kernel_test.h,
tests/kt.py), on tensors of 4 .. 16 GiB that are generated on the device from a seed (kernel_bounds.Big); only the checked images or rows
are copied to the host, and the references (kernel_refs.ref_*) and bounds (kernel_bounds: _assert_close with C, C_F32) are the ones of the
small-shape tests.  DESIGN.md section "Offsets past 2^31 and 2^32" holds the table of offset widths and limits this file exercises.

A  deep batch    many 64 x 64 images, and for every hook at least one case of ragged 33 x 50 images (no tile, strip or block size divides them): the 64-bit image base, the grid-stride loops, the row and segment
                 counters.  Checked: image 0, the last image, and for every crossing (byte 2^31, byte 2^32, element 2^31 of any tensor of the
                 launch) the image it falls into, or the two images it falls between (kernel_bounds.boundary_images).  The case id names
                 what the largest tensor crosses: 2^31el (which for 2-byte storage is 2^32 bytes as well) or, where fp32 / bf16x3 cannot
                 reach 2^31 elements inside 32 GiB, 2^32B only.  Kernels whose output is a sum over all images (conv_wgrad, stem_wgrad,
                 colsum, prelu_bwd_bias' db / dslope, decoder_bwd's five gradients) get tensors that are zero except at the checked images:
                 a kernel that mis-addresses a high image reads zeros or misses the data.
B  big frame     one image at each fast kernel's in-image limit, W a multiple of 32 and ragged, and the smallest image the guard refuses:
                 three strips (top, middle, bottom; tile-aligned, >= 24 rows, real neighbour rows as halo) per element.  The bf16
                 convolutions must then run on conv3x3.hip's general kernel (read from the profiler's family names) and be right;
                 v6x3, wgrad_x3, the MFMA stem, stem_dgrad_route and stem_dgrad_ref must return -2 with their message and write nothing.
                 The masked composite (hrn_masked_composite, f32 only) has both regimes too: a deep batch of 32-view samples, and one
                 sample whose 32 views of 8200 x 8190 pass 2^31 elements; bit for bit against its numpy restatement.
C  whole network HRNet.forward in bf16 with B V H W 64 > 2^31 elements (B = 33, V = 16, 256 x 256): samples 0 and B - 1 bit-identical to their
                 forward alone.
Negative controls: the comparison fails when the reference is taken from the image a 32-bit base would address (m - 2^32 / image bytes).

Every tensor of a test is registered with the `pool` fixture, which frees it whatever the outcome, prints the test's peak device memory
and holds it to 32 GiB."""
import gc

import pytest
import torch

import kernel_refs as K
from kernel_bounds import (C, C_F32, GIB, Acc, Big, _assert_close, _bits_equal, _nan_out, _nchw, _need, _Pool, _ratio, _sum64, boundary_images,
                           crossed)
from kt import BF16, BF16X3, F32, _launches, _p, _stream, lib as _lib

pytestmark = pytest.mark.gpu

DT = {"bf16": BF16, "bf16x3": BF16X3, "f32": F32}
DTN = ["bf16", "bf16x3", "f32"]
KIND = {F32: "f32", BF16: "bf16", BF16X3: "x3"}
ES = {F32: 4, BF16: 2, BF16X3: 2}                # bytes per element of one plane
V2, LEVEL = 2, dict(n=2, half=1, pair_last=1)      # every view stack of this file: two views per sample = one pair, pair_last = 1
SHAPES = {"64x64": (64, 64), "33x50": (33, 50)}
# every storage at 64 x 64, and the ragged images in bf16
DT_SHAPES = [(d, "64x64") for d in DTN] + [("bf16", "33x50")]
DT_SHAPE_IDS = [f"{d}-{s}-2^31el" for d, s in DT_SHAPES]


def _top(dt, cross):
    """elements a plane needs to cross what the id says"""
    return {"2^31el": 1 << 31, "2^32B": (1 << 32) // ES[dt]}[cross]


def _count(dt, cross, per):
    """images of `per` elements so that the tensor crosses `cross`, with one whole image behind the crossing"""
    return _top(dt, cross) // per + 2


@pytest.fixture
def pool(request):
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    p = _Pool()
    yield p
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    p.free()
    gc.collect()
    torch.cuda.empty_cache()
    print(f"\nPEAK {request.node.name}: {peak / GIB:.2f} GiB")
    assert peak <= 32 * GIB, f"{peak / GIB:.1f} GiB held at once"


def _scratch(pool):
    return pool.keep(torch.empty(_lib().hrn_kt_wgrad_scratch_bytes(), dtype=torch.uint8, device="cuda"))


def _dev1(a):
    return torch.tensor([a], dtype=torch.float32, device="cuda")


def _images(*tensors):
    """the union of the boundary images of (M, elements per image, plane element size) triples"""
    out = set()
    for M, per, es in tensors:
        out |= set(boundary_images(M, per, es))
    return sorted(out)


def _says(tag, cross, *tensors):
    """print what each tensor crosses; the largest must cross what the case id says"""
    got = [crossed(t.n, t.esize) for t in tensors]
    print(f"{tag}: " + ", ".join(f"{t.n * t.esize / GIB:.2f} GiB per plane {c}" for t, c in zip(tensors, got)))
    assert any(cross in c for c in got) and all("2^31B" in c for c in got), (tag, cross, got)


# ----------------------------------------------------------------------------------------------------------- the convolutions
# layer: (cin, cout, res_mode, in_pair, slot output)
CONV = {
    "enc": (64, 64, 1, False, False),            # encoder conv 2: residual in place (bf16: conv3x3_r64<true>)
    "plain64": (64, 64, 0, False, False),        # encoder conv 1 (bf16: conv3x3_r64<false>, the fast halo form)
    "pairres": (128, 128, 2, True, False),       # pair gather in + pair residual
    "alpha": (128, 64, 3, False, "stack"),       # fusion output conv: alpha residual in place into the stack slot
    "up": (64, 128, 0, False, False),            # the data gradient of a 128 -> 64 layer as a convolution
}


def _conv_weights(dt, cin, cout, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn((cout, cin, 3, 3), generator=g) * (0.05 if cin == 64 else 0.035)
    bias = torch.randn(cout, generator=g) * 0.1
    if dt == BF16:
        w, bias = w.to(torch.bfloat16).float(), bias.to(torch.bfloat16).float()
    return w, bias


def _pad_rows(t, m, y0, y1, H, v=None):
    """rows y0 - 1 .. y1 of image m (view v) as the convolution reads them for output rows y0 .. y1: real neighbours, zeros outside"""
    a, b = max(0, y0 - 1), min(H, y1 + 1)
    r = t.rows(m, a, b, v)
    z = lambda k: torch.zeros((k,) + tuple(r.shape[1:]), dtype=torch.float64)
    return torch.cat([z(a - (y0 - 1)), r, z(y1 + 1 - b)])


def _conv_case(pool, layer, dt, route, M, H, W, regions, seed, slope=0.25, also=(), expect_rc=0):
    """Launch `layer` in storage dt on M images of H x W through hrn_kt_conv3x3_epi.  regions: (m, y0, y1) row ranges to check; their
    inputs (and those of `also`) are copied to the host before the launch, which may write in place.
    -> dict: got(region), ref(region, src=None: the region the reference's inputs are taken from), fams, the tensors"""
    cin, cout, res_mode, in_pair, slot = CONV[layer]
    lib = _lib()
    w, bias = _conv_weights(dt, cin, cout, seed)
    w64, b64 = w.double(), bias.double()
    wd, bd, sd = w.cuda(), bias.cuda(), _dev1(slope)
    pk = torch.empty(cin * cout * 9 * (1 if dt == BF16 else 2), dtype=torch.bfloat16, device="cuda")
    assert lib.hrn_kt_conv_pack(dt, cin, cout, _p(wd), _p(pk), _stream()) == 0
    uses_stack = bool(in_pair or res_mode in (2, 3) or slot)
    stack = pool.big(M, (V2, H, W, 64), dt, "rand", seed + 1, apart=True) if uses_stack else None
    inp = None if in_pair else pool.big(M, (H, W, cin), dt, "rand", seed + 2, apart=True)
    if slot:
        out = stack
    elif res_mode == 1:
        out = pool.big(M, (H, W, cout), dt, "rand", seed + 3, apart=True)        # in place: out == res
    else:
        out = pool.big(M, (H, W, cout), dt, "sent", apart=True)
    alph = K.conv_alphas(M, V2, "full" if dt == F32 else "exact") if res_mode == 3 else None
    ad = alph.cuda() if alph is not None else None
    res_ptr, res_lo, res_vs = None, 0, 0
    if res_mode == 1:
        res_ptr, res_lo = out.ptr, out.lo_off
    elif res_mode == 3:
        res_ptr, res_lo, res_vs = stack.ptr, stack.lo_off, V2

    def snap(m, y0, y1):
        s = {}
        if inp is not None:
            s["x"] = _pad_rows(inp, m, y0, y1, H)
        if stack is not None:
            s["st"] = torch.stack([_pad_rows(stack, m, y0, y1, H, v) for v in range(V2)])
        if res_mode == 1:
            s["res"] = out.rows(m, y0, y1)
        return s

    snaps = {r: snap(*r) for r in list(regions) + list(also)}
    sums = [(t, t.checksum()) for t in (inp, stack) if t is not None and t is not out]
    pair_h = 1 if (in_pair or res_mode == 2) else 0
    fams, rc = _launches(lambda: lib.hrn_kt_conv3x3_epi(
        dt, route, cin, cout, None if in_pair else inp.ptr, stack.ptr if stack is not None else None, pair_h, 1, V2 if uses_stack else 0,
        _p(pk), _p(bd), _p(sd), res_ptr, res_mode, res_vs, _p(ad), V2 if ad is not None else 0, out.ptr, 1 if slot else 0,
        V2 if slot else 0, 0 if in_pair else inp.lo_off, stack.lo_off if stack is not None else 0, out.lo_off, res_lo, M, H, W, _stream()))
    assert rc == expect_rc, (rc, lib.hrn_last_error())
    for t, c in sums:
        assert t.checksum() == c, "the launch wrote one of its inputs"
    for t in (inp, stack, out):
        assert t is None or t.guards_intact(), "a write past a tensor"

    def got(region):
        m, y0, y1 = region
        if slot:        # slot 1 (the partner) is not the launch's to write
            assert torch.equal(stack.rows(m, y0, y1, 1), snaps[region]["st"][1][1:-1]), "the launch wrote a slot it does not own"
        return out.rows(m, y0, y1, 0 if slot else None).permute(2, 0, 1)

    def ref(region, src=None):
        s = snaps[src or region]
        m, y0, y1 = src or region
        xpad = torch.cat([s["st"][0], s["st"][1]], -1) if in_pair else s["x"]
        if y0 == 0 and y1 == H:         # a whole image: the reference of the small-shape tests
            want, T = K.ref_conv_epi(x=xpad[1:-1][None], w=w64, b=b64, slope=slope, res_mode=res_mode, res=s["res"][None] if res_mode == 1 else None,
                                     stack=s["st"][:, 1:-1][None] if "st" in s else None, geo=LEVEL, alph=alph[m:m + 1] if alph is not None else None)
            return want[0], T[0]
        res = {0: None, 1: s.get("res"), 2: torch.cat([s["st"][0], s["st"][1]], -1)[1:-1] if "st" in s else None,
               3: s["st"][0][1:-1] if "st" in s else None}[res_mode]
        return K.ref_conv_rows(xpad, w64, b64, slope, res_mode, res, float(alph[m, 1]) if alph is not None else 1.0)

    return dict(got=got, ref=ref, fams=fams, out=out, inp=inp, stack=stack, c=C_F32 if dt == F32 else C, kind=KIND[dt])


def _conv_sizes(layer, dt, cross, H, W):
    """-> M, the (M, per, esize) triples of the launch's tensors, GiB needed"""
    cin, cout, res_mode, in_pair, slot = CONV[layer]
    pers = ([] if in_pair else [H * W * cin]) + ([H * W * 128] if (in_pair or res_mode in (2, 3) or slot) else []) + ([] if slot else [H * W * cout])
    M = _count(dt, cross, min(pers))
    planes = 2 if dt == BF16X3 else 1
    return M, [(M, p, ES[dt]) for p in pers], sum(M * p * ES[dt] * planes for p in pers) / GIB + 2


CONV_A = [("enc", "bf16", 0, "64x64", "2^31el"), ("enc", "bf16", 0, "33x50", "2^31el"), ("enc", "bf16", 1, "64x64", "2^31el"),
          ("enc", "bf16x3", 0, "64x64", "2^31el"), ("enc", "f32", 0, "64x64", "2^31el"), ("enc", "f32", 1, "64x64", "2^32B"),
          ("pairres", "bf16", 0, "64x64", "2^31el"), ("pairres", "bf16x3", 0, "64x64", "2^31el"), ("pairres", "f32", 0, "64x64", "2^31el"),
          ("alpha", "bf16", 0, "64x64", "2^31el"), ("alpha", "bf16x3", 0, "64x64", "2^31el"), ("alpha", "f32", 0, "64x64", "2^31el"),
          # ragged tiles of conv3x3_v6 / v6x3 at a high image base: the marked store lanes, the clamped residual fetch of res_mode 2 and 3
          ("pairres", "bf16", 0, "33x50", "2^31el"), ("alpha", "bf16x3", 0, "33x50", "2^31el")]


@pytest.mark.parametrize("layer,dtn,route,shape,cross", CONV_A, ids=[f"{a}-{b}-route{c}-{d}-{e}" for a, b, c, d, e in CONV_A])
def test_conv_deep_batch(pool, layer, dtn, route, shape, cross):
    """hrn_kt_conv3x3_epi, regime A: conv3x3_r64<true> / conv3x3_v6 / conv3x3_v6x3 / conv3x3_kernel<F32> on route 0, conv3x3_kernel<BF16 |
    F32> on route 1"""
    dt, (H, W) = DT[dtn], SHAPES[shape]
    M, tensors, need = _conv_sizes(layer, dt, cross, H, W)
    _need(need)
    imgs = _images(*tensors)
    tag = f"conv {layer} {dtn} route {route} {shape} M={M}"
    r = _conv_case(pool, layer, dt, route, M, H, W, [(m, 0, H) for m in imgs], 500 + len(layer))
    _says(tag, cross, *[t for t in (r["inp"], r["stack"], r["out"]) if t is not None])
    for m in imgs:
        want, T = r["ref"]((m, 0, H))
        _assert_close(f"{tag} image {m}", r["kind"], r["got"]((m, 0, H)), want, T, layout="c y x", c=r["c"])


# ----------------------------------------------------------------------------------------------------------- data gradient
DGRAD = {"64x64+res": (64, 64, True), "128x64": (128, 64, False)}


DGRAD_CASES = [(l, d, "64x64") for l in DGRAD for d in DTN] + [("128x64", "bf16", "33x50"), ("64x64+res", "bf16x3", "33x50")]


@pytest.mark.parametrize("layer,dtn,shape", DGRAD_CASES, ids=[f"{a}-{b}-{c}-2^31el" for a, b, c in DGRAD_CASES])
def test_conv_dgrad_deep_batch(pool, layer, dtn, shape):
    """hrn_kt_conv_dgrad: dx = conv3x3(g, W^T flipped) (+ res) of a cin -> cout layer, every tensor past 2^31 elements (the lo planes
    directly behind the hi planes); 128 -> 64 is the 64 -> 128 convolution of conv3x3_v6 / v6x3"""
    dt, (cin, cout, with_res), (H, W) = DT[dtn], DGRAD[layer], SHAPES[shape]
    lib = _lib()
    M = _count(dt, "2^31el", H * W * min(cin, cout))
    planes = 2 if dt == BF16X3 else 1
    _need(M * H * W * (cout + cin * (2 if with_res else 1)) * ES[dt] * planes / GIB + 2)
    imgs = _images((M, H * W * cout, ES[dt]), (M, H * W * cin, ES[dt]))
    w = torch.randn((cout, cin, 3, 3), generator=torch.Generator().manual_seed(71)) * 0.05
    if dt == BF16:
        w = w.to(torch.bfloat16).float()
    g = pool.big(M, (H, W, cout), dt, "rand", 72)
    res = pool.big(M, (H, W, cin), dt, "rand", 73) if with_res else None
    dx = pool.big(M, (H, W, cin), dt, "sent")
    wd, wt, wtp, zb = w.cuda(), torch.empty(cin * cout * 9, device="cuda"), torch.empty(cin * cout * 9, device="cuda"), torch.zeros(128, device="cuda")
    sums = [(t, t.checksum()) for t in (g, res) if t is not None]
    rc = lib.hrn_kt_conv_dgrad(dt, cin, cout, _p(wd), g.ptr, dx.ptr, res.ptr if res is not None else None, M, H, W, _p(wt), _p(wtp), _p(zb), _stream())
    assert rc == 0, (rc, lib.hrn_last_error())
    torch.cuda.synchronize()
    assert all(t.checksum() == c for t, c in sums) and dx.guards_intact()
    tag = f"conv_dgrad {layer} {dtn} {shape} M={M}"
    _says(tag, "2^31el", g, dx)
    for m in imgs:
        want, T = K.ref_conv_dgrad(g.img(m)[None], w.double(), res.img(m)[None] if res is not None else None)
        _assert_close(f"{tag} image {m}", KIND[dt], _nchw(dx.img(m)[None]), want, T, c=C_F32 if dt == F32 else C)


# ----------------------------------------------------------------------------------------------------------- weight gradient
WGRAD_CASES = [(p, d, "64x64") for p in (False, True) for d in DTN] + [(False, "bf16", "33x50"), (True, "bf16x3", "33x50")]


@pytest.mark.parametrize("pair,dtn,shape", WGRAD_CASES, ids=[f"{'pair' if a else 'plain'}-{b}-{c}-2^31el" for a, b, c in WGRAD_CASES])
def test_conv_wgrad_deep_batch(pool, pair, dtn, shape):
    """hrn_kt_conv_wgrad (conv_wgrad_x3_kernel<false | true>, conv_wgrad_kernel): x and g are zero except at the checked images"""
    dt, (H, W) = DT[dtn], SHAPES[shape]
    lib = _lib()
    cin, cout = (128, 128) if pair else (64, 64)
    M = _count(dt, "2^31el", H * W * cout)
    _need(M * H * W * (cin + cout) * ES[dt] * (2 if dt == BF16X3 else 1) / GIB + 2)
    imgs = _images((M, H * W * cin, ES[dt]), (M, H * W * cout, ES[dt]))
    x = pool.big(M, (V2, H, W, 64) if pair else (H, W, cin), dt, "zero", 81)
    g = pool.big(M, (H, W, cout), dt, "zero", 82)
    x.rand_images(imgs)
    g.rand_images(imgs)
    dw = Acc((cout, cin, 3, 3), 83)
    sc = _scratch(pool)
    sums = [(t, t.checksum()) for t in (x, g)]
    rc = lib.hrn_kt_conv_wgrad(dt, None if pair else x.ptr, x.ptr if pair else None, 1 if pair else 0, 1 if pair else 0, V2 if pair else 0, g.ptr,
                               M, H, W, cin, cout, dw.ptr, _p(sc), _stream())
    assert rc == 0, (rc, lib.hrn_last_error())
    torch.cuda.synchronize()
    assert all(t.checksum() == c for t, c in sums), "an input (or the sentinels behind it) was written"
    tag = f"conv_wgrad {'pair' if pair else 'plain'} {dtn} {shape} M={M} images {imgs}"
    _says(tag, "2^31el", x, g)
    xs = torch.stack([torch.cat(list(x.img(m)), -1) if pair else x.img(m) for m in imgs])
    gs = torch.stack([g.img(m) for m in imgs])
    want, T = K.ref_conv_wgrad(xs, gs)
    dw.check(tag, want, T, layout="co ci ky kx")


# ----------------------------------------------------------------------------------------------------------- the stem
def _k16_dev(shape, gen):
    """values k / 2^16, 0 <= k < 2^16, on the device (16 significant bits: hi + lo of the stem's input split is exact)"""
    return torch.randint(0, 1 << 16, shape, device="cuda", generator=gen).float() / 65536.0


def _stem_inputs(M, H, W, rep1, seed, dt):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    x0, x1 = _k16_dev((M, H, W), gen), _k16_dev((-(-M // rep1), H, W), gen)
    g = torch.Generator().manual_seed(seed)
    w = torch.randn((64, 2, 3, 3), generator=g) * 0.3
    if dt == BF16:
        w = w.to(torch.bfloat16).float()
    bias = (torch.randint(-(1 << 14), 1 << 14, (64,), generator=g).double() / 65536.0).float()
    return x0, x1, w, bias


STEM_A = [("mfma", "bf16", "64x64"), ("mfma", "bf16", "33x50"), ("mfma", "bf16x3", "64x64"), ("sub", "bf16", "64x64"), ("valu", "f32", "64x64")]


@pytest.mark.parametrize("mode,dtn,shape", STEM_A, ids=[f"{a}-{b}-{c}-2^31el" for a, b, c in STEM_A])
def test_stem_deep_batch(pool, mode, dtn, shape):
    """hrn_kt_stem: stem_mfma_kernel<false | true> (sub NULL), the VALU stem_kernel<BF16> with `sub`, stem_kernel<F32>; the output passes
    2^31 elements, the segment / patch counters run to M H ceil(W / 32)"""
    dt, (H, W), rep1, slope = DT[dtn], SHAPES[shape], 3, 0.25
    lib = _lib()
    M = _count(dt, "2^31el", H * W * 64)
    _need(M * H * W * 64 * ES[dt] * (2 if dt == BF16X3 else 1) / GIB + 2)
    imgs = boundary_images(M, H * W * 64, ES[dt])
    x0, x1, w, bias = _stem_inputs(M, H, W, rep1, 91, dt)
    sub = _k16_dev((M, 2), torch.Generator(device="cuda").manual_seed(92)) if mode == "sub" else None
    out = pool.big(M, (H, W, 64), dt, "sent", apart=True)
    wd, bd, sd = w.cuda(), bias.cuda(), _dev1(slope)
    rc = lib.hrn_kt_stem(dt, _p(x0), H * W, _p(x1), rep1, H * W, _p(sub), _p(wd), _p(bd), _p(sd), out.ptr, out.lo_off, M, H, W, _stream())
    assert rc == 0, (rc, lib.hrn_last_error())
    torch.cuda.synchronize()
    assert out.guards_intact()
    tag = f"stem {mode} {dtn} {shape} M={M}"
    _says(tag, "2^31el", out)
    for m in imgs:
        want, T = K.ref_stem_fwd(x0[m:m + 1].cpu().double(), x1[m // rep1:m // rep1 + 1].cpu().double(), 1,
                                 sub[m:m + 1].cpu().double() if sub is not None else None, w.double(), bias.double(), slope, 0, 1)
        _assert_close(f"{tag} image {m}", KIND[dt], _nchw(out.img(m)[None]), want, T, c=C_F32 if dt == F32 else C)


@pytest.mark.parametrize("dtn,shape", DT_SHAPES, ids=DT_SHAPE_IDS)
def test_stem_pre_deep_batch(pool, dtn, shape):
    """hrn_kt_stem_pre with a slope of 0: the gated launch runs and writes the pre-activation (bf16x3: lo plane directly behind hi)"""
    dt, (H, W), rep1 = DT[dtn], SHAPES[shape], 3
    lib = _lib()
    M = _count(dt, "2^31el", H * W * 64)
    _need(M * H * W * 64 * ES[dt] * (2 if dt == BF16X3 else 1) / GIB + 2)
    imgs = boundary_images(M, H * W * 64, ES[dt])
    x0, x1, w, bias = _stem_inputs(M, H, W, rep1, 95, dt)
    out = pool.big(M, (H, W, 64), dt, "sent")
    wd, bd, sd = w.cuda(), bias.cuda(), _dev1(0.0)
    rc = lib.hrn_kt_stem_pre(dt, _p(x0), H * W, _p(x1), rep1, H * W, _p(wd), _p(bd), out.ptr, M, H, W, _p(sd), _stream())
    assert rc == 0, (rc, lib.hrn_last_error())
    torch.cuda.synchronize()
    assert out.guards_intact()
    _says(f"stem_pre {dtn} M={M}", "2^31el", out)
    for m in imgs:
        want, T = K.ref_stem_pre(x0[m:m + 1].cpu().double(), x1[m // rep1:m // rep1 + 1].cpu().double(), 1, w.double(), bias.double())
        _assert_close(f"stem_pre {dtn} image {m}", KIND[dt], _nchw(out.img(m)[None]), want, T)


@pytest.mark.parametrize("dtn,shape", DT_SHAPES, ids=DT_SHAPE_IDS)
def test_stem_wgrad_deep_batch(pool, dtn, shape):
    """hrn_kt_stem_wgrad (sub NULL): g is zero except at the checked images, so a workgroup adds at most a few non-zero tiles in fp32"""
    dt, (H, W), rep1 = DT[dtn], SHAPES[shape], 3
    lib = _lib()
    M = _count(dt, "2^31el", H * W * 64)
    _need(M * H * W * 64 * ES[dt] * (2 if dt == BF16X3 else 1) / GIB + 2)
    imgs = boundary_images(M, H * W * 64, ES[dt])
    x0, x1, _, _ = _stem_inputs(M, H, W, rep1, 97, dt)
    g = pool.big(M, (H, W, 64), dt, "zero", 98)
    g.rand_images(imgs)
    dw = Acc((64, 2, 3, 3), 99)
    sc = _scratch(pool)
    c0 = g.checksum()
    rc = lib.hrn_kt_stem_wgrad(dt, _p(x0), H * W, _p(x1), rep1, H * W, None, g.ptr, M, H, W, dw.ptr, _p(sc), _stream())
    assert rc == 0, (rc, lib.hrn_last_error())
    torch.cuda.synchronize()
    assert g.checksum() == c0
    _says(f"stem_wgrad {dtn} M={M}", "2^31el", g)
    xs0 = torch.cat([x0[m:m + 1] for m in imgs]).cpu().double()
    xs1 = torch.cat([x1[m // rep1:m // rep1 + 1] for m in imgs]).cpu().double()
    want, T = K.ref_stem_wgrad(xs0, xs1, 1, None, torch.stack([g.img(m) for m in imgs]))
    dw.check(f"stem_wgrad {dtn} M={M} images {imgs}", want, T, layout="co c ky kx")


@pytest.mark.parametrize("dtn,shape", DT_SHAPES, ids=DT_SHAPE_IDS)
def test_stem_dgrad_route_deep_batch(pool, dtn, shape):
    """hrn_kt_stem_dgrad_route: dA [B V][H][W][64] past 2^31 elements; the bound is test_stem_dgrad_route's (n_seq = 9 x 64 + V fp32 terms)"""
    dt, (H, W), V = DT[dtn], SHAPES[shape], 2
    lib = _lib()
    M = _count(dt, "2^31el", H * W * 64)
    M += M % V
    B = M // V
    _need(M * H * W * 64 * ES[dt] * (2 if dt == BF16X3 else 1) / GIB + 2)
    bs = sorted({m // V for m in boundary_images(M, H * W * 64, ES[dt])})
    dA = pool.big(M, (H, W, 64), dt, "rand", 101)
    lrs = torch.randint(0, 2, (B, V, H, W), device="cuda", generator=torch.Generator(device="cuda").manual_seed(102)).float()
    ref = torch.median(lrs, 1).values.contiguous()
    w = torch.randn((64, 2, 3, 3), generator=torch.Generator().manual_seed(103)) * 0.3
    d_lrs = pool.keep(torch.full((B * V * H * W + 64,), float("nan"), device="cuda"))
    wd, wt = w.cuda(), torch.empty(64 * 18, device="cuda")
    c0 = dA.checksum()
    rc = lib.hrn_kt_stem_dgrad_route(dt, dA.ptr, _p(wd), _p(wt), _p(lrs), _p(ref), _p(d_lrs), B, V, H, W, _stream())
    assert rc == 0, (rc, lib.hrn_last_error())
    torch.cuda.synchronize()
    assert dA.checksum() == c0 and bool(torch.isnan(d_lrs[B * V * H * W:]).all())
    _says(f"stem_dgrad_route {dtn} B={B}", "2^31el", dA)
    c = max(C, (9 * 64 + V) * 2.0 ** -24)
    for b in bs:
        dAb = torch.stack([dA.img(b * V + v) for v in range(V)])
        want, T = K.ref_stem_dgrad_route(dAb, w.double(), lrs[b:b + 1].cpu(), ref[b:b + 1].cpu())
        got = d_lrs[b * V * H * W:(b + 1) * V * H * W].cpu().double().reshape(1, V, H, W)
        _assert_close(f"stem_dgrad_route {dtn} sample {b}", "f32", got, want, T * (c / C), layout="b v y x")


@pytest.mark.parametrize("dtn,shape", DT_SHAPES, ids=DT_SHAPE_IDS)
def test_stem_dgrad_ref_deep_batch(pool, dtn, shape):
    """hrn_kt_stem_dgrad_ref (the frame given from outside: no routing, d_lrs and d_ref both wanted): dA [B V][H][W][64] past 2^31 elements;
    the bound is test_stem_dgrad_ref's (n_seq = 9 x 64 + V fp32 terms), no element excluded"""
    dt, (H, W), V = DT[dtn], SHAPES[shape], 2
    lib = _lib()
    M = _count(dt, "2^31el", H * W * 64)
    M += M % V
    B = M // V
    _need(M * H * W * 64 * ES[dt] * (2 if dt == BF16X3 else 1) / GIB + 2)
    bs = sorted({m // V for m in boundary_images(M, H * W * 64, ES[dt])})
    dA = pool.big(M, (H, W, 64), dt, "rand", 105)
    w = torch.randn((64, 2, 3, 3), generator=torch.Generator().manual_seed(106)) * 0.3
    d_lrs = pool.keep(torch.full((B * V * H * W + 64,), float("nan"), device="cuda"))
    d_ref = pool.keep(torch.full((B * H * W + 64,), float("nan"), device="cuda"))
    wd, wt = w.cuda(), torch.empty(64 * 18, device="cuda")
    c0 = dA.checksum()
    rc = lib.hrn_kt_stem_dgrad_ref(dt, dA.ptr, _p(wd), _p(wt), _p(d_lrs), _p(d_ref), B, V, H, W, _stream())
    assert rc == 0, (rc, lib.hrn_last_error())
    torch.cuda.synchronize()
    assert dA.checksum() == c0 and bool(torch.isnan(d_lrs[B * V * H * W:]).all()) and bool(torch.isnan(d_ref[B * H * W:]).all())
    _says(f"stem_dgrad_ref {dtn} B={B}", "2^31el", dA)
    c = max(C, (9 * 64 + V) * 2.0 ** -24)
    for b in bs:
        dAb = torch.stack([dA.img(b * V + v) for v in range(V)])
        want_l, T_l, want_r, T_r = K.ref_stem_dgrad_ref(dAb, w.double(), 1, V)
        got_l = d_lrs[b * V * H * W:(b + 1) * V * H * W].cpu().double().reshape(1, V, H, W)
        got_r = d_ref[b * H * W:(b + 1) * H * W].cpu().double().reshape(1, H, W)
        _assert_close(f"stem_dgrad_ref {dtn} sample {b} d_lrs", "f32", got_l, want_l, T_l * (c / C), layout="b v y x")
        _assert_close(f"stem_dgrad_ref {dtn} sample {b} d_ref", "f32", got_r, want_r, T_r * (c / C), layout="b y x")


# ----------------------------------------------------------------------------------------------------------- the decoder
DEC_CASES = [(2, d, "64x64") for d in DTN] + [(2, "bf16", "33x50")] + [(4, d, "64x64") for d in DTN]


@pytest.mark.parametrize("S,dtn,shape", DEC_CASES, ids=[f"S{a}-{b}-{c}-{'fused-2^31el' if a == 2 else 'sr-2^32B'}" for a, b, c in DEC_CASES])
def test_decoder_deep_batch(pool, S, dtn, shape):
    """hrn_kt_decoder: S = 2 with `fused` past 2^31 elements, S = 4 with the SR planes past 2^32 bytes (and `fused` then twice as far)"""
    dt, (H, W) = DT[dtn], SHAPES[shape]
    lib = _lib()
    N = _count(dt, "2^31el", H * W * 64) if S == 2 else (1 << 32) // (S * S * H * W * 4) + 2
    _need((N * H * W * 64 * ES[dt] * (2 if dt == BF16X3 else 1) + N * S * S * H * W * 4) / GIB + 2)
    imgs = _images((N, H * W * 64, ES[dt]), (N, S * S * H * W, 4))
    g = torch.Generator().manual_seed(110 + S)
    wd_ = torch.randn((64, 64, S, S), generator=g) * 0.05
    if dt == BF16:
        wd_ = wd_.to(torch.bfloat16).float()
    bd_, wf, bf, slope = torch.randn(64, generator=g) * 0.1, torch.randn(64, generator=g) * 0.2, torch.randn(1, generator=g) * 0.1, 0.25
    fused = pool.big(N, (H, W, 64), dt, "rand", 111, apart=True)
    sr = pool.keep(torch.full(((N + 1) * S * H * S * W,), float("nan"), device="cuda"))
    wpk = torch.empty(64 * 64 * S * S, dtype=torch.float32, device="cuda")
    dev = [t.cuda() for t in (wd_, bd_, wf, bf)] + [_dev1(slope)]
    c0 = fused.checksum()
    rc = lib.hrn_kt_decoder(dt, S, fused.ptr, fused.lo_off, _p(dev[0]), _p(wpk), _p(dev[1]), _p(dev[4]), _p(dev[2]), _p(dev[3]), _p(sr), N, H, W, _stream())
    assert rc == 0, (rc, lib.hrn_last_error())
    torch.cuda.synchronize()
    per = S * H * S * W
    assert fused.checksum() == c0 and bool(torch.isnan(sr[N * per:]).all()), "the decoder wrote its input or past the SR output"
    tag = f"decoder {dtn} S={S} {shape} N={N}"
    print(f"{tag}: fused {crossed(fused.n, fused.esize)}, sr {crossed(N * per, 4)}")
    assert "2^31el" in crossed(fused.n, fused.esize) if S == 2 else "2^32B" in crossed(N * per, 4)
    for m in imgs:
        want, T = K.ref_decoder_fwd(fused.img(m)[None], wd_.double(), bd_.double(), slope, wf.double(), bf.double(), S)
        got = sr[m * per:(m + 1) * per].cpu().double().reshape(1, S * H, S * W)
        _assert_close(f"{tag} image {m}", "f32", got, want, T, layout="n y x", c=C_F32 if dt == F32 else C)


@pytest.mark.parametrize("S,shape", [(2, "64x64"), (4, "64x64"), (2, "33x50")], ids=["S2-64x64-2^32B", "S4-64x64-2^32B", "S2-33x50-2^32B"])
def test_decoder_bwd_deep_batch(pool, S, shape):
    """hrn_kt_decoder_bwd (f32): `fused` and d_fused past 2^32 bytes.  fused and d_sr are zero except at the checked images (every one
    of the five gradients is a sum over all images); there they are decoder_inputs' values, which make `up` exact"""
    H, W = SHAPES[shape]
    lib = _lib()
    N = _count(F32, "2^32B", H * W * 64)
    _need(2 * N * H * W * 64 * 4 / GIB + N * S * S * H * W * 4 / GIB + 2)
    imgs = _images((N, H * W * 64, 4), (N, S * S * H * W, 4))
    fz, dz, wd_, bd_, wf = K.decoder_inputs(len(imgs), H, W, S, 120 + S)
    fused = pool.big(N, (H, W, 64), F32, "zero")
    d_sr = pool.big(N, (S * H, S * W), F32, "zero")
    for k, m in enumerate(imgs):
        fused.set_img(m, fz[k])
        d_sr.set_img(m, dz[k])
    d_fused = pool.big(N, (H, W, 64), F32, "sent")
    a = 0.25
    names = ["dwd", "dbd", "dad", "dwf", "dbf"]
    shapes = {"dwd": (64, 64, S, S), "dbd": (64,), "dad": (), "dwf": (64,), "dbf": ()}
    acc = {k: Acc(shapes[k], 121 + i) for i, k in enumerate(names)}
    dev = [t.cuda() for t in (wd_, bd_, torch.tensor([a]), wf)]
    sc = _scratch(pool)
    sums = [(t, t.checksum()) for t in (fused, d_sr)]
    rc = lib.hrn_kt_decoder_bwd(S, fused.ptr, d_sr.ptr, *[_p(t) for t in dev], d_fused.ptr, *[acc[k].ptr for k in names], N, H, W, _p(sc), _stream())
    assert rc == 0, (rc, lib.hrn_last_error())
    torch.cuda.synchronize()
    assert all(t.checksum() == c for t, c in sums) and d_fused.guards_intact()
    tag = f"decoder_bwd S={S} {shape} N={N}"
    _says(tag, "2^32B", fused, d_fused)
    ref = K.ref_decoder_bwd(fz.double(), dz.double(), wd_.double(), bd_.double(), a, wf.double(), S)
    for k, m in enumerate(imgs):
        _assert_close(f"{tag} d_fused image {m}", "f32", d_fused.img(m), ref["d_fused"][0][k], ref["d_fused"][1][k], layout="y x c")
    for k in names:
        acc[k].check(f"{tag} {k}", *ref[k], layout="ci co ky kx" if k == "dwd" else "i")


# ----------------------------------------------------------------------------------------------------------- the backward's elementwise kernels
def _plain(dt, cross, per):
    M = _count(dt, cross, per)
    return M, boundary_images(M, per, ES[dt])


HW = 64 * 64
# F32 and bf16x3 hold twice the bytes per element: three tensors of 2^31 elements are 24 GiB
ELEM = [("bf16", "2^31el", HW), ("bf16", "2^31el", 33 * 50), ("bf16x3", "2^31el", HW), ("f32", "2^31el", HW)]
ELEM_IDS = [f"{a}-{'64x64' if c == HW else '33x50'}-{b}" for a, b, c in ELEM]


@pytest.mark.parametrize("dtn,cross,hw", ELEM, ids=ELEM_IDS)
def test_prelu_bwd_bias_deep_batch(pool, dtn, cross, hw):
    """hrn_kt_prelu_bwd_bias, C = 64: g per element at the checked images; db and dslope are sums over all rows, so dy is zero elsewhere"""
    dt, Cc, a = DT[dtn], 64, 0.25
    lib = _lib()
    M, imgs = _plain(dt, cross, hw * Cc)
    _need(3 * M * hw * Cc * ES[dt] * (2 if dt == BF16X3 else 1) / GIB + 2)
    dy = pool.big(M, (hw, Cc), dt, "zero", 131)
    dy.rand_images(imgs)
    y = pool.big(M, (hw, Cc), dt, "rand", 132)
    g = pool.big(M, (hw, Cc), dt, "sent")
    db, dsl = Acc((Cc,), 133), Acc((), 134)
    sc, sl = _scratch(pool), _dev1(a)
    sums = [(t, t.checksum()) for t in (dy, y)]
    # (a > 0: the kernel reads the stored post-activation y and never xpre, which is handed the same tensor)
    rc = lib.hrn_kt_prelu_bwd_bias(dt, dy.ptr, y.ptr, y.ptr, _p(sl), g.ptr, M * hw, Cc, dsl.ptr, db.ptr, _p(sc), _stream())
    assert rc == 0, (rc, lib.hrn_last_error())
    torch.cuda.synchronize()
    assert all(t.checksum() == c for t, c in sums) and g.guards_intact()
    tag = f"prelu_bwd_bias {dtn} rows={M * hw}"
    _says(tag, cross, dy)
    dslope = Ts = 0.0
    dbw, Tb = torch.zeros(Cc, dtype=torch.float64), torch.zeros(Cc, dtype=torch.float64)
    for m in imgs:
        gw, s, ts, b, tb = K.ref_prelu_bwd(dy.img(m), y.img(m), a)
        _assert_close(f"{tag} g image {m}", KIND[dt], g.img(m), gw, gw.abs(), layout="row c")
        dslope, Ts, dbw, Tb = dslope + s, Ts + ts, dbw + b, Tb + tb
    db.check(tag + " db", dbw, Tb, layout="c")
    dsl.check(tag + " dslope", dslope, Ts, layout="")


@pytest.mark.parametrize("dtn,shape", DT_SHAPES, ids=DT_SHAPE_IDS)
def test_colsum_deep_batch(pool, dtn, shape):
    """hrn_kt_colsum, C = 128: g zero except at the checked images"""
    dt, Cc, HW = DT[dtn], 128, SHAPES[shape][0] * SHAPES[shape][1]
    lib = _lib()
    M, imgs = _plain(dt, "2^31el", HW * Cc)
    _need(M * HW * Cc * ES[dt] * (2 if dt == BF16X3 else 1) / GIB + 2)
    g = pool.big(M, (HW, Cc), dt, "zero", 141)
    g.rand_images(imgs)
    db = Acc((Cc,), 142)
    sc = _scratch(pool)
    c0 = g.checksum()
    assert lib.hrn_kt_colsum(dt, g.ptr, M * HW, Cc, db.ptr, _p(sc), _stream()) == 0
    torch.cuda.synchronize()
    assert g.checksum() == c0
    _says(f"colsum {dtn} rows={M * HW}", "2^31el", g)
    vals = torch.cat([g.img(m) for m in imgs])
    db.check(f"colsum {dtn} rows={M * HW}", vals.sum(0), vals.abs().sum(0), layout="c")


def _add_case(pool, dt, cross, hw):
    lib = _lib()
    per = hw * 64
    M, imgs = _plain(dt, cross, per)
    _need(3 * M * per * ES[dt] * (2 if dt == BF16X3 else 1) / GIB + 2)
    a, b, o = pool.big(M, (per,), dt, "rand", 151), pool.big(M, (per,), dt, "rand", 152), pool.big(M, (per,), dt, "sent")
    sums = [(t, t.checksum()) for t in (a, b)]
    assert lib.hrn_kt_add(dt, a.ptr, b.ptr, o.ptr, M * per, _stream()) == 0
    torch.cuda.synchronize()
    assert all(t.checksum() == c for t, c in sums) and o.guards_intact()
    return a, b, o, M, imgs


@pytest.mark.parametrize("dtn,cross,hw", ELEM, ids=ELEM_IDS)
def test_add_deep_batch(pool, dtn, cross, hw):
    """hrn_kt_add: o = a + b"""
    dt = DT[dtn]
    a, b, o, M, imgs = _add_case(pool, dt, cross, hw)
    _says(f"add {dtn} n={o.n}", cross, o)
    for m in imgs:
        _assert_close(f"add {dtn} image {m}", KIND[dt], o.img(m), a.img(m) + b.img(m), a.img(m).abs() + b.img(m).abs(), layout="i")


@pytest.mark.parametrize("dtn,cross,hw", ELEM, ids=ELEM_IDS)
def test_pair_add_deep_batch(pool, dtn, cross, hw):
    """hrn_kt_pair_add: t2 = cat(view 0, view 1) + u, three tensors of the same size"""
    dt = DT[dtn]
    lib = _lib()
    B, bs = _plain(dt, cross, hw * 128)
    _need(3 * B * hw * 128 * ES[dt] * (2 if dt == BF16X3 else 1) / GIB + 2)
    stack, u, t2 = pool.big(B, (V2, hw, 64), dt, "rand", 161), pool.big(B, (hw, 128), dt, "rand", 162), pool.big(B, (hw, 128), dt, "sent")
    sums = [(t, t.checksum()) for t in (stack, u)]
    assert lib.hrn_kt_pair_add(dt, stack.ptr, V2, 1, 1, u.ptr, t2.ptr, hw, B, _stream()) == 0
    torch.cuda.synchronize()
    assert all(t.checksum() == c for t, c in sums) and t2.guards_intact()
    _says(f"pair_add {dtn} B={B}", cross, t2)
    for b in bs:
        want, T = K.ref_pair_add(stack.img(b)[None], u.img(b)[None, None], 1)
        _assert_close(f"pair_add {dtn} sample {b}", KIND[dt], t2.img(b)[None, None], want, T, layout="b v p c")


@pytest.mark.parametrize("dtn,cross,shape", [("bf16", "2^31el", "64x64"), ("bf16x3", "2^32B", "64x64"), ("f32", "2^32B", "64x64"), ("bf16", "2^31el", "33x50")],
                         ids=["bf16-64x64-2^31el", "bf16x3-64x64-2^32B", "f32-64x64-2^32B", "bf16-33x50-2^31el"])
def test_fuse_update_deep_batch(pool, dtn, cross, shape):
    """hrn_kt_fuse_update: the stack [B][2][hw][64] is twice the size of f and of the output.  bf16: f passes 2^31 elements (the stack
    2^32).  bf16x3 / f32: that would put 32 GiB on the device, so the stack passes 2^31 elements (2^32 bytes a plane) and f 2^31 bytes (f32:
    2^32)"""
    dt, hw = DT[dtn], SHAPES[shape][0] * SHAPES[shape][1]
    lib = _lib()
    B = _count(dt, cross, hw * 64) if dtn == "bf16" else (1 << 31) // (hw * 128) + 2
    planes = 2 if dt == BF16X3 else 1
    _need(4 * B * hw * 64 * ES[dt] * planes / GIB + 2)
    bs = _images((B, hw * 128, ES[dt]), (B, hw * 64, ES[dt]))
    stack, f, out = pool.big(B, (V2, hw, 64), dt, "rand", 171), pool.big(B, (1, hw, 64), dt, "rand", 172), pool.big(B, (1, hw, 64), dt, "sent")
    al = K._alphas(B, V2)
    ad = al.cuda()
    sums = [(t, t.checksum()) for t in (stack, f)]
    assert lib.hrn_kt_fuse_update(dt, stack.ptr, V2, f.ptr, _p(ad), V2, 1, 1, 1, out.ptr, hw, B, _stream()) == 0
    torch.cuda.synchronize()
    assert all(t.checksum() == c for t, c in sums) and out.guards_intact()
    print(f"fuse_update {dtn} B={B}: stack {crossed(stack.n, stack.esize)}, f {crossed(f.n, f.esize)}")
    assert cross in crossed(stack.n, stack.esize) and "2^31B" in crossed(f.n, f.esize)
    for b in bs:
        want, T = K.ref_fuse_update(stack.img(b)[None], f.img(b)[None], al[b:b + 1], 1, 1)
        _assert_close(f"fuse_update {dtn} sample {b}", KIND[dt], out.img(b)[None], want, T, layout="b v p c")


@pytest.mark.parametrize("dtn,shape", DT_SHAPES, ids=DT_SHAPE_IDS)
def test_fuse_df_deep_batch(pool, dtn, shape):
    """hrn_kt_fuse_df: df = alpha[partner] ds'"""
    dt, hw = DT[dtn], SHAPES[shape][0] * SHAPES[shape][1]
    lib = _lib()
    B, bs = _plain(dt, "2^31el", hw * 64)
    _need(2 * B * hw * 64 * ES[dt] * (2 if dt == BF16X3 else 1) / GIB + 2)
    dsn, df = pool.big(B, (1, hw, 64), dt, "rand", 181), pool.big(B, (1, hw, 64), dt, "sent")
    al = K._alphas(B, V2)
    ad = al.cuda()
    c0 = dsn.checksum()
    assert lib.hrn_kt_fuse_df(dt, dsn.ptr, _p(ad), V2, 1, 1, 1, df.ptr, hw, B, _stream()) == 0
    torch.cuda.synchronize()
    assert dsn.checksum() == c0 and df.guards_intact()
    _says(f"fuse_df {dtn} B={B}", "2^31el", df)
    for b in bs:
        want, T = K.ref_fuse_df(dsn.img(b)[None], al[b:b + 1], 1, 1)
        _assert_close(f"fuse_df {dtn} sample {b}", KIND[dt], df.img(b)[None], want, T, layout="b v p c")


@pytest.mark.parametrize("dtn,shape", DT_SHAPES, ids=DT_SHAPE_IDS)
def test_fuse_scatter_deep_batch(pool, dtn, shape):
    """hrn_kt_fuse_scatter: dz [B][hw][128] and ds [B][2][hw][64] pass 2^31 elements, dsn is half their size"""
    dt, hw, cross = DT[dtn], SHAPES[shape][0] * SHAPES[shape][1], "2^31el"
    lib = _lib()
    B = _count(dt, cross, hw * 128)
    _need(5 * B * hw * 64 * ES[dt] * (2 if dt == BF16X3 else 1) / GIB + 2)
    bs = _images((B, hw * 128, ES[dt]), (B, hw * 64, ES[dt]))
    dsn, dz, ds = pool.big(B, (1, hw, 64), dt, "rand", 191), pool.big(B, (1, hw, 128), dt, "rand", 192), pool.big(B, (V2, hw, 64), dt, "sent")
    sums = [(t, t.checksum()) for t in (dsn, dz)]
    assert lib.hrn_kt_fuse_scatter(dt, dsn.ptr, dz.ptr, V2, 1, 1, 1, ds.ptr, hw, B, _stream()) == 0
    torch.cuda.synchronize()
    assert all(t.checksum() == c for t, c in sums) and ds.guards_intact()
    print(f"fuse_scatter {dtn} B={B}: ds {crossed(ds.n, ds.esize)}, dsn {crossed(dsn.n, dsn.esize)}")
    assert cross in crossed(ds.n, ds.esize)
    for b in bs:
        want, T = K.ref_fuse_scatter(dsn.img(b)[None], dz.img(b)[None], V2, 1, 1)
        _assert_close(f"fuse_scatter {dtn} sample {b}", KIND[dt], ds.img(b)[None], want, T, layout="b v p c")


@pytest.mark.parametrize("dtn,shape", DT_SHAPES, ids=DT_SHAPE_IDS)
def test_alpha_grad_deep_batch(pool, dtn, shape):
    """hrn_kt_alpha_grad: one sum per image, so the inputs are dense; d_alphas[b][1] per checked sample, column 0 untouched everywhere"""
    dt, hw = DT[dtn], SHAPES[shape][0] * SHAPES[shape][1]
    lib = _lib()
    B, bs = _plain(dt, "2^31el", hw * 64)
    _need(2 * B * hw * 64 * ES[dt] * (2 if dt == BF16X3 else 1) / GIB + 2)
    dsn, f = pool.big(B, (1, hw, 64), dt, "rand", 201), pool.big(B, (1, hw, 64), dt, "rand", 202)
    da0 = torch.randn((B, V2), generator=torch.Generator().manual_seed(203))
    da = torch.cat([da0.reshape(-1), torch.full((64,), float("nan"))]).cuda()
    nbytes = lib.hrn_kt_alpha_grad_scratch_bytes(B)
    sc = torch.empty(nbytes + 64, dtype=torch.uint8, device="cuda")
    sums = [(t, t.checksum()) for t in (dsn, f)]
    assert lib.hrn_kt_alpha_grad(dt, dsn.ptr, f.ptr, 1, 1, _p(da), B, V2, hw, _p(sc), nbytes, _stream()) == 0
    torch.cuda.synchronize()
    assert all(t.checksum() == c for t, c in sums)
    _says(f"alpha_grad {dtn} B={B}", "2^31el", dsn)
    got = da.cpu()
    assert bool(torch.isnan(got[B * V2:]).all())
    got = got[:B * V2].reshape(B, V2)
    assert torch.equal(got[:, 0].view(torch.int32), da0[:, 0].contiguous().view(torch.int32)), "an entry outside the level was written"
    for b in bs:
        want, T = K.ref_alpha_grad(dsn.img(b)[None], f.img(b)[None])
        _assert_close(f"alpha_grad {dtn} sample {b}", "f32", got[b:b + 1, 1:2].double(), want, T, layout="b v")


# ----------------------------------------------------------------------------------------------------------- bit-exact: planes, median
@pytest.mark.parametrize("two", [True, False], ids=["two-2^31el", "one-2^31el"])
def test_f32_to_planes_deep(pool, two):
    """hrn_kt_f32_to_planes: 2^31 elements and more, bit for bit at the chunks around every crossing of the input and of a plane"""
    lib = _lib()
    per = 1 << 16
    M = _count(F32, "2^31el", per)
    _need((M * per * 4 + M * per * 2 * (2 if two else 1)) / GIB + 2)
    imgs = _images((M, per, 4), (M, per, 2))
    src = pool.big(M, (per,), F32, "rand", 211)
    out = pool.big(M, (per,), BF16X3 if two else BF16, "sent")
    c0 = src.checksum()
    assert lib.hrn_kt_f32_to_planes(src.ptr, out.ptr, out.lo_off, M * per, _stream()) == 0
    torch.cuda.synchronize()
    assert src.checksum() == c0 and out.guards_intact()
    _says(f"f32_to_planes two={two} n={M * per}", "2^31el", src)
    for m in imgs:
        hi, lo = K.ref_split_planes(src.bits(m).view(torch.float32))
        want = torch.cat([hi.view(torch.int16), lo.view(torch.int16)]) if two else hi.view(torch.int16)
        bad = int((out.bits(m) != want).sum())
        print(f"f32_to_planes chunk {m}: {bad} words differ")
        assert bad == 0


@pytest.mark.parametrize("two", [True, False], ids=["two-2^31el", "one-2^31el"])
def test_planes_to_f32_deep(pool, two):
    """hrn_kt_planes_to_f32: out = float(hi) + float(lo) (one plane: float(hi)), bit for bit"""
    lib = _lib()
    per = 1 << 16
    M = _count(F32, "2^31el", per)
    _need((M * per * 4 + M * per * 2 * (2 if two else 1)) / GIB + 2)
    imgs = _images((M, per, 4), (M, per, 2))
    planes = pool.big(M, (per,), BF16X3 if two else BF16, "rand", 221)
    out = pool.big(M, (per,), F32, "sent")
    c0 = planes.checksum()
    assert lib.hrn_kt_planes_to_f32(planes.ptr, planes.lo_off, out.ptr, M * per, _stream()) == 0
    torch.cuda.synchronize()
    assert planes.checksum() == c0 and out.guards_intact()
    _says(f"planes_to_f32 two={two} n={M * per}", "2^31el", out)
    for m in imgs:
        b = planes.bits(m).view(torch.bfloat16).float()
        want = b[:per] + b[per:] if two else b
        bad = int((out.bits(m).view(torch.int32) != want.view(torch.int32)).sum())
        print(f"planes_to_f32 chunk {m}: {bad} words differ")
        assert bad == 0


@pytest.mark.parametrize("shape", list(SHAPES), ids=[s + "-2^31el" for s in SHAPES])
def test_median_deep_batch(pool, shape):
    """hrn_kt_median: lrs [B][9][H][W] f32 past 2^31 elements, == torch.median at the checked samples"""
    lib = _lib()
    V, (H, W) = 9, SHAPES[shape]
    B = _count(F32, "2^31el", V * H * W)
    _need((B * V * H * W * 4 + B * H * W * 4) / GIB + 2)
    bs = boundary_images(B, V * H * W, 4)
    lrs = pool.big(B, (V, H, W), F32, "rand", 231)
    ref = pool.keep(torch.full((B * H * W + 64,), float("nan"), device="cuda"))
    c0 = lrs.checksum()
    assert lib.hrn_kt_median(lrs.ptr, _p(ref), B, V, H, W, _stream()) == 0
    torch.cuda.synchronize()
    assert lrs.checksum() == c0 and bool(torch.isnan(ref[B * H * W:]).all())
    _says(f"median B={B}", "2^31el", lrs)
    for b in bs:
        want = K.ref_median(lrs.img(b)[None])
        got = ref[b * H * W:(b + 1) * H * W].cpu().double().reshape(1, H, W)
        bad = int((got != want).sum())
        print(f"median sample {b}: {bad} pixels differ")
        assert bad == 0


# ----------------------------------------------------------------------------------------------------------- the masked composite
def _composite_inputs(pool, B, V, H, W, seed):
    """views (eighths in [0, 3): ties) and masks (0 at 40 % of the pixels, else 1, 2 or 3) of (B, V, H, W), generated on the device in
    place, chunk by chunk; alphas (B, V) with 0, 3, 6, 9 or 12 trailing zeros by sample"""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    n = B * V * H * W
    views, masks = pool.keep(torch.empty(n, device="cuda")), pool.keep(torch.empty(n, device="cuda"))
    for a in range(0, n, Big.CHUNK):
        b = min(n, a + Big.CHUNK)
        views[a:b].random_(0, 24, generator=gen).mul_(0.125)
        masks[a:b].random_(0, 5, generator=gen).sub_(1.0).clamp_(min=0.0)
    alphas = (torch.arange(V)[None] < (V - 3 * (torch.arange(B)[:, None] % 5))).float()
    return views.view(B, V, H, W), masks.view(B, V, H, W), alphas


@pytest.mark.parametrize("shape", list(SHAPES), ids=[s + "-2^31el" for s in SHAPES])
def test_masked_composite_deep_batch(pool, shape):
    """hrn_masked_composite, masked_composite_kernel<9>: views, masks and filled [B][32][H][W] f32 past 2^31 elements, n_ref = 9 so that the
    loop over the views 9..31 that do not vote runs at the high offsets too; ref, count and filled bit for bit against the numpy
    restatement at sample 0, the last sample and the samples at every crossing.  Control (64 x 64, where it is a whole number of samples):
    the restatement of the views a 32-bit byte base would address, sample b - 2^32 / (V H W 4), is told from the output"""
    import composite_ref as R
    lib = _lib()
    V, n_ref, (H, W) = 32, 9, SHAPES[shape]
    hw = H * W
    B = _count(F32, "2^31el", V * hw)
    _need(3 * B * V * hw * 4 / GIB + 2 * B * hw * 4 / GIB + 2)
    bs = boundary_images(B, V * hw, 4)
    views, masks, alphas = _composite_inputs(pool, B, V, H, W, 261)
    ad = alphas.cuda()
    ref, count, filled = _nan_out(pool, B * hw), _nan_out(pool, B * hw), _nan_out(pool, B * V * hw)
    sums = [(t, _sum64(t)) for t in (views, masks)]
    rc = lib.hrn_masked_composite(_p(views), _p(masks), _p(ad), B, V, H, W, n_ref, _p(ref), _p(count), _p(filled), _stream())
    assert rc == 0, (rc, lib.hrn_last_error())
    torch.cuda.synchronize()
    assert all(_sum64(t) == c for t, c in sums) and torch.equal(ad.cpu(), alphas), "the launch wrote one of its inputs"
    for t, n in ((ref, B * hw), (count, B * hw), (filled, B * V * hw)):
        assert bool(torch.isnan(t[n:]).all()), "a write past an output"
    got = crossed(B * V * hw, 4)
    print(f"masked_composite {shape} B={B}: views {B * V * hw * 4 / GIB:.2f} GiB {got}; samples {bs}")
    assert "2^31el" in got and len(bs) >= 5
    assert any(float(alphas[b, -1]) == 0 for b in bs) and any(float(alphas[b, -1]) != 0 for b in bs)
    wrap = (1 << 32) // (V * hw * 4) if (1 << 32) % (V * hw * 4) == 0 else None
    told = 0
    for b in bs:
        v, m, a = views[b:b + 1].cpu().numpy(), masks[b:b + 1].cpu().numpy(), alphas[b:b + 1].numpy()
        want_ref, want_count, want_filled = R.masked_composite(v, m, a, n_ref)
        g_ref, g_count = ref[b * hw:(b + 1) * hw].view(1, H, W), count[b * hw:(b + 1) * hw].view(1, H, W)
        assert _bits_equal(g_ref, want_ref), ("ref", b)
        assert _bits_equal(g_count, want_count), ("count", b)
        assert _bits_equal(filled[b * V * hw:(b + 1) * V * hw].view(1, V, H, W), want_filled), ("filled", b)
        if wrap is not None and b >= wrap:
            wrong = R.masked_composite(views[b - wrap:b - wrap + 1].cpu().numpy(), m, a, n_ref)[0]
            differ = int((g_ref.cpu().numpy() != wrong).sum())
            print(f"masked_composite sample {b} against the views of sample {b - wrap}: {differ} of {hw} pixels differ")
            assert differ > hw // 2, f"the comparison does not tell sample {b - wrap} from sample {b}"
            told += 1
    assert wrap is None or told >= 2


def test_masked_composite_big_frame(pool):
    """hrn_masked_composite, masked_composite_kernel<32>: one sample of 32 views of 8200 x 8190, 32 H W > 2^31 elements.  Only view 31 reaches
    past element 2^31 (from row 8008 on; views 16..31 lie past byte 2^32), so view 31 is a real view that votes - the views without a
    vote are 3, 4 and 5 - and the bottom strip lies wholly past element 2^31 in it.  The grid is 262336 tiles of one sample.  ref and count
    bit for bit against the numpy restatement on two rows each at the top, in the middle and at the bottom.  Control: at the bottom strip
    the restatement of the same pixels with view 31's values and mask exchanged for others must NOT be the output - a kernel that read view
    31 from a wrapped offset would otherwise pass"""
    import composite_ref as R
    lib = _lib()
    B, V, n_ref, H, W = 1, 32, 32, 8200, 8190
    hw = H * W
    first_past = ((1 << 31) - (V - 1) * hw) // W                 # the first row of view 31 that lies wholly or partly past element 2^31
    assert (V - 1) * hw < 1 << 31 < V * hw and first_past == 8008 and first_past < H - 2
    _need(2 * V * hw * 4 / GIB + 2 * hw * 4 / GIB + 2)
    views, masks, alphas = _composite_inputs(pool, B, V, H, W, 262)
    alphas[0, 3:6] = 0
    assert float(alphas[0, V - 1]) != 0
    ad = alphas.cuda()
    ref, count = _nan_out(pool, hw), _nan_out(pool, hw)
    sums = [(t, _sum64(t)) for t in (views, masks)]
    rc = lib.hrn_masked_composite(_p(views), _p(masks), _p(ad), B, V, H, W, n_ref, _p(ref), _p(count), None, _stream())
    assert rc == 0, (rc, lib.hrn_last_error())
    torch.cuda.synchronize()
    assert all(_sum64(t) == c for t, c in sums), "the launch wrote one of its inputs"
    assert bool(torch.isnan(ref[hw:]).all()) and bool(torch.isnan(count[hw:]).all()), "a write past an output"
    print(f"masked_composite big frame {H}x{W}: views {V * hw * 4 / GIB:.2f} GiB {crossed(V * hw, 4)}")
    assert "2^31el" in crossed(V * hw, 4)
    for y0 in (0, H // 2, H - 2):
        y1 = y0 + 2
        v, m = views[:, :, y0:y1].cpu().numpy(), masks[:, :, y0:y1].cpu().numpy()
        want_ref, want_count, _ = R.masked_composite(v, m, alphas.numpy(), n_ref)
        g_ref, g_count = ref[y0 * W:y1 * W].view(1, 2, W), count[y0 * W:y1 * W].view(1, 2, W)
        assert _bits_equal(g_ref, want_ref), ("ref", y0)
        assert _bits_equal(g_count, want_count), ("count", y0)
        assert want_count.max() > 16 and want_count.min() < 16
        if y0 >= first_past:
            # the outputs depend on view 31 here: its mask inverted moves count at every pixel, its values moved out of the others' range
            # move the median wherever it votes as one of the upper half
            v2, m2 = v.copy(), m.copy()
            v2[:, V - 1] += 100.0
            m2[:, V - 1] = (m[:, V - 1] == 0).astype(m.dtype)
            wrong_ref = R.masked_composite(v2, m, alphas.numpy(), n_ref)[0]
            wrong_count = R.masked_composite(v, m2, alphas.numpy(), n_ref)[1]
            d_ref, d_count = int((g_ref.cpu().numpy() != wrong_ref).sum()), int((g_count.cpu().numpy() != wrong_count).sum())
            print(f"masked_composite big frame rows {y0}..{y1}: with another view 31, ref differs at {d_ref} and count at {d_count} of {2 * W} pixels")
            assert d_count == 2 * W and d_ref > 2 * W // 20, "the comparison does not see view 31, the one view past element 2^31"


# ----------------------------------------------------------------------------------------------------------- negative controls
@pytest.mark.parametrize("which", ["conv", "add"])
def test_negative_control(pool, which):
    """The comparison must FAIL on the same GPU output when the reference is taken from the image a base truncated to 32 bits would
    address, m - 2^32 / image bytes, and pass against the right one: the encoder's bf16 convolution and add_kernel<BF16> of regime A."""
    H, W = 64, 64
    wrap = (1 << 32) // (H * W * 64 * 2)
    if which == "conv":
        M, tensors, need = _conv_sizes("enc", BF16, "2^31el", H, W)
        _need(need)
        high = [m for m in _images(*tensors) if m >= wrap]
        r = _conv_case(pool, "enc", BF16, 0, M, H, W, [(m, 0, H) for m in high], 500 + 3, also=[(m - wrap, 0, H) for m in high])
        pairs = [(r["got"]((m, 0, H)), r["ref"]((m, 0, H)), r["ref"]((m, 0, H), src=(m - wrap, 0, H))) for m in high]
        layout = "c y x"
    else:
        a, b, o, M, imgs = _add_case(pool, BF16, "2^31el", HW)
        high = [m for m in imgs if m >= wrap]
        pairs = [(o.img(m), (a.img(m) + b.img(m), a.img(m).abs() + b.img(m).abs()),
                  (a.img(m - wrap) + b.img(m - wrap), a.img(m - wrap).abs() + b.img(m - wrap).abs())) for m in high]
        layout = "i"
    assert len(high) >= 2 and M > wrap
    for m, (got, right, wrong) in zip(high, pairs):
        ok = _assert_close(f"{which} image {m} (right reference)", "bf16", got, *right, layout=layout)
        worst, _ = _ratio("bf16", got, *wrong)
        print(f"{which} image {m} against image {m - wrap}: error / bound {worst:.3e} (right one {ok:.3e})")
        assert worst > 1.0, f"{which}: the comparison does not tell image {m - wrap} from image {m}"


# ----------------------------------------------------------------------------------------------------------- B: one big frame
def _strips(H, rows=32, align=16):
    """top, middle and bottom strips: starts aligned to every kernel's tile height (8 and 16 rows), >= 24 rows each"""
    mid = (H // 2) // align * align
    bot = (H - 24) // align * align
    assert rows >= 24 and H - bot >= 24 and rows < mid and mid + rows < bot
    return [(0, 0, rows), (0, mid, mid + rows), (0, bot, H)]


# (layer, storage, H, W, the family the profiler must show, a family it must not show: a layer with a residual is filed under "...+res" by
# r64 / v6 and under the plain name by the general kernel; the plain layers share one name, and the launch counter "conv_general" tells)
FRAME_CONV = [
    # conv3x3_r64: H W 128 < 2^31
    ("enc", "bf16", 4095, 4096, "conv3x3_bf16_64x64+res", None), ("enc", "bf16", 4093, 4090, "conv3x3_bf16_64x64+res", None),
    ("enc", "bf16", 4096, 4096, "conv3x3_bf16_64x64", "conv3x3_bf16_64x64+res"),
    ("plain64", "bf16", 4095, 4096, "conv3x3_bf16_64x64", None),
    # conv3x3_v6 at cin 128: H W 256 < 2^31
    ("alpha", "bf16", 2047, 4096, "conv3x3_bf16_128x64+res", None), ("alpha", "bf16", 2045, 4090, "conv3x3_bf16_128x64+res", None),
    ("alpha", "bf16", 2048, 4096, "conv3x3_bf16_128x64", "conv3x3_bf16_128x64+res"),
    # conv3x3_v6 at cout 128 (cin 64): the OUTPUT image is the wider one
    ("up", "bf16", 2047, 4096, "conv3x3_bf16_64x128", None), ("up", "bf16", 2045, 4090, "conv3x3_bf16_64x128", None),
    ("up", "bf16", 2048, 4096, "conv3x3_bf16_64x128", None),
    # conv3x3_kernel, the general kernel, where ONE image passes 2^32 bytes (its in-image offsets are 64-bit): bf16 behind r64's refusal, f32
    ("enc", "bf16", 8200, 4096, "conv3x3_bf16_64x64", "conv3x3_bf16_64x64+res"), ("enc", "f32", 4100, 4096, "conv3x3_f32_64x64", None),
    # conv3x3_v6x3, 64 -> 64: H W 128 < 2^31
    ("enc", "bf16x3", 4095, 4096, "conv3x3_bf16x3_64x64+res", None), ("enc", "bf16x3", 4093, 4090, "conv3x3_bf16x3_64x64+res", None),
]


@pytest.mark.parametrize("layer,dtn,H,W,fam,not_fam", FRAME_CONV, ids=[f"{a}-{b}-{c}x{d}" for a, b, c, d, _, _ in FRAME_CONV])
def test_conv_big_frame(pool, layer, dtn, H, W, fam, not_fam):
    """One image just under a fast kernel's in-image limit (W a multiple of 32 and ragged), and the smallest image its guard refuses,
    which must run on conv3x3.hip's general kernel - as must an image of more than 2^32 bytes, the bottom strip of which lies past every
    32-bit offset: three strips per element, the route read from the profiler's family names and the launch counter `conv_general`"""
    dt = DT[dtn]
    cin, cout = CONV[layer][:2]
    _need(H * W * (cin + cout + 128) * ES[dt] * (2 if dt == BF16X3 else 1) / GIB + 2)
    regions = _strips(H)
    r = _conv_case(pool, layer, dt, 0, 1, H, W, regions, 600 + len(layer))
    ran = sorted(k[5:] for k in r["fams"] if k.startswith("prof:conv3x3"))
    print(f"conv {layer} {dtn} {H}x{W}: H W = {H * W}, families {ran}")
    assert fam in ran and not_fam not in ran, ran
    general = dt == F32 or (dt == BF16 and H * W * 2 * max(cin, cout) >= 1 << 31)       # f32 has no other kernel; bf16: refused by r64 / v6
    assert r["fams"]["conv_general"] == (1 if general else 0), (r["fams"]["conv_general"], general)
    for reg in regions:
        want, T = r["ref"](reg)
        _assert_close(f"conv {layer} {dtn} {H}x{W} rows {reg[1]}..{reg[2]}", r["kind"], r["got"](reg), want, T, layout="c y x", c=r["c"])


@pytest.mark.parametrize("layer,H,W", [("enc", 4096, 4096), ("up", 2048, 4096)], ids=["enc-4096x4096", "up-2048x4096"])
def test_conv_x3_refuses_big_frame(pool, layer, H, W):
    """conv3x3_v6x3 has no general kernel behind it: the smallest image past its limit (of the wider of input and output) is an error,
    and nothing is written"""
    cin, cout = CONV[layer][:2]
    _need(H * W * (cin + cout) * 4 / GIB + 2)
    lib = _lib()
    inp, out = pool.big(1, (H, W, cin), BF16X3, "sent", apart=True), pool.big(1, (H, W, cout), BF16X3, "sent", apart=True)
    pk = torch.zeros(cin * cout * 9 * 2, dtype=torch.bfloat16, device="cuda")
    bd = torch.zeros(cout, device="cuda")
    res = out if layer == "enc" else None
    rc = lib.hrn_kt_conv3x3_epi(BF16X3, 0, cin, cout, inp.ptr, None, 0, 0, 0, _p(pk), _p(bd), None, res.ptr if res else None, 1 if res else 0, 0, None, 0,
                                out.ptr, 0, 0, inp.lo_off, 0, out.lo_off, out.lo_off if res else 0, 1, H, W, _stream())
    msg = lib.hrn_last_error()
    torch.cuda.synchronize()
    assert rc == -2 and b"image too large for 32-bit in-image offsets" in msg, (rc, msg)
    assert out.all_sentinels() and inp.all_sentinels()


@pytest.mark.parametrize("dtn", ["bf16", "bf16x3"])
@pytest.mark.parametrize("H,W", [(2047, 4096), (2045, 4090), (2048, 4096)], ids=["2047x4096", "2045x4090", "2048x4096-refused"])
def test_conv_wgrad_big_frame(pool, H, W, dtn):
    """conv_wgrad_x3_kernel<false | true>, 64 -> 64, one image: H W 256 < 2^31 is accepted and right (x and g non-zero in three strips
    only), H W 256 = 2^31 is refused with -2 and dw stays as it was"""
    dt = DT[dtn]
    lib = _lib()
    _need(H * W * 128 * 2 * (2 if dt == BF16X3 else 1) / GIB + 2)
    refused = H * W * 256 >= 1 << 31
    x, g = pool.big(1, (H, W, 64), dt, "zero", 241), pool.big(1, (H, W, 64), dt, "zero", 242)
    regions = _strips(H)
    for t in (x, g):
        for _, y0, y1 in regions:
            t._rand(y0 * W * 64, y1 * W * 64)
    dw = Acc((64, 64, 3, 3), 243)
    sc = _scratch(pool)
    sums = [(t, t.checksum()) for t in (x, g)]
    rc = lib.hrn_kt_conv_wgrad(dt, x.ptr, None, 0, 0, 0, g.ptr, 1, H, W, 64, 64, dw.ptr, _p(sc), _stream())
    msg = lib.hrn_last_error()
    torch.cuda.synchronize()
    assert all(t.checksum() == c for t, c in sums)
    if refused:
        assert rc == -2 and b"conv_wgrad_x3: image too large for 32-bit in-image offsets" in msg, (rc, msg)
        assert torch.equal(dw.buf.cpu()[:dw.n], dw.start) and bool(torch.isnan(dw.buf[dw.n:]).all()), "the refused launch wrote dw"
        return
    assert rc == 0, (rc, msg)
    want, T = 0.0, 0.0
    for _, y0, y1 in regions:       # x is zero around every strip: a strip alone, zero-padded, is the whole sum of its rows
        dwk, Tk = K.ref_conv_wgrad(x.rows(0, y0, y1)[None], g.rows(0, y0, y1)[None])
        want, T = want + dwk, T + Tk
    dw.check(f"conv_wgrad {dtn} {H}x{W}", want, T, layout="co ci ky kx")


@pytest.mark.parametrize("dtn", ["bf16", "bf16x3"])
def test_stem_refuses_segment_count(pool, dtn):
    """The MFMA stem counts its 32-pixel row segments in 32 bits: M H ceil(W / 32) = 2^31 is refused before any launch.  (The accepted side
    of this limit cannot be run: 2^31 - 1 segments are at least 256 GiB of output.)"""
    dt = DT[dtn]
    lib = _lib()
    out = pool.big(1, (4096,), dt, "sent", apart=True)
    small = torch.zeros(4096, device="cuda")
    rc = lib.hrn_kt_stem(dt, _p(small), 1 << 15, _p(small), 1, 1 << 15, None, _p(small), _p(small), None, out.ptr, out.lo_off, 1 << 16, 1 << 15, 1, _stream())
    msg = lib.hrn_last_error()
    torch.cuda.synchronize()
    assert rc == -2 and b"exceed the 32-bit segment count" in msg, (rc, msg)
    assert out.all_sentinels()


def test_stem_dgrad_route_refuses_grid(pool):
    """stem_dgrad_route launches one workgroup per (sample, tile): tiles B = 2^31 is refused before any launch (the accepted side would
    need 2^31 - 1 tiles of dA: terabytes)"""
    lib = _lib()
    out = pool.keep(torch.full((4096,), float("nan"), device="cuda"))
    small = torch.zeros(4096, device="cuda")
    rc = lib.hrn_kt_stem_dgrad_route(BF16, _p(small), _p(small), _p(small), _p(small), _p(small), _p(out), 1 << 30, 1, 9, 1, _stream())
    msg = lib.hrn_last_error()
    torch.cuda.synchronize()
    assert rc == -2 and b"exceed the grid" in msg, (rc, msg)
    assert bool(torch.isnan(out).all())


def test_stem_dgrad_ref_refuses_grid(pool):
    """stem_dgrad_ref launches the routed kernel's grid: tiles B = 2^31 is refused before any launch, and neither output is written"""
    lib = _lib()
    d_lrs, d_ref = pool.keep(torch.full((4096,), float("nan"), device="cuda")), pool.keep(torch.full((4096,), float("nan"), device="cuda"))
    small = torch.zeros(4096, device="cuda")
    rc = lib.hrn_kt_stem_dgrad_ref(BF16, _p(small), _p(small), _p(small), _p(d_lrs), _p(d_ref), 1 << 30, 1, 9, 1, _stream())
    msg = lib.hrn_last_error()
    torch.cuda.synchronize()
    assert rc == -2 and b"exceed the grid" in msg, (rc, msg)
    assert bool(torch.isnan(d_lrs).all()) and bool(torch.isnan(d_ref).all()) and not bool(small.any())


# ----------------------------------------------------------------------------------------------------------- C: the whole network
def test_hrnet_forward_past_2_31_elements(pool):
    """HRNet.forward, inference, bf16, B V H W 64 > 2^31 elements (a workspace of about 13 GiB): finite, and samples 0 and B - 1 are
    bit-identical to their forward alone, as test_hrnet_large_tiles_512 holds inference to at 0.2 G elements"""
    import util
    from hrnet_hip import binding
    B, V, S = 33, 16, 256               # (B = 32 is 2^31 elements exactly)
    assert B * V * S * S * 64 > 1 << 31 and (B - 1) * V * S * S * 64 == 1 << 31       # the last sample lies wholly past element 2^31
    _need(20)
    gen = torch.Generator(device="cuda").manual_seed(251)
    lrs = pool.keep(torch.rand((B, V, S, S), device="cuda", generator=gen))
    alphas = pool.keep((torch.arange(V)[None] < (V - torch.arange(B)[:, None] % 5)).float().cuda())
    m = util.hip_hrnet("bf16")
    try:
        with torch.no_grad():
            y = pool.keep(m(lrs, alphas).clone())
            assert y.shape == (B, 1, 3 * S, 3 * S) and bool(torch.isfinite(y).all())
            for b in (B - 1, 0):
                yb = m(lrs[b:b + 1].contiguous(), alphas[b:b + 1].contiguous())
                assert torch.equal(yb[0], y[b]), f"sample {b} of the batch differs from its forward alone"
    finally:
        binding._ws_cache.clear()
