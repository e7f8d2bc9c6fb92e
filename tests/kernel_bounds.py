"""The conventions of the per-element kernel tests (tests/test_gpu_kernels_fwd.py, test_gpu_kernels_bwd.py, test_gpu_kernels_shiftnet.py,
test_gpu_bf16_train.py, test_gpu_shiftnet_bf16.py, test_gpu_kernels_tail.py): the bound |got - want| <= rounding + C T with its one constant
C (and C_F32 / C_TAIL, the measured bounds of the fp32 forward kernels and of the registered tail's fp32 kernels; the derived bounds of
the tail's fp64 reductions), the sentinel patterns, the tensor builders whose values make a kernel's products exact, and
the shapes and launcher grids the tests share."""
import numpy as np
import torch

from kt import BF16, BF16X3, F32, _cus, _p

C = 1e-5                    # the one constant of every bound (derived in tests/test_gpu_kernels_fwd.py's docstring)
# The fp32 forward kernels (conv3x3_kernel<F32>, stem_kernel<F32>, decoder_kernel<F32, false, S>) are held to |got - want| <= C_F32 T:
# four times the largest "C needed" any fp32 case of tests/test_gpu_kernels_fwd.py measured on the MI355X against fp64, rounded up to one
# significant digit (the margin is for other accumulation orders).  Measured: 4.02e-7 at test_conv[f32encres-multi] (the `full` operand
# set; the other conv instances 3.1e-7 .. 3.9e-7, the stem 3.1e-7, the decoder 2.5e-8; float32 on the CPU needs 2e-7 .. 3e-7), so
# 4 x 4.02e-7 = 1.6e-6 -> 2e-6.  C stays the ceiling: C_F32 <= C.
C_F32 = 2e-6
F32_MEASURED = (4.02e-7, "test_conv[f32encres-multi]")       # (largest C needed, the id of its case)
GUARD = 512                 # sentinel int16 words behind every tensor
SENT = 0x7F7F               # sentinel bit pattern: bf16 3.4e38, and 0x7F7F7F7F as f32
NAN16 = 0x7FC0              # NaN as bf16, and 0x7FC07FC0 as f32
BF = lambda v: float(torch.tensor(v).to(torch.bfloat16))


def _ulp_bf16(x):
    """ulp of bf16 at |x| (fp64 tensor): 2^(e - 7) for |x| in [2^e, 2^(e + 1)), the smallest normal's below it"""
    _, e = torch.frexp(x.abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(x), (e - 8).to(torch.int32))


def _rounding(kind, got, want):
    """the bound's output-rounding term"""
    if kind == "bf16":
        return 0.5 * _ulp_bf16(torch.maximum(got.abs(), want.abs()))
    if kind == "x3":
        return 2.0 ** -16 * want.abs()
    return torch.zeros_like(want)


def _bound(kind, got, want, T, c=C):
    return _rounding(kind, got, want) + c * T


def _ratio(kind, got, want, T, c=C):
    """-> (max error / bound, index of the worst element)"""
    r = (got - want).abs() / (_bound(kind, got, want, T, c) + 1e-300)
    i = int(torch.argmax(r))
    return float(r.reshape(-1)[i]), np.unravel_index(i, tuple(r.shape))


def _assert_close(tag, kind, got, want, T, layout="m c y x", c=C):
    r, idx = _ratio(kind, got, want, T, c)
    c_used = float((((got - want).abs() - _rounding(kind, got, want)).clamp_min(0) / (T + 1e-300)).max())    # the smallest C that passes
    print(f"{tag}: max error / bound {r:.3e} at ({layout}) = {tuple(int(i) for i in idx)}; C needed {c_used:.2e}")
    assert r <= 1.0, (f"{tag}: element ({layout}) = {tuple(int(i) for i in idx)}: got {float(got[idx]):.9g}, want {float(want[idx]):.9g}, "
                      f"bound {float(_bound(kind, got, want, T, c)[idx]):.3g} (error / bound {r:.3g})")
    return r


def _ulp_ok(got, want, n_ulp=1.0, floor=0.0):
    """|got - want| <= n_ulp bf16 ulps of want (+ floor): got a bf16 tensor, want fp64"""
    got, want = got.double().cpu(), want.double().cpu()
    e = torch.floor(torch.log2(want.abs().clamp_min(1e-30)))
    ulp = torch.pow(2.0, e - 7)
    bad = (got - want).abs() > n_ulp * ulp + floor
    return int(bad.sum()), float(((got - want).abs() / ulp).max())


# (H, W); "multi": many 3 x 33 images, enough that a workgroup walks two tiles at least
SHAPES = {"1x1": (1, 1), "2x3": (2, 3), "9x27": (9, 27), "15x33": (15, 33), "17x50": (17, 50), "9x63": (9, 63), "16x64": (16, 64),
          "multi": (3, 33)}


def _grid(route, cout, total, dt=None):
    """the launcher's persistent grid: r64 / v6 / v6x3 min(CUs, total), the general kernel (route 1, and F32 on either route)
    min((2 / (cout / 64)) CUs, total); & ~7"""
    g = (2 // (cout // 64)) * _cus() if route == 1 or dt == F32 else _cus()
    g = min(g, total)
    return g & ~7 if g >= 8 else g


def _tiles(dt, route, cin, cout, H, W):
    # conv3x3.hip (route 1, and every F32 launch) / r64: 8 x 32; v6 / v6x3: 16 x 32
    th, tw = (8, 32) if route == 1 or dt == F32 or (dt == BF16 and cin == 64 and cout == 64) else (16, 32)
    return -(-H // th) * -(-W // tw)


def _bf(shape, seed, scale=1.0):
    """a bf16 device tensor (and its exact fp64 CPU copy) of random values"""
    g = torch.Generator().manual_seed(seed)
    t = (torch.randn(shape, generator=g) * scale).to(torch.bfloat16)
    return t.cuda(), t.double()


def _x3(shape, seed, scale=1.0):
    """a bf16x3 device tensor (2, *shape) - plane 0 hi = bf16(v), plane 1 lo = bf16(v - hi) of random fp32 v, the lo plane directly behind
    the hi plane - and the exact fp64 CPU value hi + lo"""
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(shape, generator=g) * scale
    hi = v.to(torch.bfloat16)
    lo = (v - hi.float()).to(torch.bfloat16)
    return torch.stack([hi, lo]).cuda(), hi.double() + lo.double()


def _f32(shape, seed, scale=1.0):
    """an f32 device tensor of bf16-representable random values (and its exact fp64 CPU copy): the fp32 kernels' products are exact too"""
    t, t64 = _bf(shape, seed, scale)
    return t.float().contiguous(), t64


def _full32(shape, seed, scale=1.0):
    """general fp32 random values (24 significant bits; CPU): the `full` operand set of the fp32 kernels' tests"""
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def round_sig(x, bits):
    """fp64 tensor -> its values rounded (to nearest even) to `bits` significant bits: 8 = bf16, 11 = 10 mantissa bits, 16 = the bf16x3 class"""
    m, e = torch.frexp(x)
    return torch.ldexp(torch.round(torch.ldexp(m, torch.tensor(bits))), e - bits)


def sig_bits(v):
    """fp32 tensor -> the number of significant bits each element carries (24 - trailing zero bits of its mantissa; 0 for 0)"""
    b = v.contiguous().view(torch.int32) & 0x7FFFFF
    tz = torch.full(b.shape, 23, dtype=torch.int32)
    for k in range(22, -1, -1):
        tz = torch.where((b & ((1 << (k + 1)) - 1)) == 0, tz, torch.full_like(tz, k))
    return torch.where(v == 0, torch.zeros_like(tz), 24 - tz)


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _pair_gather(stack, half, pair_last):
    """stack (B, n, H, W, 64) -> (B * half, H, W, 128): cat(view i, view pair_last - i) on channels"""
    B = stack.shape[0]
    idx = torch.arange(half)
    return torch.cat([stack[:, idx], stack[:, pair_last - idx]], -1).reshape((B * half,) + tuple(stack.shape[2:4]) + (128,))


def _quantised(shape, seed, levels=16, scale=0.25):
    """bf16-exact values on a coarse grid (k / 8 * scale, |k| < levels): many ties inside pool windows"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-levels, levels, shape, generator=g).double() / 8 * scale)


def _exact_affine(C, seed):
    """scale a power of two, shift on a coarse bf16 grid: x * scale + shift is exact in fp32 for the quantised x"""
    g = torch.Generator().manual_seed(seed)
    sc = torch.pow(2.0, torch.randint(-1, 2, (C,), generator=g).float())
    sh = torch.randint(-4, 5, (C,), generator=g).float() / 16
    return sc, sh


def q16(v):
    """fp32 tensor -> at most 16 significant bits: hi + lo of its bf16 split is then exact, in fp32 too"""
    return (v.contiguous().view(torch.int32) & ~0xFF).view(torch.float32)


def rnd(shape, seed, dt, scale=1.0):
    """random fp32 values representable in storage dt with at most 16 significant bits (bf16: 8)"""
    v = torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale
    return v.to(torch.bfloat16).float() if dt == BF16 else q16(v)


class Ten:
    """a tensor in storage dt inside an int16 device buffer: f32 (two words per element), one bf16 plane, or bf16x3 = the hi plane and the
    lo plane directly behind it (as every backward kernel derives it from the element count); GUARD sentinels behind.  v: fp32 CPU values
    (rounded to bf16 for BF16; split into hi + lo for BF16X3), or None: filled with `fill`.  val: the exact fp64 value the kernel reads."""

    def __init__(self, shape, dt, v=None, fill=SENT):
        self.shape, self.dt = tuple(shape), dt
        self.n = int(np.prod(shape))
        self.words = self.n * (1 if dt == BF16 else 2)
        raw = torch.full((self.words + GUARD,), SENT, dtype=torch.int16)
        raw[:self.words] = fill
        self.val = None
        if v is not None:
            v = v.contiguous().reshape(-1)
            assert v.dtype == torch.float32 and v.numel() == self.n
            if dt == F32:
                raw[:self.words], self.val = v.view(torch.int16), v.double()
            else:
                hi = v.to(torch.bfloat16)
                raw[:self.n], self.val = hi.view(torch.int16), hi.double()
                if dt == BF16X3:
                    lo = (v - hi.float()).to(torch.bfloat16)
                    raw[self.n:2 * self.n], self.val = lo.view(torch.int16), hi.double() + lo.double()
            self.val = self.val.reshape(self.shape)
        self.bits0 = raw
        self.raw = raw.cuda()

    @property
    def ptr(self):
        return _p(self.raw)

    def planes(self):
        """the payload as CPU tensors: [f32] or [hi] or [hi, lo]"""
        raw = self.raw[:self.words].cpu()
        if self.dt == F32:
            return [raw.view(torch.float32).reshape(self.shape)]
        return [raw[k * self.n:(k + 1) * self.n].view(torch.bfloat16).reshape(self.shape) for k in range(self.words // self.n)]

    def value(self):
        return sum(p.double() for p in self.planes())

    def unchanged(self):
        return torch.equal(self.raw.cpu(), self.bits0)

    def guard_ok(self):
        return bool((self.raw[self.words:] == SENT).all())


class Acc:
    """an f32 gradient the kernel accumulates into (+=): starts from random values, NaN guard behind; none = True: handed over as NULL"""

    def __init__(self, shape, seed, none=False):
        self.shape, self.n = tuple(shape), int(np.prod(shape))
        self.start = torch.randn(self.n, generator=torch.Generator().manual_seed(seed))
        self.buf = None if none else torch.cat([self.start, torch.full((64,), float("nan"))]).cuda()

    @property
    def ptr(self):
        return _p(self.buf)

    def check(self, tag, want, T, c=C, layout="i"):
        """got against start + want, T = |start| + sum |terms|"""
        if self.buf is None:
            return None
        got = self.buf.double().cpu()
        assert bool(torch.isnan(got[self.n:]).all()), f"{tag}: a write past the gradient"
        s0 = self.start.double().reshape(self.shape)
        return _assert_close(tag, "f32", got[:self.n].reshape(self.shape), s0 + want, (s0.abs() + T) * (c / C), layout=layout)


# ----------------------------------------------------------------------------------------------------------- tensors of several GiB
# tests/test_gpu_large_offsets.py: tensors that cross 2^31 bytes, 2^32 bytes and 2^31 elements are generated on the device from a seed and
# only the checked images (or rows) ever reach the host.
def crossings(n, esize):
    """the element offsets inside a plane of n elements of esize bytes at which a 32-bit offset wraps: byte 2^31, byte 2^32, element 2^31"""
    return sorted({e for e in ((1 << 31) // esize, (1 << 32) // esize, 1 << 31) if e < n})


def crossed(n, esize):
    """what a plane of n elements of esize bytes crosses, as the case ids name it: '2^31B', '2^32B', '2^31el'"""
    return [name for name, e in (("2^31B", (1 << 31) // esize), ("2^32B", (1 << 32) // esize), ("2^31el", 1 << 31)) if e < n]


def boundary_images(M, per, esize):
    """the images worth checking of M images of `per` elements (esize bytes each) in one plane: image 0, the last one, and for every
    crossing the image it falls into - or, where it falls exactly between two images, both of them"""
    out = {0, M - 1}
    for e in crossings(M * per, esize):
        out.add(e // per)
        if e % per == 0:
            out.add(e // per - 1)
    return sorted(out)


class Big:
    """M images of shape `img` in storage dt, generated ON THE DEVICE inside a sentinel-guarded int16 buffer: f32 (two words per element),
    one bf16 plane, or bf16x3 = hi plane and lo plane (apart = False: the lo plane directly behind the hi plane, as every backward kernel
    derives it from the element count; apart = True: GUARD + 1024 sentinel words between the planes, as the convolutions' free lo offsets
    allow).  fill: "rand" (normal values x scale from `seed`: bf16 values for BF16, fp32 values for F32, hi + lo of fp32 values for
    BF16X3), "zero", or "sent" (an output: every word a sentinel).  Only img() / rows() copy anything to the host."""
    CHUNK = 1 << 27

    def __init__(self, M, img, dt, fill="sent", seed=0, scale=1.0, apart=False):
        self.M, self.img_shape, self.dt = M, tuple(img), dt
        self.per = int(np.prod(img))
        self.n = M * self.per
        self.wpe = 2 if dt == F32 else 1
        self.esize = 2 * self.wpe
        words = self.n * self.wpe
        self.lo_e = (self.n + (GUARD + 1024 if apart else 0)) if dt == BF16X3 else 0
        total = (self.lo_e + self.n if dt == BF16X3 else words) + GUARD
        total += -total % 4                                     # (checksum() reads the buffer as int64)
        self.raw = torch.empty(total, dtype=torch.int16, device="cuda")
        self.raw.fill_(SENT)
        self.lo_off = 2 * self.lo_e
        self.gen = torch.Generator(device="cuda").manual_seed(seed)
        self.scale = scale
        if fill == "zero":
            for a, b in self._planes(0, self.n):
                self.raw[a:b].zero_()
        elif fill == "rand":
            for a in range(0, self.n, self.CHUNK):
                self._rand(a, min(self.n, a + self.CHUNK))
        else:
            assert fill == "sent", fill

    def _planes(self, a, b):
        """the word ranges of elements a..b in each plane"""
        if self.dt == BF16X3:
            return [(a, b), (self.lo_e + a, self.lo_e + b)]
        return [(a * self.wpe, b * self.wpe)]

    def _rand(self, a, b):
        if self.dt == BF16:
            self.raw[a:b].view(torch.bfloat16).normal_(0.0, self.scale, generator=self.gen)
        elif self.dt == F32:
            self.raw[2 * a:2 * b].view(torch.float32).normal_(0.0, self.scale, generator=self.gen)
        else:
            v = torch.empty(b - a, dtype=torch.float32, device="cuda").normal_(0.0, self.scale, generator=self.gen)
            hi = v.to(torch.bfloat16)
            self.raw[a:b] = hi.view(torch.int16)
            self.raw[self.lo_e + a:self.lo_e + b] = (v - hi.float()).to(torch.bfloat16).view(torch.int16)

    def rand_images(self, images):
        """random values at the listed images (of a zero tensor: the sparse inputs of the kernels whose output is a sum over all images)"""
        for m in images:
            self._rand(m * self.per, (m + 1) * self.per)

    def set_img(self, m, v):
        """image m <- the fp32 CPU values v (exact in dt or not: the kernel's value is what img() reads back)"""
        v = v.contiguous().reshape(-1).cuda()
        assert v.dtype == torch.float32 and v.numel() == self.per
        a, b = m * self.per, (m + 1) * self.per
        if self.dt == F32:
            self.raw[2 * a:2 * b] = v.view(torch.int16)
        else:
            hi = v.to(torch.bfloat16)
            self.raw[a:b] = hi.view(torch.int16)
            if self.dt == BF16X3:
                self.raw[self.lo_e + a:self.lo_e + b] = (v - hi.float()).to(torch.bfloat16).view(torch.int16)

    @property
    def ptr(self):
        return _p(self.raw)

    def _val(self, a, b, shape):
        if self.dt == F32:
            return self.raw[2 * a:2 * b].cpu().view(torch.float32).double().reshape(shape)
        v = self.raw[a:b].cpu().view(torch.bfloat16).double()
        if self.dt == BF16X3:
            v = v + self.raw[self.lo_e + a:self.lo_e + b].cpu().view(torch.bfloat16).double()
        return v.reshape(shape)

    def img(self, m):
        """the exact fp64 CPU value of image m (hi + lo)"""
        assert 0 <= m < self.M
        return self._val(m * self.per, (m + 1) * self.per, self.img_shape)

    def rows(self, m, y0, y1, v=None):
        """rows y0..y1 of image m (img (H, W, C)), or of its view v (img (V, H, W, C)): fp64 (y1 - y0, W, C)"""
        shp = self.img_shape if v is None else self.img_shape[1:]
        row = shp[1] * shp[2]
        base = m * self.per + (0 if v is None else v * shp[0] * row)
        assert 0 <= y0 <= y1 <= shp[0]
        return self._val(base + y0 * row, base + y1 * row, (y1 - y0,) + tuple(shp[1:]))

    def bits(self, m):
        """the raw words of image m, every plane (to compare an input or an untouched slot bit for bit)"""
        return torch.cat([self.raw[a:b].cpu() for a, b in self._planes(m * self.per, (m + 1) * self.per)])

    def checksum(self):
        """a wrapping int64 sum of every word, guards included, computed on the device: equal before and after <=> (for a test) unchanged"""
        return int(self.raw.view(torch.int64).sum())

    def guards_intact(self):
        words = self.n * self.wpe
        if self.dt == BF16X3:
            pieces = [self.raw[self.n:self.lo_e], self.raw[self.lo_e + self.n:]]
        else:
            pieces = [self.raw[words:]]
        return all(bool((p == SENT).all()) for p in pieces)

    def all_sentinels(self):
        return bool((self.raw == SENT).all())


GIB = 1 << 30


class _Pool:
    """the device tensors of one test: freed at teardown whatever happened (a failed test's frames would otherwise keep them alive).
    tests/test_gpu_large_offsets.py and tests/test_gpu_large_offsets_scene.py each build their `pool` fixture from it."""

    def __init__(self):
        self.items = []

    def big(self, *a, **k):
        t = Big(*a, **k)
        self.items.append(t)
        return t

    def keep(self, t):
        self.items.append(t)
        return t

    def free(self):
        for t in self.items:
            if isinstance(t, Big):
                t.raw = None
            else:
                t.untyped_storage().resize_(0)
        self.items = []


def _need(gib):
    import pytest
    free, _ = torch.cuda.mem_get_info()
    if free < gib * GIB:
        pytest.skip(f"needs {gib} GiB of device memory, {free / GIB:.1f} free")


def _sum64(t):
    """a wrapping int64 sum of an f32 device tensor's words (an even count), computed on the device: equal before and after <=> unchanged"""
    return int(t.view(torch.int64).sum())


def _nan_out(pool, n):
    return pool.keep(torch.full((n + 64,), float("nan"), device="cuda"))


def _bits_equal(got, want):
    return np.array_equal(got.cpu().numpy().view(np.uint32), np.ascontiguousarray(want).view(np.uint32))


# ----------------------------------------------------------------------------------------------------------- the registered tail
# tests/test_gpu_kernels_tail.py (GPU) and tests/test_kernels_tail_host.py (CPU): the Lanczos shift, its backward, the loss and score kernels.
# The fp32 kernels (taps, shift, adjoint, tap gradient, loss_backward_kernel) are held to c T like every other family; the kernels that
# accumulate in fp64 (masked_cmse, loss_partial + loss_finish, shift_cpsnr) to a derived bound with no constant in it:
#   a double they store (stats, per-shift scores)   |got - want| <= n 2^-52 T          n = the pixels summed, T = sum |terms| of the value
#   cMSE = (S2 - S1^2 / S0) / S0                     T = (S2 + S1^2 / S0) / S0
#   cPSNR = -10 log10 cMSE                           (10 / ln 10) e / (cMSE - e), e = cMSE's bound: the mean-value form of 10 / (ln 10 cMSE);
#                                                    where cMSE <= 2 e (a window whose cMSE lies within rounding of zero) no cPSNR is determined
#   a float they store                               + 2^-23 |want| for the store and the log10
U64 = 2.0 ** -52
U32 = 2.0 ** -23
# The fp32 kernels of the tail are held to |got - want| <= C_TAIL T, made the way C_F32 was: four times the largest "C needed" any case of
# tests/test_gpu_kernels_tail.py measured on the MI355X against fp64, rounded up to one significant digit.  Measured per family (largest,
# with its case): taps 3.30e-8 at test_taps[63]; lanczos_shift 1.07e-8 at test_lanczos_shift[38x134-b2c3]; d_img 9.76e-9 at
# test_lanczos_shift_backward[5x64-b2c3]; d_shift 3.6e-10 at test_lanczos_shift_backward[7x9-b2c3]; d_srs 1.59e-7 at
# test_get_loss_train_and_backward[65-0-B65-mixed-cMSE] (coef, the bias and three operations: 2.7 roundings of float32).  The largest is
# below C / 4, so the family has its own constant: 4 x 1.59e-7 = 6.4e-7 -> 7e-7.  The float32 restatement of
# tests/test_kernels_tail_host.py needs 3.3e-8 / 1.1e-8 / 1.3e-8 / 1.1e-9 / 1.6e-7 on the CPU.  The taps' own error inside the Lanczos
# bounds is e = C_TAIL T_j as well.  C stays the ceiling: C_TAIL <= C.
C_TAIL = 7e-7
TAIL_MEASURED = (1.59e-7, "test_get_loss_train_and_backward[65-0-B65-mixed-cMSE]")      # (largest C needed, the id of its case)


def cmse_bound(n, S0, S1, S2):
    """the bound of a cMSE whose three sums run over n pixels in fp64"""
    return n * U64 * (S2 + S1 * S1 / S0) / S0


def cpsnr_bound(cmse, e):
    """cMSE's bound e carried through -10 log10; inf where cMSE <= 2 e"""
    ok = cmse > 2 * e
    return torch.where(ok, (10.0 / np.log(10.0)) * e / torch.where(ok, cmse - e, torch.ones_like(cmse)), torch.full_like(cmse, float("inf")))


def _assert_within(tag, got, want, bound, layout="i"):
    """|got - want| <= bound per element, for bounds that are not C T.  Where want is NaN or +-inf, got must be the same; where the bound is
    inf (and want finite) anything passes: the value is not determined.  -> max error / bound"""
    got, want, bound = got.double(), want.double(), bound.double().expand_as(want)
    odd = ~torch.isfinite(want)
    same = torch.where(torch.isnan(want), torch.isnan(got), got == want)
    assert bool(same[odd].all()), (f"{tag}: want {want[odd][~same[odd]][:4].tolist()}, got {got[odd][~same[odd]][:4].tolist()} at "
                                   f"({layout}) = {torch.nonzero(odd & ~same)[:4].tolist()}")
    free = odd | torch.isinf(bound)
    z = torch.zeros_like(want)
    g, w, b = torch.where(free, z, got), torch.where(free, z, want), torch.where(free, z + 1, bound)
    assert bool(torch.isfinite(g).all()), f"{tag}: got a non-finite value at ({layout}) = {torch.nonzero(~torch.isfinite(g))[:4].tolist()}"
    return _assert_close(tag, "f32", g, w, b, layout=layout, c=1.0)


def _within_ratio(got, want, bound):
    """max |got - want| / bound over the elements whose want and bound are finite (a class mismatch counts as inf)"""
    got, want, bound = got.double(), want.double(), bound.double().expand_as(want)
    odd = ~torch.isfinite(want)
    same = torch.where(torch.isnan(want), torch.isnan(got), got == want)
    if not bool(same[odd].all()):
        return float("inf")
    use = ~(odd | torch.isinf(bound))
    r = (got[use] - want[use]).abs() / (bound[use] + 1e-300)
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    return float(r.max()) if r.numel() else 0.0


class Guarded:
    """`shape` elements of `dtype` (float32 / float64) for a kernel to write, inside a device buffer of sentinel bytes: GUARD words in front
    (the kernel gets an offset pointer) and behind.  v: the start values (CPU); otherwise every payload byte is `fill` (0x7F: the sentinel;
    0xFF: NaN in both types, for what a kernel must not read)."""

    def __init__(self, shape, dtype=torch.float32, v=None, fill=SENT & 0xFF):
        self.shape, self.dtype = tuple(shape), dtype
        self.n = int(np.prod(shape))
        self.front = 2 * GUARD                                  # bytes; a multiple of 8
        self.nbytes = self.n * torch.empty((), dtype=dtype).element_size()
        raw = torch.full((self.front + self.nbytes + 2 * GUARD,), SENT & 0xFF, dtype=torch.uint8)
        if v is not None:
            raw[self.front:self.front + self.nbytes] = v.to(dtype).contiguous().reshape(-1).view(torch.uint8)
        else:
            raw[self.front:self.front + self.nbytes] = fill
        self.raw = raw.cuda()

    @property
    def ptr(self):
        import ctypes
        return ctypes.c_void_p(self.raw.data_ptr() + self.front)

    def bits(self):
        """the payload's bytes on the CPU (to compare two runs bit for bit)"""
        return self.raw[self.front:self.front + self.nbytes].cpu()

    def get(self):
        """the payload on the CPU, in its own type"""
        return self.bits().view(self.dtype).reshape(self.shape)

    def guard_ok(self):
        r = self.raw.cpu()
        return bool((r[:self.front] == (SENT & 0xFF)).all()) and bool((r[self.front + self.nbytes:] == (SENT & 0xFF)).all())


# ----------------------------------------------------------------------------------------------------------- the second score, cSSIM
# tests/test_gpu_cssim_pin.py (GPU) and tests/test_cssim_pin_host.py (CPU).  A score of hrn_shift_cssim is held to an absolute bound for
# data in [0, 1] with data_range = 1: CSSIM_BOUND is the project's cap, CSSIM_TOL_PIN the pinning pass's bound, made
# the way C_F32 was: four times the largest |GPU - fp64 restatement| any case of the pinning pass measured on the MI355X, rounded up to one
# significant digit, never above the cap: 4 x 9.73e-8 = 3.9e-7 -> 4e-7.  CSSIM_MEASURED: the largest per family, with its case.
# CSSIM_MEASURED_UNCENTRED: the same cases on the tile kernel as it shipped (v = cov_norm (G X^2 - mu^2) on uncentred fields), in the same
# session - 23 of the 40 conditioning cases, every clear instance case and every clear seam case beyond the cap - which is why the tile
# kernel centres its fields per tile now.
CSSIM_BOUND = 1e-5
CSSIM_TOL_PIN = 4e-7
CSSIM_MEASURED = {"conditioning": (4.41e-8, "cond-24x24-uniform-L0.05-c0.05-clear"),
                  "instances": (9.73e-8, "test_all_eighteen_instances_launch: border 8, uniform, 25 x 27"),
                  "seams": (2.32e-8, "seam-45x129-uniform-clear"),
                  "runs": (1.44e-8, "runs-2050-uniform")}
CSSIM_MEASURED_UNCENTRED = {"conditioning": (1.04e-4, "cond-24x24-gaussian-L0.9-c0.005-clear"),
                            "instances": (6.78e-5, "inst-b5-uniform-clear"),
                            "seams": (4.69e-5, "seam-45x129-uniform-clear"),
                            "runs": (1.51e-7, "runs-2048-uniform")}

# ------------------------------------------------------------------------------------ masked-NCC scores off the frame's mean
# tests/test_gpu_registration_pin.py (GPU) and tests/test_registration_pin_host.py (CPU): frames with a level step, a contrast of 0.01 and
# a mask that keeps one side in one image (tests/registration_cases.py, which also holds the bounds: the registration tests' own 4e-7 of
# a device score against the fp64 restatement and 8e-7 between two device paths, DESIGN.md sections 7f, 7g).  Only measurements here.
# MNCC_PIN_MEASURED: the largest |device - fp64| per family on the MI355X, with its case, of the level kernels as they are - the five
# per-pixel sums in fp64; every case is admitted at 1e-7 on the CPU model at every compared point, and the resident figure is the
# model's own for that case (fp32 resampling with exact sums).  MNCC_PIN_MEASURED_FP32_SUMS: the same cases in the same session on the
# kernels as they shipped (a thread's 16 / 32 pixels added in fp32 on images centred on whole-frame means): 98 of the 150 tests
# failed, every one of the 38 conditioning cases among them and no control - which is why the sums are fp64 now.
MNCC_PIN_MEASURED = {"resident": (9.81e-8, "grid resident-24x40-c0.01-s0.6-col20-ref-hides"),
                     "scene": (7.33e-8, "grid_scene scene-130x203-c0.01-s0.6-col100-ref-hides speckle"),
                     "local": (3.00e-8, "local trace local-130x203-c0.01-s0.3-col128-both-sides null"),
                     "pyramid": (4.17e-8, "pyramid trace pyramid-130x203-c0.01-s0.6-col128-ref-hides speckle")}
MNCC_PIN_MEASURED_FP32_SUMS = {"resident": (2.01e-5, "grid resident-24x40-c0.01-s0.6-col20-view-hides"),
                               "scene": (7.41e-6, "search_scene scene-128x128-c0.01-s0.6-col64-ref-hides null"),
                               "local": (1.35e-5, "local trace local-130x203-c0.01-s0.6-col128-both-sides speckle"),
                               "pyramid": (7.28e-6, "pyramid trace pyramid-130x203-c0.01-s0.6-col128-ref-hides null")}
