"""GPU (-m gpu): the scene, loss, resampling, ensemble, tiling and collate kernels where offsets pass 2^31 bytes, 2^32 bytes and 2^31
elements - the kernels added after HRNet's own, which tests/test_gpu_large_offsets.py does not reach.  Calls go through the public C ABI
with ctypes (binding.load_library()).  tests/large_offsets_cases.py holds the cases (tests/test_large_offsets_host.py shows on the CPU
that each crosses what its id names and stays inside the entry point's guards); DESIGN.md section "Offsets past 2^31 and 2^32" holds the
table of offset widths.

Every input is generated on the device from a seed, chunk by chunk (Big.CHUNK elements) from one generator, so that the data are not
periodic in 2^32 bytes; every output is prefilled with NaN (or a sentinel) with 64 spare words behind it that must still hold it
afterwards; inputs are checksummed before and after the launch; only the checked planes, rows or windows reach the host.

A  deep batch   many small planes (64 x 64; 33 x 50, which no tile, run or vector width divides; 192 x 192 / 181 x 203 / 128 x 256 where a
                guard caps the batch at 65535).  Checked: plane 0, the last plane and the plane(s) at every crossing of every tensor of
                the launch (kernel_bounds.boundary_images; large_offsets_cases.checked_planes).  The check: the result at a checked plane is
                BIT-IDENTICAL to the same entry point called on that plane (for a view stack: that sample) alone, on fresh small copies
                of its inputs - these kernels promise batch independence - and the alone result meets the fp64 restatement under the
                bound of the kernel's own
                small-shape test, imported from that test's helper module.  The pure data movers (hrn_dihedral_*, hrn_collate_device*)
                are compared bit for bit against their restatements directly.
B  big frame    few planes near an entry point's own limit.  The local kernels (apply_scene, d_views, apply_field, reduce2 on (1, V) planes
                of 16002 x 16001, V = 5 with masks / V = 9 without; the Lanczos shift and its d_img on one plane of 33000 x 33001): strips of
                24 rows - top, middle, bottom, and around the row of each crossing - against the fp64 restatement of the strip with its
                real neighbour rows, under the small-shape bound; valid exactly.  The kernels whose result is a sum over the frame
                (grid_scene, search_scene, d_shifts; the three losses' forward, with their elementwise backward): the mask that gates the
                sum (ref_mask; valid; maps) is zero except in the checked blocks or strips, so the result depends on those pixels alone
                and the reference is the restatement of the stacked blocks or strips; a kernel that reads a wrapped offset sees masked or
                different pixels.  hrn_shift_cssim also at the int limit of cssim.hip, 46340 x 46340.  hrn_tile_gather on (1, 9) planes of
                16002 x 16001 and hrn_tile_scatter x3 into one plane of 36000 x 36003, bit for bit against tiling.gather / tiling.scatter at
                the first window, the last window and the windows at every crossing; the smallest refused shapes of hrn_tile_scatter and
                hrn_shift_cssim return -2 and write nothing.
Negative controls (apply_scene A, the searched loss A, tile gather B, collate): at every checked plane past byte 2^32 the comparison must
reject what a base truncated to 32 bits would address, plane m - 2^32 / plane bytes: more than half the pixels differ in bits, or error /
bound > 1.  The sparse-mask cases have a second one: the restatement with the strips or blocks past byte 2^32 read 2^32 bytes lower must
not meet the output.

Where a case's id says 2^32B and not 2^31el, its docstring (or tests/large_offsets_cases.py) says why: four or more tensors of 8 GiB do
not fit the 32 GiB cap, or a guard caps the batch.

Every tensor of a test is registered with the `pool` fixture, which frees it whatever the outcome, prints the test's peak device memory
and holds it to 32 GiB.  Peak memory and wall time per test on the MI355X: DESIGN.md, the same section."""
import ctypes
import gc

import numpy as np
import pytest
import torch

import large_offsets_cases as LC
from kernel_bounds import C, GIB, Big, _assert_close, _bits_equal, _nan_out, _need, _Pool, _sum64, crossed

pytestmark = pytest.mark.gpu

SPARE = 64
NULL = ctypes.c_void_p(0)


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
    assert peak <= LC.CAP_GIB * GIB, f"{peak / GIB:.1f} GiB held at once"


def _lib():
    from hrnet_hip import binding
    return binding.load_library()


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _ok(lib, rc):
    assert rc == 0, (rc, lib.hrn_last_error())
    torch.cuda.synchronize()


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _fill(pool, n, gen, kind, a=0.0, b=1.0):
    """n f32 on the device, in chunks from `gen`, and SPARE (+ n & 1: the checksum reads pairs) NaN words behind them.  kind: "uniform" in
    [a, b); "normal"; "mask": 0 with probability a, else 1"""
    t = pool.keep(torch.empty(n + SPARE + (n & 1), device="cuda"))
    t[n:] = float("nan")
    for lo in range(0, n, Big.CHUNK):
        c = t[lo:min(n, lo + Big.CHUNK)]
        if kind == "normal":
            c.normal_(generator=gen)
        else:
            c.uniform_(generator=gen)
            if kind == "mask":
                c.gt_(a)
            elif (a, b) != (0.0, 1.0):
                c.mul_(b - a).add_(a)
    return t


def _spare_ok(t, n):
    return bool(torch.isnan(t[n:]).all())


def _says(tag, cross, tensors, checked):
    """print what each tensor crosses and what is checked; the largest must cross what the case id says, and at least five planes are
    checked"""
    got = {name: crossed(n, 4) for name, n in tensors.items()}
    print(f"{tag}: " + ", ".join(f"{name} {n * 4 / GIB:.2f} GiB {got[name]}" for name, n in tensors.items()) + f"; checked {checked}")
    largest = max(tensors, key=tensors.get)
    assert cross in got[largest] and (cross == "2^31el" or "2^31el" not in got[largest]), (tag, cross, got)
    assert len(checked) >= 5, (tag, checked)


_planes = LC.checked_planes


def _differ(a, b):
    """how many words of two equally shaped f32 arrays / tensors differ in bits"""
    a = a.cpu().numpy() if torch.is_tensor(a) else np.ascontiguousarray(a, np.float32)
    b = b.cpu().numpy() if torch.is_tensor(b) else np.ascontiguousarray(b, np.float32)
    return int((a.view(np.uint32) != b.view(np.uint32)).sum())


def _wrap_planes(per):
    """2^32 bytes as a whole number of planes of `per` f32 elements, or None"""
    return (1 << 30) // per if (1 << 30) % per == 0 else None


# ----------------------------------------------------------------------------------------------------------- hrn_mncc_apply_scene
def _shifts(B, V):
    """(B, V, 2): the views cycle through warp_ref.SHIFTS - whole pixels, negative values, "nothing valid" - by their plane index"""
    import warp_ref as WR
    idx = torch.arange(B * V) % len(WR.SHIFTS)
    return torch.tensor(WR.SHIFTS, dtype=torch.float32)[idx].reshape(B, V, 2).contiguous()


def _apply(lib, views, masks, shifts, B, V, H, W, out, valid):
    _ok(lib, lib.hrn_mncc_apply_scene(_p(views), _p(masks) if masks is not None else NULL, _p(shifts), B, V, H, W, _p(out), _p(valid), NULL))


def _apply_alone(pool, lib, views, masks, shifts, b, V, H, W):
    """sample b alone: fresh copies of its inputs, fresh NaN outputs -> (out, valid) (V, H, W) on the device, and the copies"""
    per = V * H * W
    v1 = views[b * per:(b + 1) * per].clone()
    m1 = masks[b * per:(b + 1) * per].clone() if masks is not None else None
    s1 = shifts[b:b + 1].clone()
    o1, k1 = torch.full((per + SPARE,), float("nan"), device="cuda"), torch.full((per + SPARE,), float("nan"), device="cuda")
    _apply(lib, v1, m1, s1, 1, V, H, W, o1, k1)
    assert _spare_ok(o1, per) and _spare_ok(k1, per)
    return o1[:per].view(V, H, W), k1[:per].view(V, H, W), v1.view(V, H, W), (m1.view(V, H, W) if m1 is not None else None)


def _apply_against_fp64(tag, out1, valid1, v1, m1, shifts_b):
    """the alone result against tests/registration_ref.py under test_gpu_registration_scene.py's APPLY_BOUND: valid exactly, out within
    the bound where valid and exactly 0 elsewhere -> the worst error"""
    import registration_ref as R
    from registration_cases import APPLY_BOUND
    V, H, W = out1.shape
    out1, valid1, v1 = out1.cpu().numpy(), valid1.cpu().numpy(), v1.cpu().numpy()
    m1 = m1.cpu().numpy() if m1 is not None else None
    worst = 0.0
    for v in range(V):
        s = shifts_b[v].numpy()
        m = np.ones((H, W)) if m1 is None else m1[v]
        off = np.abs(R.mask_bilinear(m, s) - 0.5)
        assert not ((off > 0.0) & (off <= 1e-9)).any(), f"{tag}: a mask sample within rounding of 0.5"
        want_valid = R.shifted_mask(m, s)
        assert np.array_equal(valid1[v], want_valid.astype(np.float32)), f"{tag} view {v}: valid"
        assert np.all(out1[v][~want_valid] == 0.0)
        if want_valid.any():
            worst = max(worst, float(np.abs(out1[v] - R.sample(v1[v], s))[want_valid].max()))
    assert worst <= APPLY_BOUND, (tag, worst)
    return worst


APPLY_IDS = [f"{a}-{b}-{c}" for a, b, c in LC.APPLY_A]


@pytest.mark.parametrize("masks,shape,cross", LC.APPLY_A, ids=APPLY_IDS)
def test_apply_scene_deep_batch(pool, masks, shape, cross):
    """hrn_mncc_apply_scene, regime A: out and out_valid at the checked samples, bit for bit against the sample alone; the sample alone
    against fp64.  With masks the launch has four tensors of one size (32 GiB at 2^31 elements: the cap), so that case stops past 2^32
    bytes.  Control (64 x 64): at the checked samples past byte 2^32, the alone result of sample b - 2^32 / sample bytes is rejected"""
    case = LC.apply_case(masks, shape, cross)
    B, V, H, W, per = (case[k] for k in ("B", "V", "H", "W", "per"))
    _need(LC.gib(case["tensors"]))
    lib = _lib()
    g = _gen(301)
    views = _fill(pool, B * per, g, "uniform")
    vm = _fill(pool, B * per, g, "mask", 0.15) if masks == "masks" else None
    shifts = _shifts(B, V)
    sd = shifts.cuda()
    out, valid = _nan_out(pool, B * per), _nan_out(pool, B * per)
    sums = [(t, _sum64(t)) for t in (views, vm) if t is not None]
    _apply(lib, views, vm, sd, B, V, H, W, out, valid)
    assert all(_sum64(t) == c for t, c in sums) and torch.equal(sd.cpu(), shifts), "the launch wrote one of its inputs"
    assert _spare_ok(out, B * per) and _spare_ok(valid, B * per), "a write past an output"
    bs = _planes((B, per))
    tag = f"apply_scene {masks} {shape} B={B}"
    _says(tag, cross, case["tensors"], bs)
    wrap = _wrap_planes(per)
    told = 0
    for b in bs:
        o1, k1, v1, m1 = _apply_alone(pool, lib, views, vm, sd, b, V, H, W)
        g_out, g_valid = out[b * per:(b + 1) * per].view(V, H, W), valid[b * per:(b + 1) * per].view(V, H, W)
        assert _differ(g_out, o1) == 0 and _differ(g_valid, k1) == 0, f"{tag}: sample {b} differs from its launch alone"
        worst = _apply_against_fp64(f"{tag} sample {b}", o1, k1, v1, m1, shifts[b])
        print(f"{tag} sample {b}: bit-identical to the sample alone; alone against fp64 {worst:.3e}")
        if wrap is not None and b >= wrap:
            # the views (and masks) a 32-bit byte base would address, under this sample's shifts: the same entry point, alone
            lo = (b - wrap) * per
            w1 = views[lo:lo + per].clone()
            wm = vm[lo:lo + per].clone() if vm is not None else None
            wo, wk = torch.full((per + SPARE,), float("nan"), device="cuda"), torch.full((per + SPARE,), float("nan"), device="cuda")
            _apply(lib, w1, wm, sd[b:b + 1].clone(), 1, V, H, W, wo, wk)
            live = int((k1 != 0).sum())
            d = int(((g_out.reshape(-1) != wo[:per]) & (k1.reshape(-1) != 0)).sum())
            print(f"{tag} sample {b} against the views of sample {b - wrap}: {d} of {live} valid pixels differ")
            if live:
                assert d > live // 2, f"the comparison does not tell sample {b - wrap} from sample {b}"
                told += 1
    assert wrap is None or told >= 1


# ----------------------------------------------------------------------------------------------------------- hrn_mncc_apply_backward
BACKWARD_IDS = [f"{a}-{b}-{c}" for a, b, c in LC.BACKWARD_A]


def _backward(lib, views, shifts, valid, d_out, B, V, H, W, d_views, d_shifts):
    nbytes = lib.hrn_mncc_apply_backward_workspace_bytes(B, V, H, W)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device="cuda")
    _ok(lib, lib.hrn_mncc_apply_backward(_p(views) if views is not None else NULL, _p(shifts), _p(valid), _p(d_out), B, V, H, W, _p(d_views),
                                         _p(d_shifts) if d_shifts is not None else NULL, _p(ws), nbytes, NULL))


@pytest.mark.parametrize("which,shape,cross", LC.BACKWARD_A, ids=BACKWARD_IDS)
def test_apply_backward_deep_batch(pool, which, shape, cross):
    """hrn_mncc_apply_backward, regime A: d_views and d_shifts (both halves launched) with `valid` from the forward of the same tensors and
    the forward's `out` as the gradient that arrives - five tensors of one size, so past 2^32 bytes; and d_views alone past 2^31 elements
    (that half needs no `views`: they are freed after the forward).  Bit for bit against the sample alone, the sample alone against
    tests/warp_ref.py under test_gpu_warp.py's bounds"""
    import warp_ref as WR
    case = LC.backward_case(which, shape, cross)
    B, V, H, W, per = (case[k] for k in ("B", "V", "H", "W", "per"))
    _need(LC.gib({k: B * per for k in range(case["held"])}))
    lib = _lib()
    g = _gen(311)
    views = _fill(pool, B * per, g, "uniform")
    vm = _fill(pool, B * per, g, "mask", 0.15) if which == "both" else None
    shifts = _shifts(B, V)
    sd = shifts.cuda()
    d_out, valid = _nan_out(pool, B * per), _nan_out(pool, B * per)
    _apply(lib, views, vm, sd, B, V, H, W, d_out, valid)
    bs = _planes((B, per))
    if which == "d_views":                                   # keep the checked samples' views for the restatement, free the rest
        kept = {b: views[b * per:(b + 1) * per].clone() for b in bs}
        views.untyped_storage().resize_(0)
        views = None
    d_views = _nan_out(pool, B * per)
    d_shifts = torch.full((B * V * 2 + SPARE,), float("nan"), device="cuda") if which == "both" else None
    sums = [(t, _sum64(t)) for t in (views, valid, d_out) if t is not None]
    _backward(lib, views, sd, valid, d_out, B, V, H, W, d_views, d_shifts)
    assert all(_sum64(t) == c for t, c in sums) and torch.equal(sd.cpu(), shifts), "the launch wrote one of its inputs"
    assert _spare_ok(d_views, B * per) and (d_shifts is None or _spare_ok(d_shifts, B * V * 2)), "a write past an output"
    tag = f"apply_backward {which} {shape} B={B}"
    _says(tag, cross, case["tensors"], bs)
    for b in bs:
        sl = slice(b * per, (b + 1) * per)
        v1 = views[sl].clone() if views is not None else None
        k1, g1, s1 = valid[sl].clone(), d_out[sl].clone(), sd[b:b + 1].clone()
        dv1 = torch.full((per + SPARE,), float("nan"), device="cuda")
        ds1 = torch.full((V * 2 + SPARE,), float("nan"), device="cuda") if which == "both" else None
        _backward(lib, v1, s1, k1, g1, 1, V, H, W, dv1, ds1)
        assert _spare_ok(dv1, per) and _differ(d_views[sl], dv1[:per]) == 0, f"{tag}: d_views of sample {b} differs from its launch alone"
        if ds1 is not None:
            assert _differ(d_shifts[b * V * 2:(b + 1) * V * 2], ds1[:V * 2]) == 0, f"{tag}: d_shifts of sample {b} differs from its launch alone"
        T = (v1 if v1 is not None else kept[b]).view(V, H, W).cpu().numpy()
        kn, gn = k1.view(V, H, W).cpu().numpy(), g1.view(V, H, W).cpu().numpy()
        got_dv = dv1[:per].view(V, H, W).cpu().double()
        for v in range(V):
            s = shifts[b, v].numpy()
            mag_v, mag_s = WR.magnitudes(T[v], gn[v], kn[v], s)
            r = _assert_close(f"{tag} d_views sample {b} view {v}", "f32", got_dv[v], torch.from_numpy(WR.d_views(gn[v], kn[v], s)),
                              torch.from_numpy(mag_v), layout="y x")
            if ds1 is not None:
                want = WR.d_shifts(T[v], gn[v], kn[v], s)
                got = ds1[2 * v:2 * v + 2].cpu().numpy().astype(np.float64)
                bound = 2.0 ** -24 * np.abs(want) + C * mag_s
                assert np.all(np.abs(got - want) <= bound), (tag, b, v, got, want, bound)
        print(f"{tag} sample {b}: bit-identical to the sample alone; alone d_views error / bound {r:.3e}")


# ----------------------------------------------------------------------------------------------------------- hrn_mncc_reduce2
REDUCE_IDS = [f"{a}-{b}-{c}" for a, b, c in LC.REDUCE_A]


def _reduce(lib, x, mask, N, H, W, out, om):
    _ok(lib, lib.hrn_mncc_reduce2(_p(x), _p(mask) if mask is not None else NULL, N, H, W, _p(out), _p(om), NULL))


@pytest.mark.parametrize("masks,shape,cross", LC.REDUCE_A, ids=REDUCE_IDS)
def test_reduce2_deep_batch(pool, masks, shape, cross):
    """hrn_mncc_reduce2, regime A: x (and its mask) past 2^31 elements, out and out_mask a quarter of that (past 2^31 bytes): the checked
    planes are the union of both tensors' boundary planes.  Bit for bit against the plane alone; the plane alone against
    tests/registration_pyramid_ref.py under its REDUCE2_BOUND, the coarse mask exactly"""
    import registration_pyramid_ref as Y
    case = LC.reduce_case(masks, shape, cross)
    N, H, W = case["N"], case["H"], case["W"]
    hw, q = H * W, (H // 2) * (W // 2)
    _need(LC.gib(case["tensors"]))
    lib = _lib()
    g = _gen(321)
    x = _fill(pool, N * hw, g, "uniform")
    mask = _fill(pool, N * hw, g, "mask", 0.35) if masks == "masks" else None
    out, om = _nan_out(pool, N * q), _nan_out(pool, N * q)
    sums = [(t, _sum64(t)) for t in (x, mask) if t is not None]
    _reduce(lib, x, mask, N, H, W, out, om)
    assert all(_sum64(t) == c for t, c in sums), "the launch wrote one of its inputs"
    assert _spare_ok(out, N * q) and _spare_ok(om, N * q), "a write past an output"
    ns = _planes((N, hw), (N, q))
    tag = f"reduce2 {masks} {shape} N={N}"
    _says(tag, cross, case["tensors"], ns)
    for n in ns:
        x1 = x[n * hw:(n + 1) * hw].clone()
        m1 = mask[n * hw:(n + 1) * hw].clone() if mask is not None else None
        o1, k1 = torch.full((q + SPARE,), float("nan"), device="cuda"), torch.full((q + SPARE,), float("nan"), device="cuda")
        _reduce(lib, x1, m1, 1, H, W, o1, k1)
        assert _spare_ok(o1, q) and _spare_ok(k1, q)
        assert _differ(out[n * q:(n + 1) * q], o1[:q]) == 0 and _differ(om[n * q:(n + 1) * q], k1[:q]) == 0, f"{tag}: plane {n} differs from its launch alone"
        want, clear, _ = Y.reduce2(x1.view(H, W).cpu().numpy(), m1.view(H, W).cpu().numpy() if m1 is not None else None)
        got, got_clear = o1[:q].view(H // 2, W // 2).cpu().numpy(), k1[:q].view(H // 2, W // 2).cpu().numpy()
        assert np.array_equal(got_clear, clear.astype(np.float32)) and np.all(got[~clear] == 0.0)
        worst = float(np.abs(got.astype(np.float64) - want).max())
        print(f"{tag} plane {n}: bit-identical to the plane alone; alone against fp64 {worst:.3e}")
        assert worst <= Y.REDUCE2_BOUND


# ----------------------------------------------------------------------------------------------------------- hrn_shift_loss_*
LOSS_IDS = [f"{a}-border{b}-{c}{'-clip' if d else ''}{'-bwd' if e else ''}-{f}" for a, b, c, d, e, f in LC.LOSS_A]
METRIC = {"cMSE": 1, "cPSNR": 2}
D_OUT = (1.0, -0.5, 2.0)


def _loss(lib, srs, hrs, maps, B, H, W, border, metric, clip, d_out, d_srs):
    """forward (and, with d_srs, backward with the forward's stats) -> (out (B + SPARE) f32, stats (B, 4) f64)"""
    nbytes = lib.hrn_shift_loss_workspace_bytes(B, H, W, border)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    out = torch.full((B + SPARE,), float("nan"), device="cuda")
    stats = torch.full((B * 4 + SPARE,), float("nan"), dtype=torch.float64, device="cuda")
    _ok(lib, lib.hrn_shift_loss_train(_p(srs), _p(hrs), _p(maps), B, H, W, border, METRIC[metric], int(clip), _p(out), _p(stats), _p(ws), nbytes, NULL))
    assert _spare_ok(out, B) and _spare_ok(stats, 4 * B)
    if d_srs is not None:
        _ok(lib, lib.hrn_shift_loss_backward(_p(srs), _p(hrs), _p(maps), _p(stats), _p(d_out), B, H, W, border, METRIC[metric], int(clip), _p(d_srs), NULL))
    del ws
    return out, stats


@pytest.mark.parametrize("shape,border,metric,clip,backward,cross", LC.LOSS_A, ids=LOSS_IDS)
def test_shift_loss_deep_batch(pool, shape, border, metric, clip, backward, cross):
    """hrn_shift_loss_train / _backward, regime A: the losses, stats and d_srs of the checked samples, bit for bit against the sample
    alone; the sample alone against tests/shift_loss_ref.py under test_gpu_shift_loss.py's tolerances.  The batch is capped at 65535, so
    the planes are 192 x 192 (2^31 elements, the forward alone: a fourth tensor of 8 GiB does not fit the cap beside the workspace) and
    181 x 203 / 128 x 256 with the backward, past 2^32 bytes.  Control (128 x 256, where 2^32 bytes are 32768 samples): the restatement of
    sample b - 32768 is rejected by both tolerances"""
    import shift_loss_ref as R
    import util
    case = LC.loss_case(shape, border, metric, clip, backward, cross)
    B, H, W = case["B"], case["H"], case["W"]
    hw = H * W
    lib = _lib()
    ws_bytes = lib.hrn_shift_loss_workspace_bytes(B, H, W, border)
    _need(LC.gib(case["tensors"], ws_bytes))
    g = _gen(331)
    lo, hi = (-0.2, 1.2) if clip else (0.0, 1.0)
    srs, hrs, maps = _fill(pool, B * hw, g, "uniform", lo, hi), _fill(pool, B * hw, g, "uniform"), _fill(pool, B * hw, g, "mask", 0.1)
    d_out = torch.tensor(D_OUT, device="cuda")[torch.arange(B, device="cuda") % 3].contiguous()
    d_srs = _nan_out(pool, B * hw) if backward else None
    sums = [(t, _sum64(t)) for t in (srs, hrs, maps)]
    out, stats = _loss(lib, srs, hrs, maps, B, H, W, border, metric, clip, d_out, d_srs)
    pool.keep(out), pool.keep(stats)
    assert all(_sum64(t) == c for t, c in sums), "a launch wrote one of its inputs"
    assert d_srs is None or _spare_ok(d_srs, B * hw), "a write past d_srs"
    bs = _planes((B, hw))
    tag = f"shift_loss {shape} border {border} {metric} B={B} workspace {ws_bytes / GIB:.2f} GiB"
    _says(tag, cross, case["tensors"], bs)
    wrap = _wrap_planes(hw)
    told = 0

    def restated(b):
        x = tuple(t[b * hw:(b + 1) * hw].view(1, H, W).cpu() for t in (srs, hrs, maps))
        s = x[0].double().requires_grad_(True)
        want, k, cm = R.shift_loss(s, x[1], x[2], metric, border, clip)
        (want * D_OUT[b % 3]).sum().backward()
        return want.detach(), k, cm, s.grad

    def errors(b, want, grad):
        e = util.rel_err(out[b:b + 1].cpu().numpy(), want.numpy())
        if d_srs is None:
            return e, 0.0
        got = d_srs[b * hw:(b + 1) * hw].view(1, H, W).cpu().double()
        return e, float((got - grad).abs().amax()) / float(grad.abs().amax())

    for b in bs:
        one = tuple(t[b * hw:(b + 1) * hw].clone() for t in (srs, hrs, maps))
        d1 = torch.full((hw + SPARE,), float("nan"), device="cuda") if backward else None
        out1, stats1 = _loss(lib, *one, 1, H, W, border, metric, clip, d_out[b:b + 1].clone(), d1)
        assert _differ(out[b:b + 1], out1[:1]) == 0 and torch.equal(stats[4 * b:4 * b + 4].view(torch.int64), stats1[:4].view(torch.int64)), \
            f"{tag}: sample {b} differs from its launch alone"
        if backward:
            assert _spare_ok(d1, hw) and _differ(d_srs[b * hw:(b + 1) * hw], d1[:hw]) == 0, f"{tag}: d_srs of sample {b} differs from its launch alone"
        want, k, cm, grad = restated(b)
        assert float(R.top_two_gap(cm).min()) > 1e-6 and int(stats[4 * b + 3]) == int(k[0])
        e, eg = errors(b, want, grad)
        print(f"{tag} sample {b}: bit-identical to the sample alone; against fp64: rel err {e:.2e}, d_srs err / max-norm {eg:.2e}")
        assert e <= R.TOL and eg <= R.GRAD_TOL
        if backward and border:
            frame = torch.ones((H, W), dtype=torch.bool)
            frame[border:-border, border:-border] = False
            assert bool((d_srs[b * hw:(b + 1) * hw].view(H, W).cpu()[frame] == 0).all())
        if wrap is not None and b >= wrap:
            w_want, _, _, w_grad = restated(b - wrap)
            e, eg = errors(b, w_want, w_grad * (D_OUT[b % 3] / D_OUT[(b - wrap) % 3]))
            print(f"{tag} sample {b} against the restatement of sample {b - wrap}: rel err / TOL {e / R.TOL:.3e}, d_srs err / GRAD_TOL {eg / R.GRAD_TOL:.3e}")
            assert e > R.TOL and (not backward or eg > R.GRAD_TOL), f"the comparison does not tell sample {b - wrap} from sample {b}"
            told += 1
    assert wrap is None or told >= 1


# ----------------------------------------------------------------------------------------------------------- hrn_dihedral_*
DIHEDRAL_IDS = [f"{a}-{b}-K{len(c)}-2^31el" for a, b, c in LC.DIHEDRAL]


@pytest.mark.parametrize("path,shape,codes", LC.DIHEDRAL, ids=DIHEDRAL_IDS)
def test_dihedral_deep(pool, path, shape, codes):
    """hrn_dihedral_expand / hrn_dihedral_mean with member_elems > 2^31 / K: the last member of the (K, N, H, W) stack lies past element
    2^31.  Bit for bit against hrnet_hip/augment.py (the restatement of tests/test_gpu_ensemble.py) at plane 0, the last plane and the
    planes at the stack's crossings, for the first member, a middle one and the last; the mean reads a stack of fresh random values"""
    from hrnet_hip import augment
    case = LC.dihedral_case(path, shape, codes)
    N, K, H, W = case["N"], case["K"], case["H"], case["W"]
    hw, me = H * W, case["member_elems"]
    _need(LC.gib(case["tensors"]))
    lib = _lib()
    g = _gen(341)
    x = _fill(pool, me, g, "normal")
    stack, mean = _nan_out(pool, K * me), _nan_out(pool, me)
    assert (W % 4 == 0 and x.data_ptr() % 16 == 0 and stack.data_ptr() % 16 == 0) == (path == "vec")
    carr = (ctypes.c_int32 * K)(*codes)
    c0 = _sum64(x)
    _ok(lib, lib.hrn_dihedral_expand(_p(x), N, H, W, carr, K, _p(stack), NULL))
    assert _sum64(x) == c0 and _spare_ok(stack, K * me), "expand wrote its input or past its output"
    planes = _planes((K * N, hw))                            # of the stack: (member, plane) = divmod(., N)
    ns = sorted({0, N - 1} | {p % N for p in planes})
    members = sorted({0, K // 2 - 1 if K == 8 else 1, K - 1})
    tag = f"dihedral {path} {shape} K={K} N={N}"
    _says(tag, "2^31el", case["tensors"], [(k, n) for k in members for n in ns])
    assert (K - 1) * me < 1 << 31 < K * me               # the crossing lies inside the last member
    for k in members:
        for n in ns:
            got = stack[k * me + n * hw:k * me + (n + 1) * hw].view(H, W)
            want = augment.apply(x[n * hw:(n + 1) * hw].view(H, W), codes[k])
            assert _differ(got, want.contiguous()) == 0, f"{tag}: expand member {k} (code {codes[k]}) plane {n}"
    # the mean of a stack of fresh values (the members of an expanded x would all be x itself)
    for lo in range(0, K * me, Big.CHUNK):
        stack[lo:min(K * me, lo + Big.CHUNK)].normal_(generator=g)
    c0 = _sum64(stack)
    _ok(lib, lib.hrn_dihedral_mean(_p(stack), N, H, W, carr, K, _p(mean), NULL))
    assert _sum64(stack) == c0 and _spare_ok(mean, me), "mean wrote its input or past its output"
    for n in ns:
        y = torch.stack([stack[k * me + n * hw:k * me + (n + 1) * hw].view(H, W) for k in range(K)])
        want = augment.mean_inverse(y, list(codes))
        assert _differ(mean[n * hw:(n + 1) * hw].view(H, W), want.contiguous()) == 0, f"{tag}: mean plane {n}"
        # the last member counts: without it the mean is another
        other = augment.mean_inverse(torch.cat([y[:-1], y[:1]]), list(codes))
        assert _differ(want.contiguous(), other.contiguous()) > hw // 2
    print(f"{tag}: expand members {members} and the mean bit-identical to the rule at planes {ns}")


# ----------------------------------------------------------------------------------------------------------- hrn_collate_device(_m)
@pytest.mark.parametrize("S", LC.COLLATE_S, ids=[f"S{s}-2^31el" for s in LC.COLLATE_S])
def test_collate_deep_arena(pool, S):
    """hrn_collate_device and hrn_collate_device_m on an LR arena of 2^31 + 1024 uint16 (4 GiB) and a QM arena of the same length: a
    hand-written plan whose rows point at stored images at offset 0, on either side of element 2^30 (byte 2^31), on either side of element
    2^31 (byte 2^32) and at the last image, codes 0, 3 and 5, S = 4 (16-byte path) and 6 (per element).  Bit for bit against the value
    rule of test_bad_plan_rows_give_nan_planes; an odd-sided image that ends three elements inside the arena is exact, one that ends ONE
    element past it is NaN.  Control: the window a 32-bit byte base would address (offset - 2^31 elements) is told from the output"""
    from hrnet_hip import augment, binding
    L, rows = LC.collate_case()
    _need((2 * L + L) / GIB + 2)
    lib = _lib()
    M, min_L, scale = binding.COLLATE_META, 2, 3
    r, c = LC.COLLATE_CORNER
    g = _gen(351 + S)
    lr = pool.keep(torch.empty(L, dtype=torch.int16, device="cuda"))
    qm = pool.keep(torch.empty(L, dtype=torch.uint8, device="cuda"))
    for lo in range(0, L, Big.CHUNK):
        lr[lo:lo + Big.CHUNK].random_(generator=g)           # 0 .. 32767
        qm[lo:lo + Big.CHUNK].random_(0, 3, generator=g)
    hside = scale * LC.COLLATE_SIDE
    hr = torch.empty(2 * hside * hside, dtype=torch.int16, device="cuda").random_(generator=g)
    sm = torch.empty(2 * hside * hside, dtype=torch.uint8, device="cuda").random_(0, 3, generator=g)
    B = len(rows)
    plan_rows = [[(b % 2) * hside * hside if side == LC.COLLATE_SIDE else -1, (b % 2) * hside * hside if side == LC.COLLATE_SIDE else 0, side, r, c] + offs
                 for b, (side, offs, _) in enumerate(rows)]
    # an odd-sided row's SM image would be 39 x 39 = 1521 elements from offset 0: inside the SM arena; its HR plane is absent (zeros)
    plan = torch.tensor(plan_rows, dtype=torch.int64, device="cuda")
    assert plan.shape == (B, M + min_L)
    codes = torch.tensor([LC.COLLATE_CODES[b % 3] for b in range(B)], dtype=torch.int32)
    cd = codes.cuda()
    u16 = lambda t: t.cpu().numpy().view(np.uint16)
    f = lambda u: (u.astype(np.float64) / 65535.0).astype(np.float32)
    print(f"collate S={S}: LR arena {L} uint16 = {2 * L / GIB:.2f} GiB {crossed(L, 2)}, QM arena {L / GIB:.2f} GiB {crossed(L, 1)}; offsets "
          f"{[o for _, offs, _ in rows for o in offs]}")
    assert "2^31el" in crossed(L, 2) and "2^32B" in crossed(L, 2) and sum(len(offs) for _, offs, _ in rows) >= 5

    def window(arena, off, side, n, mul, as_mask):
        """the n x n window at (mul r, mul c) of the image of mul side a side at `off`, or None where it does not fit the arena"""
        p = mul * side
        if off < 0 or off % 4 or off + p * p > arena.numel():
            return None
        img = arena[off:off + p * p].cpu().numpy()
        img = (img != 0).astype(np.float32) if as_mask else f(img.view(np.uint16))
        return img.reshape(p, p)[mul * r:mul * r + n, mul * c:mul * c + n]

    sums = [(t, int(t.view(torch.int64).sum())) for t in (lr, qm)]
    for with_masks in (False, True):
        mk = lambda n: pool.keep(torch.full((n + SPARE,), 7.0, device="cuda"))
        n_lr, n_hr = B * min_L * S * S, B * 9 * S * S
        lrs, alphas, hrs, maps, lms = mk(n_lr), mk(B * min_L), mk(n_hr), mk(n_hr), mk(n_lr)
        if with_masks:
            rc = lib.hrn_collate_device_m(_p(lr), L, _p(hr), hr.numel(), _p(sm), sm.numel(), _p(qm), L, _p(plan), B, min_L, S, scale,
                                          _p(lrs), _p(alphas), _p(hrs), _p(maps), _p(lms), _p(cd), NULL)
        else:
            rc = lib.hrn_collate_device(_p(lr), L, _p(hr), hr.numel(), _p(sm), sm.numel(), _p(plan), B, min_L, S, _p(lrs), _p(alphas), _p(hrs),
                                        _p(maps), NULL)
        _ok(lib, rc)
        for t, n in ((lrs, n_lr), (alphas, B * min_L), (hrs, n_hr), (maps, n_hr), (lms, n_lr if with_masks else 0)):
            assert bool((t[n:] == 7.0).all()), "a write past an output"
        lrs_h, lms_h = lrs[:n_lr].view(B, min_L, S, S).cpu().numpy(), lms[:n_lr].view(B, min_L, S, S).cpu().numpy()
        hrs_h, maps_h = hrs[:n_hr].view(B, 3 * S, 3 * S).cpu().numpy(), maps[:n_hr].view(B, 3 * S, 3 * S).cpu().numpy()
        al = alphas[:B * min_L].view(B, min_L).cpu().numpy()
        told = 0
        for b, (side, offs, what) in enumerate(rows):
            code = int(codes[b]) if with_masks else 0
            turn = lambda w: np.ascontiguousarray(augment.apply(w, code))
            for v, off in enumerate(offs):
                tagv = f"collate S={S} masks={with_masks} row {b} slot {v} offset {off} code {code}"
                if off < 0:
                    assert not lrs_h[b, v].any() and al[b, v] == 0 and (not with_masks or not lms_h[b, v].any()), tagv
                    continue
                assert al[b, v] == 1
                want = window(lr, off, side, S, 1, False)
                if want is None:
                    assert what == "slot 0 NaN" and v == 0 and off + side * side == L + 1
                    assert np.isnan(lrs_h[b, v]).all() and (not with_masks or np.isnan(lms_h[b, v]).all()), tagv
                    continue
                assert _bits_equal(torch.from_numpy(lrs_h[b, v]), turn(want)), tagv
                if with_masks:
                    assert _bits_equal(torch.from_numpy(lms_h[b, v]), turn(window(qm, off, side, S, 1, True))), tagv
                if off >= 1 << 31:
                    wrong = turn(window(lr, off - (1 << 31), side, S, 1, False))
                    d = _differ(lrs_h[b, v], wrong)
                    print(f"{tagv} against the image at offset {off - (1 << 31)}: {d} of {S * S} pixels differ")
                    assert d > S * S // 2, "the comparison does not tell a wrapped offset"
                    told += 1
            if side == LC.COLLATE_SIDE:
                assert _bits_equal(torch.from_numpy(hrs_h[b]), turn(window(hr, plan_rows[b][0], side, 3 * S, 3, False))), (b, "hrs")
            else:
                assert not hrs_h[b].any()
            assert _bits_equal(torch.from_numpy(maps_h[b]), turn(window(sm, plan_rows[b][1], side, 3 * S, 3, True))), (b, "maps")
        assert told >= 3
    assert all(int(t.view(torch.int64).sum()) == s for t, s in sums), "a launch wrote an arena"


# ----------------------------------------------------------------------------------------------------------- B: hrn_tile_gather / _scatter
def _crossing_windows(plan, n_planes, hw, W, t, per_window):
    """the windows of `plan` worth checking as (window, plane) pairs: the first and the last of plane 0 and of the last plane, the windows
    whose rows straddle each crossing of the scene tensor (n_planes planes of hw elements, rows of W), and the windows at each crossing of
    the window-major tensor (per_window elements per (window, plane))"""
    from kernel_bounds import crossings
    n = len(plan.windows)
    out = {(0, 0), (n - 1, 0), (0, n_planes - 1), (n - 1, n_planes - 1)}
    for e in crossings(n_planes * hw, 4):
        p, y = e // hw, (e % hw) // W
        hit = [i for i, w in enumerate(plan.windows) if w.y0 <= y < w.y0 + t]
        out |= {(hit[0], p), (hit[len(hit) // 2], p), (hit[-1], p)}
    for e in crossings(n * n_planes * per_window, 4):
        i, p = divmod(e // per_window, n_planes)
        out |= {(i, p), (i - 1 if p == 0 else i, (p - 1) % n_planes)}
    return sorted(out)


def test_tile_gather_big_frame(pool):
    """hrn_tile_gather, regime B: one scene of (1, 9) planes of 16002 x 16001 (past 2^31 elements), t = 128 with hrn_hrnet_halo's R, every
    window of the plan in one launch (the kMaxRows guard asks for no split: 30.6 M rows): the output passes 2^31 elements too.  Bit for bit
    against tiling.gather for the first window, the last window and the windows whose rows straddle each crossing.  Control: at the
    checked windows whose source lies past byte 2^32, the rows a 32-bit byte offset would address are told from the output"""
    from hrnet_hip import tiling
    case = LC.gather_case()
    B, V, H, W, t, R = (case[k] for k in ("B", "V", "H", "W", "t", "R"))
    _need(LC.gib(case["tensors"]))
    lib = _lib()
    assert lib.hrn_hrnet_halo(LC.TILE_LAYERS, V) == R
    plan = tiling.plan(H, W, t, R)
    n = len(plan.windows)
    assert n == case["windows"] == lib.hrn_tile_count(H, W, t, R) and case["rows"] < LC.TILE_MAX_ROWS
    lrs = _fill(pool, V * H * W, _gen(361), "normal")
    out = _nan_out(pool, n * V * t * t)
    c0 = _sum64(lrs)
    _ok(lib, lib.hrn_tile_gather(_p(lrs), B, V, H, W, t, R, 0, n, _p(out), NULL))
    assert _sum64(lrs) == c0 and _spare_ok(out, n * V * t * t), "the launch wrote its input or past its output"
    checked = _crossing_windows(plan, V, H * W, W, t, t * t)
    _says(f"tile_gather {H}x{W} V={V} t={t} R={R} windows {n}", "2^31el", case["tensors"], checked)
    scene = lrs[:V * H * W].view(B, V, H, W)
    got_all = out[:n * V * t * t].view(n, B, V, t, t)
    told = 0
    for i, p in checked:
        w = plan.windows[i]
        want = tiling.gather(scene, [w], t)[0, 0, p]
        got = got_all[i, 0, p]
        assert _differ(got, want.contiguous()) == 0, f"tile_gather: window {i} plane {p}"
        e0 = p * H * W + w.y0 * W + w.x0
        if e0 >= 1 << 30:
            e1 = e0 - (1 << 30)
            wrong = torch.stack([lrs[e1 + r * W:e1 + r * W + t] for r in range(t)])
            d = _differ(got, wrong)
            print(f"tile_gather window {i} plane {p} (source element {e0}) against element {e1}: {d} of {t * t} pixels differ")
            assert d > t * t // 2, "the comparison does not tell a wrapped source offset"
            told += 1
    assert told >= 2


def test_tile_scatter_big_frame(pool):
    """hrn_tile_scatter, regime B: x3 into one plane of 36000 x 36003 - 5.2e9 bytes, 1.296e9 pixels, under the INT32_MAX pixel guard - from
    the 15129 windows' forwards (8.9e9 bytes, past 2^31 elements), in two launches around one row of windows that is left out.  The output
    is prefilled with NaN: the cores of the left-out windows must still hold it, pixel for pixel, and the spare words too.  Bit for bit
    against tiling.scatter (into a second plane) for the first window, the last window and the windows at each crossing of either
    tensor"""
    from hrnet_hip import tiling
    case = LC.scatter_case()
    B, H, W, t, R, S = (case[k] for k in ("B", "H", "W", "t", "R", "S"))
    _need(LC.gib(case["tensors"]))
    lib = _lib()
    plan = tiling.plan(H, W, t, R)
    n = len(plan.windows)
    a, b = case["skip"]
    assert n == case["windows"] == lib.hrn_tile_count(H, W, t, R) and 0 < a < b < n and S * H * S * W <= 2 ** 31 - 1 and S * H * S * W * 4 > 1 << 32
    St, SH, SW = S * t, S * H, S * W
    srs = _fill(pool, n * St * St, _gen(371), "normal")
    out, ref = _nan_out(pool, SH * SW), _nan_out(pool, SH * SW)
    c0 = _sum64(srs)
    for w0, w1 in ((0, a), (b, n)):
        rows = (w1 - w0) * B * S * t
        assert rows < LC.TILE_MAX_ROWS
        _ok(lib, lib.hrn_tile_scatter(_p(srs[w0 * St * St:]), B, H, W, t, R, S, w0, w1, _p(out), NULL))
    assert _sum64(srs) == c0 and _spare_ok(out, SH * SW), "a launch wrote its input or past its output"
    left = sum((w.cy1 - w.cy0) * (w.cx1 - w.cx0) for w in plan.windows[a:b]) * S * S
    nans = sum(int(torch.count_nonzero(torch.isnan(out[lo:min(SH * SW, lo + Big.CHUNK)]))) for lo in range(0, SH * SW, Big.CHUNK))    # (a sum of bools would widen them)
    print(f"tile_scatter: {nans} pixels still NaN, the cores of the windows [{a}, {b}) left out are {left}")
    assert nans == left
    plane = out[:SH * SW].view(SH, SW)
    for w in plan.windows[a:b]:
        assert bool(torch.isnan(plane[S * w.cy0:S * w.cy1, S * w.cx0:S * w.cx1]).all())
    checked = [(i, p) for i, p in _crossing_windows(plan, 1, SH * SW, SW * S, t, St * St)]
    # (a row of the x3 plane is SW elements, S of them per LR row: W' = S SW above turns a plane offset into an LR row)
    checked = sorted({i for i, _ in checked if not a <= i < b})
    _says(f"tile_scatter {H}x{W} x{S} t={t} R={R} windows {n}", "2^31el", {k: v for k, v in case["tensors"].items() if k != "ref"}, checked)
    sel = [plan.windows[i] for i in checked]
    src = torch.stack([srs[i * St * St:(i + 1) * St * St].view(1, 1, St, St) for i in checked])
    tiling.scatter(ref[:SH * SW].view(1, 1, SH, SW), src, sel, t, S)
    rplane = ref[:SH * SW].view(SH, SW)
    for i, w in zip(checked, sel):
        core = (slice(S * w.cy0, S * w.cy1), slice(S * w.cx0, S * w.cx1))
        assert _differ(plane[core].contiguous(), rplane[core].contiguous()) == 0, f"tile_scatter: the core of window {i}"


def test_tile_scatter_refuses_its_smallest_refused_plane(pool):
    """the x2 plane of 23171 x 23171 has 2 147 580 964 pixels, the first square beyond 32-bit in-plane offsets: -2, the message, nothing
    written (23170 x 23170 passes this guard: tests/test_large_offsets_host.py)"""
    lib = _lib()
    H, W, S = (LC.SCATTER_REFUSED[k] for k in ("H", "W", "S"))
    src, out = torch.zeros(4096, device="cuda"), torch.full((4096,), float("nan"), device="cuda")
    rc = lib.hrn_tile_scatter(_p(src), 1, H, W, 128, 15, S, 0, 1, _p(out), NULL)
    msg = lib.hrn_last_error()
    torch.cuda.synchronize()
    assert rc == -2 and f"the x{S} plane of H={H} x W={W} is beyond 32-bit in-plane offsets".encode() in msg, (rc, msg)
    assert bool(torch.isnan(out).all()) and not bool(src.any())


def test_shift_cssim_refuses_its_smallest_refused_frame(pool):
    """46341 x 46341 = 2 147 488 281 pixels, the first square beyond the int in-plane indices of cssim.hip: -2, the message, nothing
    written"""
    lib = _lib()
    H, W = LC.CSSIM_REFUSED["H"], LC.CSSIM_REFUSED["W"]
    nbytes = lib.hrn_shift_cssim_workspace_bytes(1, H, W, 1, 1)
    _need(nbytes / GIB + 1)
    ws = pool.keep(torch.zeros(max(nbytes, 4096), dtype=torch.uint8, device="cuda"))
    src = torch.zeros(4096, device="cuda")
    out = torch.full((64,), float("nan"), device="cuda")
    stats, scores = torch.full((64,), float("nan"), dtype=torch.float64, device="cuda"), torch.full((64,), float("nan"), dtype=torch.float64, device="cuda")
    rc = lib.hrn_shift_cssim(_p(src), _p(src), _p(src), 1, H, W, 1, 1, 0, 1, ctypes.c_float(1.0), _p(out), _p(stats), _p(scores), _p(ws), ws.numel(), NULL)
    msg = lib.hrn_last_error()
    torch.cuda.synchronize()
    assert rc == -2 and f"cssim: a frame of {H} x {W} exceeds 2^31 pixels".encode() in msg, (rc, msg)
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(stats).all()) and bool(torch.isnan(scores).all()) and not bool(ws.any()) and not bool(src.any())


# ----------------------------------------------------------------------------------------------------------- hrn_cl1_loss_*, hrn_shift_cssim, hrn_cssim_loss_backward
SEARCHED_IDS = [f"{a}-{b}-border{c}-{'eps' if a == 'cl1' else 'window'}{d:g}{'-clip' if e else ''}{'-bwd' if f else ''}-{g}" for a, b, c, d, e, f, g in LC.SEARCHED_A]
WINDOWS = {0: "gaussian", 1: "uniform"}


def _planted(pool, n, W, border, clip, gen):
    """srs uniform (beyond [0, 1] when clip), hrs = srs moved so that the HR window at offset LC.PLANT is the SR centre crop, plus
    N(0, 0.05^2); maps 0 at a tenth of the pixels.  A flat move by e elements: inside a plane it is the shift, at a plane's edges the
    values come from the neighbouring rows or plane, which are as random"""
    lo, hi = (-0.2, 1.2) if clip else (0.0, 1.0)
    srs = _fill(pool, n, gen, "uniform", lo, hi)
    hrs = _fill(pool, n, gen, "normal")
    e = (border - LC.PLANT[0]) * W + (border - LC.PLANT[1])
    assert e > 0
    for a in range(0, n, Big.CHUNK):
        b = min(n, a + Big.CHUNK)
        c = hrs[a:b].mul_(0.05)
        k = min(b, n - e) - a
        if k > 0:
            c[:k].add_(srs[a + e:a + e + k].clamp(0.0, 1.0))
        if k < b - a:
            c[max(k, 0):].add_(0.5)
    return srs, hrs, _fill(pool, n, gen, "mask", 0.1)


def _searched(lib, kind, x, B, H, W, border, option, clip, d_out, d_srs):
    """forward (and, with d_srs, backward with the forward's stats) -> (out (B + SPARE) f32, stats f64, scores f64 or None), the
    forward's workspace freed"""
    ns = 5 if kind == "cl1" else 4
    out = torch.full((B + SPARE,), float("nan"), device="cuda")
    stats = torch.full((B * ns + SPARE,), float("nan"), dtype=torch.float64, device="cuda")
    scores = None
    if kind == "cl1":
        nbytes = lib.hrn_cl1_loss_workspace_bytes(B, H, W, border)
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        _ok(lib, lib.hrn_cl1_loss_train(*map(_p, x), B, H, W, border, int(clip), option, _p(out), _p(stats), _p(ws), nbytes, NULL))
    else:
        nk = (2 * border + 1) ** 2
        scores = torch.full((B * nk + SPARE,), float("nan"), dtype=torch.float64, device="cuda")
        nbytes = lib.hrn_shift_cssim_workspace_bytes(B, H, W, border, option)
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        _ok(lib, lib.hrn_shift_cssim(*map(_p, x), B, H, W, border, option, int(clip), 1, 1.0, _p(out), _p(stats), _p(scores), _p(ws), nbytes, NULL))
        assert _spare_ok(scores, B * nk)
    assert nbytes > 0 and _spare_ok(out, B) and _spare_ok(stats, ns * B)
    del ws
    if d_srs is not None and kind == "cl1":
        _ok(lib, lib.hrn_cl1_loss_backward(*map(_p, x), _p(stats), _p(d_out), B, H, W, border, int(clip), option, _p(d_srs), NULL))
    elif d_srs is not None:
        nbytes = lib.hrn_cssim_loss_backward_workspace_bytes(B, H, W, border, option)
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        _ok(lib, lib.hrn_cssim_loss_backward(*map(_p, x), _p(stats), _p(d_out), B, H, W, border, option, int(clip), 1, 1.0, _p(d_srs), _p(ws), nbytes, NULL))
    return out, stats, scores


def _cl1_against_fp64(tag, x, border, eps, clip, d, out, stats, grad):
    """one sample (1, H, W) against tests/cl1_ref.py under test_gpu_cl1_loss.py's tolerances"""
    import cl1_cases as CC
    import cl1_ref as R
    import util
    s = x[0].double().requires_grad_(True)
    want, k, cl, wstats = R.cl1_loss(s, x[1], x[2], border, clip, eps)
    (want * d).sum().backward()
    assert float(R.top_two_gap(cl).min()) > 1e-6 and (eps > 0 or R.min_abs_e(x[0], x[1], x[2], k, border, clip) > 1e-12)
    e_out = util.rel_err(out.numpy(), want.detach().numpy())
    e_stats = max(util.rel_err(stats[j:j + 1].numpy(), wstats[:, j].numpy()) for j in (0, 1, 2, 4))
    assert int(stats[3]) == int(k[0]) and e_out <= CC.TOL and e_stats <= CC.TOL, (tag, e_out, e_stats)
    e_grad = 0.0
    if grad is not None:
        e_grad = float((grad.double() - s.grad).abs().amax()) / float(s.grad.abs().amax())
        assert e_grad <= CC.GRAD_TOL, (tag, e_grad)
    return f"out {e_out:.2e}, stats {e_stats:.2e}, d_srs err / max-norm {e_grad:.2e}"


def _cssim_against_fp64(tag, x, border, window, clip, d, out, stats, scores, grad):
    """one sample against tests/cssim_ref.py / cssim_grad_ref.py under cssim_cases.TOL and cssim_loss_bounds.CSSIM_GRAD_TOL, as
    cssim_cases.compare and tests/test_gpu_cssim_loss.py hold them"""
    import cssim_cases as CC
    import cssim_grad_ref as G
    import cssim_ref as R
    from cssim_loss_bounds import CSSIM_GRAD_TOL
    s, h, m = (t[0].numpy() for t in x)
    want, k, bias, n = R.shift_cssim(s, h, m, border, WINDOWS[window], clip, True, 1.0)
    got = scores.numpy()
    assert np.isfinite(want).all() and np.isfinite(got).all() and k >= 0 and R.gap(want) >= 1e-3, tag
    err = float(np.abs(got - want).max())
    assert err <= CC.TOL, (tag, err)
    st = stats.numpy()
    assert st[3] == k and st[0] == n[k] and abs(st[1] - bias[k]) <= 1e-12 + 1e-12 * abs(bias[k]) and abs(st[2] - want[k]) <= CC.TOL
    assert float(out[0]) == float(np.float32(st[2]))
    e_grad = 0.0
    if grad is not None:
        e_grad = G.rel_err(grad.numpy(), d * G.grad(s, h, m, k, border, WINDOWS[window], clip, True, 1.0))
        assert e_grad <= CSSIM_GRAD_TOL, (tag, e_grad)
    return f"scores {err:.2e}, d_srs err / max |gradient| {e_grad:.2e}"


@pytest.mark.parametrize("kind,shape,border,option,clip,backward,cross", LC.SEARCHED_A, ids=SEARCHED_IDS)
def test_searched_loss_deep_batch(pool, kind, shape, border, option, clip, backward, cross):
    """hrn_cl1_loss_train / _backward (eps 0 and 1e-3) and hrn_shift_cssim / hrn_cssim_loss_backward (both windows), regime A, shaped as
    test_shift_loss_deep_batch: 192 x 192 past 2^31 elements runs the forward alone (three inputs of 8 GiB and the workspace; a fourth
    tensor does not fit the cap), 181 x 203 at border 3 with clip and the backward past 2^32 bytes.  out, stats, every offset's score
    (cssim) and d_srs of the checked samples bit for bit against the sample alone; the sample alone against its fp64 restatement under the
    tolerances of the loss's own small-shape test"""
    case = LC.searched_case(kind, shape, border, option, clip, backward, cross)
    B, H, W = case["B"], case["H"], case["W"]
    hw = H * W
    lib = _lib()
    if kind == "cl1":
        ws_bytes = lib.hrn_cl1_loss_workspace_bytes(B, H, W, border)
    else:
        ws_bytes = max(lib.hrn_shift_cssim_workspace_bytes(B, H, W, border, option), lib.hrn_cssim_loss_backward_workspace_bytes(B, H, W, border, option))
    _need(LC.gib(case["tensors"], ws_bytes))
    x = _planted(pool, B * hw, W, border, clip, _gen(381))
    d_out = torch.tensor(D_OUT, device="cuda")[torch.arange(B, device="cuda") % 3].contiguous()
    d_srs = _nan_out(pool, B * hw) if backward else None
    sums = [(t, _sum64(t)) for t in x]
    out, stats, scores = _searched(lib, kind, x, B, H, W, border, option, clip, d_out, d_srs)
    for t in (out, stats, scores):
        if t is not None:
            pool.keep(t)
    assert all(_sum64(t) == c for t, c in sums), "a launch wrote one of its inputs"
    assert d_srs is None or _spare_ok(d_srs, B * hw), "a write past d_srs"
    bs = _planes((B, hw))
    tag = f"{kind} {shape} border {border} option {option:g} B={B} workspace {ws_bytes / GIB:.2f} GiB"
    _says(tag, cross, case["tensors"], bs)
    ns, nk = (5 if kind == "cl1" else 4), (2 * border + 1) ** 2
    same = lambda a, b: torch.equal(a.view(torch.int64), b.view(torch.int64))
    for b in bs:
        one = tuple(t[b * hw:(b + 1) * hw].clone() for t in x)
        d1 = torch.full((hw + SPARE,), float("nan"), device="cuda") if backward else None
        out1, stats1, scores1 = _searched(lib, kind, one, 1, H, W, border, option, clip, d_out[b:b + 1].clone(), d1)
        assert _differ(out[b:b + 1], out1[:1]) == 0 and same(stats[ns * b:ns * b + ns], stats1[:ns]), f"{tag}: sample {b} differs from its launch alone"
        assert scores is None or same(scores[nk * b:nk * b + nk], scores1[:nk]), f"{tag}: the scores of sample {b} differ from its launch alone"
        if backward:
            assert _spare_ok(d1, hw) and _differ(d_srs[b * hw:(b + 1) * hw], d1[:hw]) == 0, f"{tag}: d_srs of sample {b} differs from its launch alone"
            frame = torch.ones((H, W), dtype=torch.bool)
            frame[border:-border, border:-border] = False
            assert bool((d1[:hw].view(H, W).cpu()[frame] == 0).all())
        host = tuple(t.view(1, H, W).cpu() for t in one)
        grad = d1[:hw].view(1, H, W).cpu() if backward else None
        if kind == "cl1":
            said = _cl1_against_fp64(f"{tag} sample {b}", host, border, float(np.float32(option)), clip, D_OUT[b % 3], out1[:1].cpu(), stats1[:ns].cpu(), grad)
        else:
            said = _cssim_against_fp64(f"{tag} sample {b}", host, border, option, clip, D_OUT[b % 3], out1[:1].cpu(), stats1[:ns].cpu(), scores1[:nk].cpu(),
                                       grad[0] if backward else None)
        print(f"{tag} sample {b}: bit-identical to the sample alone; alone against fp64: {said}")


# ----------------------------------------------------------------------------------------------------------- hrn_lanczos_shift (+ backward)
LANCZOS_IDS = [f"{a}-{b}-{c}" for a, b, c in LC.LANCZOS_A]


def _lanczos_bwd(lib, img, shift, d_out, c, H, W, d_img, d_shift):
    nbytes = lib.hrn_lanczos_shift_backward_workspace_bytes(1, c, H, W)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    _ok(lib, lib.hrn_lanczos_shift_backward(_p(img), _p(shift), _p(d_out), 1, c, H, W, _p(d_img), _p(d_shift), _p(ws), nbytes, NULL))


@pytest.mark.parametrize("which,shape,cross", LC.LANCZOS_A, ids=LANCZOS_IDS)
def test_lanczos_shift_deep_batch(pool, which, shape, cross):
    """hrn_lanczos_shift and hrn_lanczos_shift_backward (lanczos.hip, lanczos_bwd.hip), regime A: b = 1 and c = the planes, capped at 65535,
    so 192 x 192 and 181 x 203; the channels' shifts cycle through kernel_refs.TAIL_SHIFTS (an integer shift on either axis, one beyond
    the support).  The forward's two tensors pass 2^31 elements; the backward has three and a workspace as large as one of them, and stops
    past 2^32 bytes.  Bit for bit against the plane alone (d_shift += into the same start values); the plane alone against
    kernel_refs' restatement under C_TAIL"""
    import kernel_refs as K
    from kernel_bounds import C_TAIL
    case = LC.lanczos_case(which, shape, cross)
    c, H, W = case["c"], case["H"], case["W"]
    hw = H * W
    lib = _lib()
    ws_bytes = lib.hrn_lanczos_shift_backward_workspace_bytes(1, c, H, W) if which == "bwd" else 0
    _need(LC.gib(case["tensors"], ws_bytes))
    g = _gen(391)
    img = _fill(pool, c * hw, g, "uniform", 0.25, 0.75)
    shift = K.TAIL_SHIFTS[torch.arange(c) % 3].contiguous()
    sd = shift.cuda()
    ps = _planes((c, hw))
    tag = f"lanczos {which} {shape} c={c} workspace {ws_bytes / GIB:.2f} GiB"
    if which == "fwd":
        out = _nan_out(pool, c * hw)
        c0 = _sum64(img)
        _ok(lib, lib.hrn_lanczos_shift(_p(img), _p(sd), 1, c, H, W, _p(out), NULL))
        assert _sum64(img) == c0 and _spare_ok(out, c * hw), "the launch wrote its input or past its output"
    else:
        d_out = _fill(pool, c * hw, g, "normal")
        d_img = _nan_out(pool, c * hw)
        start = torch.randn((c, 2), generator=torch.Generator().manual_seed(392))
        d_shift = torch.full((2 * c + SPARE,), float("nan"), device="cuda")
        d_shift[:2 * c] = start.reshape(-1).cuda()
        sums = [(t, _sum64(t)) for t in (img, d_out)]
        _lanczos_bwd(lib, img, sd, d_out, c, H, W, d_img, d_shift)
        assert all(_sum64(t) == s for t, s in sums) and _spare_ok(d_img, c * hw) and _spare_ok(d_shift, 2 * c), "the launch wrote an input or past an output"
    _says(tag, cross, case["tensors"], ps)
    for p in ps:
        sl = slice(p * hw, (p + 1) * hw)
        i1, s1 = img[sl].clone(), sd[p:p + 1].clone()
        i64, s64 = i1.view(1, 1, H, W).cpu().double(), shift[p:p + 1].double()
        if which == "fwd":
            o1 = torch.full((hw + SPARE,), float("nan"), device="cuda")
            _ok(lib, lib.hrn_lanczos_shift(_p(i1), _p(s1), 1, 1, H, W, _p(o1), NULL))
            assert _spare_ok(o1, hw) and _differ(out[sl], o1[:hw]) == 0, f"{tag}: plane {p} differs from its launch alone"
            r = _assert_close(f"{tag} plane {p}", "f32", o1[:hw].view(1, 1, H, W).cpu(), K.ref_lanczos_shift(i64, s64), K.lanczos_shift_T(i64, s64),
                              layout="b c y x", c=C_TAIL)
        else:
            g1 = d_out[sl].clone()
            di1, ds1 = torch.full((hw + SPARE,), float("nan"), device="cuda"), torch.full((2 + SPARE,), float("nan"), device="cuda")
            ds1[:2] = start[p].cuda()
            _lanczos_bwd(lib, i1, s1, g1, 1, H, W, di1, ds1)
            assert _spare_ok(di1, hw) and _spare_ok(ds1, 2)
            assert _differ(d_img[sl], di1[:hw]) == 0 and _differ(d_shift[2 * p:2 * p + 2], ds1[:2]) == 0, f"{tag}: plane {p} differs from its launch alone"
            o64 = g1.view(1, 1, H, W).cpu().double()
            wi, ws = K.ref_lanczos_grads(i64, s64, o64)
            r = _assert_close(f"{tag} d_img plane {p}", "f32", di1[:hw].view(1, 1, H, W).cpu(), wi, K.lanczos_dimg_T(o64, s64), layout="b c y x", c=C_TAIL)
            st = start[p:p + 1].double()
            r = max(r, _assert_close(f"{tag} d_shift plane {p}", "f32", ds1[:2].view(1, 2).cpu(), st + ws, st.abs() + K.lanczos_dshift_T(i64, s64, o64),
                                     layout="c axis", c=C_TAIL))
        print(f"{tag} plane {p}: bit-identical to the plane alone; alone against fp64: error / bound {r:.3e}")


# ----------------------------------------------------------------------------------------------------------- hrn_mncc_grid_scene / _search_scene
SEARCH_IDS = [f"{a}-{b}-{c}" for a, b, c in LC.SEARCH_A]
GRID_CENTRES = [(0.0, 0.0), (-1.3, 0.7), (1.75, -0.5), (-37.25, 41.5)]     # tests/test_gpu_registration_scene.py's: the last leaves nothing
GRID_WIDTH, SEARCH_RADIUS = 2.0, 1.0


def _scene_inputs(pool, B, V, H, W, masks, gen):
    """views uniform; ref[b] = views[b, 0] + N(0, 0.1^2): view 0 of every sample matches its reference at shift 0, view 1 does not match
    anything; masks 0 at 15 % of the pixels"""
    hw = H * W
    views = _fill(pool, B * V * hw, gen, "uniform")
    ref = _fill(pool, B * hw, gen, "normal")
    step = max(1, Big.CHUNK // hw)
    for b0 in range(0, B, step):
        b1 = min(B, b0 + step)
        ref[b0 * hw:b1 * hw].view(b1 - b0, hw).mul_(0.1).add_(views[b0 * V * hw:b1 * V * hw].view(b1 - b0, V * hw)[:, :hw])
    vm = _fill(pool, B * V * hw, gen, "mask", 0.15) if masks else None
    rm = _fill(pool, B * hw, gen, "mask", 0.15) if masks else None
    return ref, rm, views, vm


def _opt(t):
    return _p(t) if t is not None else NULL


def _search_scene(lib, ref, rm, views, vm, centres, B, V, H, W):
    """one grid level at `centres` and the whole search -> scores (B V P P), shifts (B V 2), trace (B V levels 3), each + SPARE NaN"""
    P, levels = LC.MNCC_P, LC.MNCC_LEVELS
    nbytes = lib.hrn_mncc_scene_workspace_bytes(B, V, H, W, P)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    mk = lambda n: torch.full((n + SPARE,), float("nan"), device="cuda")
    scores, shifts, trace = mk(B * V * P * P), mk(B * V * 2), mk(B * V * levels * 3)
    _ok(lib, lib.hrn_mncc_grid_scene(_p(ref), _opt(rm), _p(views), _opt(vm), _p(centres), B, V, H, W, P, GRID_WIDTH, _p(scores), _p(ws), nbytes, NULL))
    _ok(lib, lib.hrn_mncc_search_scene(_p(ref), _opt(rm), _p(views), _opt(vm), B, V, H, W, P, levels, SEARCH_RADIUS, _p(shifts), _p(trace), _p(ws), nbytes, NULL))
    assert _spare_ok(scores, B * V * P * P) and _spare_ok(shifts, B * V * 2) and _spare_ok(trace, B * V * levels * 3)
    return scores, shifts, trace


@pytest.mark.parametrize("masks,shape,cross", LC.SEARCH_A, ids=SEARCH_IDS)
def test_search_scene_deep_batch(pool, masks, shape, cross):
    """hrn_mncc_grid_scene and hrn_mncc_search_scene, regime A: V = 2, P = 3 (the smallest), two levels.  scores, shifts and trace of the
    checked samples - the union of the views' and the reference's boundary samples - bit for bit against the sample alone; the sample
    alone against tests/registration_ref.py under test_gpu_registration_scene.py's GRID_BOUND, level by level along the device's path"""
    import registration_ref as R
    from registration_cases import GRID_BOUND
    case = LC.search_case(masks, shape, cross)
    B, V, H, W, per = (case[k] for k in ("B", "V", "H", "W", "per"))
    hw, P, levels = H * W, LC.MNCC_P, LC.MNCC_LEVELS
    lib = _lib()
    ws_bytes = lib.hrn_mncc_scene_workspace_bytes(B, V, H, W, P)
    _need(LC.gib(case["tensors"], ws_bytes))
    ref, rm, views, vm = _scene_inputs(pool, B, V, H, W, masks == "masks", _gen(401))
    centres = torch.tensor(GRID_CENTRES, dtype=torch.float32)[torch.arange(B * V) % 4].reshape(B, V, 2).contiguous()
    cd = centres.cuda()
    sums = [(t, _sum64(t)) for t in (ref, rm, views, vm) if t is not None]
    scores, shifts, trace = (pool.keep(t) for t in _search_scene(lib, ref, rm, views, vm, cd, B, V, H, W))
    assert all(_sum64(t) == c for t, c in sums) and torch.equal(cd.cpu(), centres), "a launch wrote one of its inputs"
    bs = _planes((B, per), (B, hw))
    tag = f"search_scene {masks} {shape} B={B} workspace {ws_bytes / GIB:.2f} GiB"
    _says(tag, cross, case["tensors"], bs)
    widths = R.level_widths(P, levels, SEARCH_RADIUS)
    for b in bs:
        one = [t[b * n:(b + 1) * n].clone() if t is not None else None for t, n in ((ref, hw), (rm, hw), (views, per), (vm, per))]
        s1, h1, t1 = _search_scene(lib, *one, cd[b:b + 1].clone(), 1, V, H, W)
        for name, big, alone, n in (("scores", scores, s1, V * P * P), ("shifts", shifts, h1, V * 2), ("trace", trace, t1, V * levels * 3)):
            assert _differ(big[b * n:(b + 1) * n], alone[:n]) == 0, f"{tag}: {name} of sample {b} differ from its launch alone"
        r_, rm_, v_, vm_ = (t.cpu().numpy().reshape((-1, H, W)) if t is not None else None for t in one)
        got_scores, got_trace = s1[:V * P * P].view(V, P, P).cpu().numpy().astype(np.float64), t1[:V * levels * 3].view(V, levels, 3).cpu().numpy()
        assert np.array_equal(h1[:V * 2].view(V, 2).cpu().numpy(), got_trace[:, -1, :2])
        worst = 0.0
        for v in range(V):
            mv = vm_[v] if vm_ is not None else None
            mr = rm_[0] if rm_ is not None else None
            want = R.grid(r_[0], mr, v_[v], mv, centres[b, v].numpy(), np.float32(GRID_WIDTH), P)[0]
            assert np.array_equal(np.isneginf(got_scores[v]), np.isneginf(want))
            fin = np.isfinite(want)
            worst = max(worst, float(np.abs(got_scores[v][fin] - want[fin]).max()) if fin.any() else 0.0)
            centre = (np.float32(0.0), np.float32(0.0))
            for k in range(levels):
                want, dys, dxs = R.grid(r_[0], mr, v_[v], mv, centre, widths[k], P)
                dy, dx, got = got_trace[v, k]
                assert np.isfinite(want).any()
                i, j = np.flatnonzero(dys == dy), np.flatnonzero(dxs == dx)
                assert len(i) and len(j), f"{tag} sample {b} view {v} level {k}: ({dy}, {dx}) is no point of the grid"
                worst = max(worst, abs(got - want[i[0], j[0]]))
                assert want.max() - want[i[0], j[0]] <= 2 * GRID_BOUND
                centre = (dy, dx)
        print(f"{tag} sample {b}: bit-identical to the sample alone; alone against fp64: {worst:.3e}")
        assert worst <= GRID_BOUND


# ----------------------------------------------------------------------------------------------------------- hrn_mncc_search_local / _apply_field
LOCAL_IDS = [f"{a}-{b}-{c}" for a, b, c in LC.LOCAL_A]
LOCAL_INITS = [(0.13, -0.21), (-0.31, 0.17), (0.07, 0.29)]      # never a whole pixel away from a grid point: no coordinate is a whole number
LOCAL_RADIUS, LOCAL_MIN_VALID = 0.5, 0.25


def _search_local(lib, ref, rm, views, vm, init, B, V, H, W, by, bx):
    P, levels, block = LC.MNCC_P, LC.MNCC_LEVELS, LC.LOCAL_BLOCK
    nbytes = lib.hrn_mncc_local_workspace_bytes(B, V, H, W, P, block)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    mk = lambda n: torch.full((n + SPARE,), float("nan"), device="cuda")
    nb = B * V * by * bx
    field, trace, ok = mk(nb * 2), mk(nb * levels * 3), mk(nb)
    _ok(lib, lib.hrn_mncc_search_local(_p(ref), _opt(rm), _p(views), _opt(vm), _p(init), B, V, H, W, P, levels, LOCAL_RADIUS, block, LOCAL_MIN_VALID,
                                       _p(field), _p(trace), _p(ok), _p(ws), nbytes, NULL))
    assert _spare_ok(field, nb * 2) and _spare_ok(trace, nb * levels * 3) and _spare_ok(ok, nb)
    return field, trace, ok


def _apply_field(lib, views, vm, field, B, V, H, W, out, valid):
    _ok(lib, lib.hrn_mncc_apply_field(_p(views), _opt(vm), _p(field), B, V, H, W, LC.LOCAL_BLOCK, _p(out), _p(valid), NULL))


@pytest.mark.parametrize("masks,shape,cross", LC.LOCAL_A, ids=LOCAL_IDS)
def test_search_local_and_apply_field_deep_batch(pool, masks, shape, cross):
    """hrn_mncc_search_local and hrn_mncc_apply_field, regime A, block 64 (the smallest): one block on 64 x 64, two per axis on the ragged
    100 x 130.  field, trace, ok, and out, out_valid under the field of the same launch, bit for bit against the sample alone; the sample
    alone against tests/registration_local_ref.py under the bounds of test_gpu_registration_local.py.  With masks the resampling has four
    tensors of one size and stops past 2^32 bytes; without, the reference is freed before the resampling and the views pass 2^31
    elements"""
    import registration_local_ref as L
    from registration_cases import APPLY_BOUND, SCORE_BOUND
    case = LC.local_case(masks, shape, cross)
    B, V, H, W, per, by, bx = (case[k] for k in ("B", "V", "H", "W", "per", "by", "bx"))
    hw, P, levels, block = H * W, LC.MNCC_P, LC.MNCC_LEVELS, LC.LOCAL_BLOCK
    lib = _lib()
    assert (by, bx) == (lib.hrn_mncc_local_blocks(H, block), lib.hrn_mncc_local_blocks(W, block))
    ws_bytes = lib.hrn_mncc_local_workspace_bytes(B, V, H, W, P, block)
    _need(LC.gib(case["tensors"], ws_bytes))
    ref, rm, views, vm = _scene_inputs(pool, B, V, H, W, masks == "masks", _gen(411))
    init = torch.tensor(LOCAL_INITS, dtype=torch.float32)[torch.arange(B * V) % 3].reshape(B, V, 2).contiguous()
    idev = init.cuda()
    sums = [(t, _sum64(t)) for t in (ref, rm, views, vm) if t is not None]
    field, trace, ok = (pool.keep(t) for t in _search_local(lib, ref, rm, views, vm, idev, B, V, H, W, by, bx))
    assert all(_sum64(t) == c for t, c in sums) and torch.equal(idev.cpu(), init), "the search wrote one of its inputs"
    bs = _planes((B, per), (B, hw))
    kept = {b: [t[b * hw:(b + 1) * hw].clone() if t is not None else None for t in (ref, rm)] for b in bs}
    if masks != "masks":                                     # make room for out and out_valid
        ref.untyped_storage().resize_(0)
    out, valid = _nan_out(pool, B * per), _nan_out(pool, B * per)
    sums = [(t, _sum64(t)) for t in (views, vm) if t is not None]
    f0 = field.clone()
    _apply_field(lib, views, vm, field, B, V, H, W, out, valid)
    assert all(_sum64(t) == c for t, c in sums) and torch.equal(f0.view(torch.int32), field.view(torch.int32)), "the resampling wrote one of its inputs"
    assert _spare_ok(out, B * per) and _spare_ok(valid, B * per), "a write past an output"
    tag = f"local {masks} {shape} B={B} blocks {by}x{bx} workspace {ws_bytes / GIB:.2f} GiB"
    _says(tag, cross, {**case["tensors"], **case["search"]}, bs)
    nb = V * by * bx
    rows, cols = L.bounds(H, block), L.bounds(W, block)
    for b in bs:
        r1, m1 = kept[b]
        v1 = views[b * per:(b + 1) * per].clone()
        k1 = vm[b * per:(b + 1) * per].clone() if vm is not None else None
        f1, t1, o1 = _search_local(lib, r1, m1, v1, k1, idev[b:b + 1].clone(), 1, V, H, W, by, bx)
        for name, big, alone, n in (("field", field, f1, nb * 2), ("trace", trace, t1, nb * levels * 3), ("ok", ok, o1, nb)):
            assert _differ(big[b * n:(b + 1) * n], alone[:n]) == 0, f"{tag}: {name} of sample {b} differs from its launch alone"
        a1, av1 = torch.full((per + SPARE,), float("nan"), device="cuda"), torch.full((per + SPARE,), float("nan"), device="cuda")
        _apply_field(lib, v1, k1, f1, 1, V, H, W, a1, av1)
        assert _spare_ok(a1, per) and _spare_ok(av1, per)
        assert _differ(out[b * per:(b + 1) * per], a1[:per]) == 0 and _differ(valid[b * per:(b + 1) * per], av1[:per]) == 0, \
            f"{tag}: the resampled sample {b} differs from its launch alone"
        r_, v_ = r1.view(H, W).cpu().numpy(), v1.view(V, H, W).cpu().numpy()
        m_ = m1.view(H, W).cpu().numpy() if m1 is not None else None
        k_ = k1.view(V, H, W).cpu().numpy() if k1 is not None else None
        tr = t1[:nb * levels * 3].view(V, by, bx, levels, 3).cpu().numpy()
        fl, okn = f1[:nb * 2].view(V, by, bx, 2).cpu().numpy(), o1[:nb].view(V, by, bx).cpu().numpy()
        got_out, got_valid = a1[:per].view(V, H, W).cpu().numpy(), av1[:per].view(V, H, W).cpu().numpy()
        worst_score = worst_px = 0.0
        for v in range(V):
            kv = k_[v] if k_ is not None else None
            for i, rr in enumerate(rows):
                for j, cc in enumerate(cols):
                    for k in range(levels):
                        dy, dx, got = tr[v, i, j, k]
                        want = L.block_score(r_, m_, v_[v], kv, (dy, dx), rr, cc)
                        assert np.isneginf(got) == np.isneginf(want)
                        if np.isfinite(want):
                            worst_score = max(worst_score, abs(float(got) - want))
                    n = L.common_valid(m_, kv, (H, W), tr[v, i, j, -1, :2], rr, cc)
                    area = (rr[1] - rr[0]) * (cc[1] - cc[0])
                    assert abs(n - LOCAL_MIN_VALID * area) > 0.0025 * area, "a block within 1 % of the threshold"
                    good = bool(np.isfinite(tr[v, i, j, -1, 2]) and n >= LOCAL_MIN_VALID * area)
                    assert bool(okn[v, i, j]) == good
                    assert np.array_equal(fl[v, i, j], tr[v, i, j, -1, :2] if good else init[b, v].numpy())
            exact = L.field_at_pixels(fl[v], H, W, block, rounded=False)
            assert np.abs(exact - np.round(exact)).min() > 1e-12
            want, want_valid, bil = L.sample_field(v_[v], kv, L.field_at_pixels(fl[v], H, W, block))
            off = np.abs(bil - 0.5)
            assert not ((off > 0.0) & (off <= 1e-9)).any()
            assert np.array_equal(got_valid[v], want_valid.astype(np.float32)) and np.all(got_out[v][~want_valid] == 0.0)
            worst_px = max(worst_px, float(np.abs(got_out[v] - want)[want_valid].max()) if want_valid.any() else 0.0)
        print(f"{tag} sample {b}: bit-identical to the sample alone; alone against fp64: trace scores {worst_score:.3e}, resampled pixels {worst_px:.3e}")
        assert worst_score <= SCORE_BOUND and worst_px <= APPLY_BOUND


# ----------------------------------------------------------------------------------------------------------- B: the local scene kernels
FRAME_IDS = [f"{a}-V{b}-{c}" for a, b, c in LC.FRAME_B]


def _rows(t, p, a, b, H, W):
    """rows a .. b - 1 of plane p of a (V, H, W) device tensor, on the host"""
    lo = p * H * W
    return t[lo + a * W:lo + b * W].view(b - a, W).cpu().numpy()


@pytest.mark.parametrize("masks,V,cross", LC.FRAME_B, ids=FRAME_IDS)
def test_scene_kernels_big_frame(pool, masks, V, cross):
    """Regime B for the kernels whose output pixel depends on a bounded neighbourhood: hrn_mncc_apply_scene, hrn_mncc_reduce2,
    hrn_mncc_apply_backward (d_views; `valid` and d_out = `out` from the forward of the same tensors) and hrn_mncc_apply_field (block 4096,
    a synthetic field of 4 x 4 nodes) on B = 1, V planes of 16002 x 16001.  Strips of 24 rows - top, middle, bottom of plane 0, of the last
    plane and of every plane with a crossing, and the strip around each crossing's row - against the fp64 restatement of the strip with
    its real neighbour rows, under the small-shape bounds; valid exactly.  The four kernels run one after the other on the same views:
    `views` is freed for d_views (which does not read it) and generated again, from the same seed, for the field and for reduce2, which
    runs last, when out and valid are gone"""
    import registration_local_ref as L
    import registration_pyramid_ref as Y
    import registration_ref as R
    import warp_ref as WR
    from registration_cases import APPLY_BOUND
    case = LC.frame_case(masks, V, cross)
    H, W, by, bx, block = case["H"], case["W"], case["by"], case["bx"], LC.FRAME_BLOCK
    hw, n = H * W, V * H * W
    _need(LC.gib(case["tensors"]))
    lib = _lib()
    assert (by, bx) == (lib.hrn_mncc_local_blocks(H, block), lib.hrn_mncc_local_blocks(W, block))

    def inputs():
        g = _gen(421)
        return _fill(pool, n, g, "uniform"), (_fill(pool, n, g, "mask", 0.15) if masks == "masks" else None)

    views, vm = inputs()
    shifts = torch.tensor(WR.SHIFTS[:6], dtype=torch.float32)[torch.arange(V) % 6].reshape(1, V, 2).contiguous()     # (300, 0) is beyond the sampler's clamp
    sd = shifts.cuda()
    out, valid = _nan_out(pool, n), _nan_out(pool, n)
    sums = [(t, _sum64(t)) for t in (views, vm) if t is not None]
    _apply(lib, views, vm, sd, 1, V, H, W, out, valid)
    assert all(_sum64(t) == c for t, c in sums) and _spare_ok(out, n) and _spare_ok(valid, n), "the launch wrote an input or past an output"
    strips = LC.frame_strips(V, H, W)
    tag = f"big frame {masks} V={V} {H}x{W}"
    _says(tag, cross, case["tensors"], strips)

    # 1. hrn_mncc_apply_scene
    worst = 0.0
    for p, y0, y1 in strips:
        s = shifts[0, p].numpy()
        a, b = LC.with_reach(H, y0, y1, abs(R.split(s[0])[0]) + 4)
        T = _rows(views, p, a, b, H, W)
        M = _rows(vm, p, a, b, H, W) if vm is not None else np.ones((b - a, W))
        sl = slice(y0 - a, y1 - a)
        off = np.abs(R.mask_bilinear(M, s)[sl] - 0.5)
        assert not ((off > 0.0) & (off <= 1e-9)).any()
        want_valid, want = R.shifted_mask(M, s)[sl], R.sample(T, s)[sl]
        got, got_valid = _rows(out, p, y0, y1, H, W), _rows(valid, p, y0, y1, H, W)
        assert np.array_equal(got_valid, want_valid.astype(np.float32)), f"{tag} apply_scene plane {p} rows {y0}..{y1}: valid"
        assert np.all(got[~want_valid] == 0.0) and want_valid.any()
        worst = max(worst, float(np.abs(got - want)[want_valid].max()))
    print(f"{tag} apply_scene: {len(strips)} strips, max |device - fp64| = {worst:.3e}")
    assert worst <= APPLY_BOUND

    # 2. hrn_mncc_apply_backward, d_views alone: it reads valid and d_out only
    for t in (views, vm):
        if t is not None:
            t.untyped_storage().resize_(0)
    d_views = _nan_out(pool, n)
    sums = [(t, _sum64(t)) for t in (valid, out)]
    _ok(lib, lib.hrn_mncc_apply_backward(NULL, _p(sd), _p(valid), _p(out), 1, V, H, W, _p(d_views), NULL, NULL, 0, NULL))
    assert all(_sum64(t) == c for t, c in sums) and _spare_ok(d_views, n), "the launch wrote an input or past its output"
    worst = 0.0
    for p, y0, y1 in strips:
        s = shifts[0, p].numpy()
        a, b = LC.with_reach(H, y0, y1, 2 * (abs(R.split(s[0])[0]) + 4))
        g, k = _rows(out, p, a, b, H, W), _rows(valid, p, a, b, H, W)
        sl = slice(y0 - a, y1 - a)
        want, mag = WR.d_views(g, k, s)[sl], WR.magnitudes(np.zeros_like(g), g, k, s)[0][sl]
        worst = max(worst, _assert_close(f"{tag} d_views plane {p} rows {y0}..{y1}", "f32", torch.from_numpy(_rows(d_views, p, y0, y1, H, W)).double(),
                                         torch.from_numpy(want), torch.from_numpy(mag), layout="y x"))
    print(f"{tag} d_views: max error / bound {worst:.3e}")
    d_views.untyped_storage().resize_(0)

    # 3. hrn_mncc_apply_field: the same views again, a field of by x bx nodes per view
    views, vm = inputs()
    out.fill_(float("nan")), valid.fill_(float("nan"))
    rng = np.random.default_rng(422)
    field = (rng.uniform(-2.5, 2.5, (1, V, by, bx, 2)) + 0.013).astype(np.float32)
    fd = torch.from_numpy(field).cuda()
    sums = [(t, _sum64(t)) for t in (views, vm) if t is not None]
    _ok(lib, lib.hrn_mncc_apply_field(_p(views), _opt(vm), _p(fd), 1, V, H, W, block, _p(out), _p(valid), NULL))
    assert all(_sum64(t) == c for t, c in sums) and _spare_ok(out, n) and _spare_ok(valid, n) and np.array_equal(fd.cpu().numpy(), field)
    worst = 0.0
    for p, y0, y1 in strips:
        a, b = LC.with_reach(H, y0, y1, 8)
        exact = L.field_at_pixels(field[0, p], H, W, block, rounded=False, rows=(y0, y1))
        assert np.abs(exact - np.round(exact)).min() > 1e-12 and np.abs(exact).max() < 4
        px = L.field_at_pixels(field[0, p], H, W, block, rows=(a, b))
        want, want_valid, bil = L.sample_field(_rows(views, p, a, b, H, W), _rows(vm, p, a, b, H, W) if vm is not None else None, px)
        sl = slice(y0 - a, y1 - a)
        off = np.abs(bil[sl] - 0.5)
        assert not ((off > 0.0) & (off <= 1e-9)).any()
        got, got_valid = _rows(out, p, y0, y1, H, W), _rows(valid, p, y0, y1, H, W)
        assert np.array_equal(got_valid, want_valid[sl].astype(np.float32)), f"{tag} apply_field plane {p} rows {y0}..{y1}: valid"
        assert np.all(got[~want_valid[sl]] == 0.0) and want_valid[sl].any()
        worst = max(worst, float(np.abs(got - want[sl])[want_valid[sl]].max()))
    print(f"{tag} apply_field: max |device - fp64| = {worst:.3e}")
    assert worst <= APPLY_BOUND

    # 4. hrn_mncc_reduce2 on the same planes, out and valid freed first: coarse rows y0 / 2 .. y1 / 2
    for t in (out, valid):
        t.untyped_storage().resize_(0)
    Hc, Wc = H // 2, W // 2
    red, red_mask = _nan_out(pool, V * Hc * Wc), _nan_out(pool, V * Hc * Wc)
    _reduce(lib, views, vm, V, H, W, red, red_mask)
    assert all(_sum64(t) == c for t, c in sums) and _spare_ok(red, V * Hc * Wc) and _spare_ok(red_mask, V * Hc * Wc)
    worst = 0.0
    for p, y0, y1 in strips:
        Y0, Y1 = y0 // 2, min(Hc, y1 // 2)
        a, b = max(0, 2 * Y0 - 2), min(H, 2 * Y1 + 2)
        want, clear, _ = Y.reduce2(_rows(views, p, a, b, H, W), _rows(vm, p, a, b, H, W) if vm is not None else None)
        sl = slice(Y0 - a // 2, Y1 - a // 2)
        got, got_clear = _rows(red, p, Y0, Y1, Hc, Wc), _rows(red_mask, p, Y0, Y1, Hc, Wc)
        assert np.array_equal(got_clear, clear[sl].astype(np.float32)) and np.all(got[~clear[sl]] == 0.0), f"{tag} reduce2 plane {p} rows {Y0}..{Y1}"
        worst = max(worst, float(np.abs(got - want[sl]).max()))
    print(f"{tag} reduce2: max |device - fp64| = {worst:.3e}")
    assert worst <= Y.REDUCE2_BOUND


# ----------------------------------------------------------------------------------------------------------- B: hrn_lanczos_shift on one big plane
@pytest.mark.parametrize("which", ["fwd", "bwd"], ids=["fwd-2^32B", "bwd-2^32B"])
def test_lanczos_shift_big_frame(pool, which):
    """hrn_lanczos_shift and the d_img half of hrn_lanczos_shift_backward on one plane of 33000 x 33001, past 2^32 bytes in-plane (2^31
    elements in one plane would be 8 GiB for each of img, d_out, d_img and the workspace).  Strips at the top (the reflected border), around
    the rows of byte 2^31 and byte 2^32 and at the bottom, against kernel_refs' restatement of the strip with four real neighbour rows,
    under C_TAIL"""
    import kernel_refs as K
    from kernel_bounds import C_TAIL
    H, W, reach = LC.LANCZOS_B["H"], LC.LANCZOS_B["W"], LC.LANCZOS_B["reach"]
    hw = H * W
    lib = _lib()
    ws_bytes = lib.hrn_lanczos_shift_backward_workspace_bytes(1, 1, H, W) if which == "bwd" else 0
    tensors = {k: hw for k in (("img", "out") if which == "fwd" else ("img", "d_out", "d_img"))}
    _need(LC.gib(tensors, ws_bytes))
    g = _gen(431)
    img = _fill(pool, hw, g, "uniform", 0.25, 0.75)
    shift = K.TAIL_SHIFTS[2:3].contiguous()                 # (0.37, -1.0): taps down the columns, a whole pixel along the rows
    sd = shift.cuda()
    if which == "fwd":
        src, dst = img, _nan_out(pool, hw)
        c0 = _sum64(img)
        _ok(lib, lib.hrn_lanczos_shift(_p(img), _p(sd), 1, 1, H, W, _p(dst), NULL))
        assert _sum64(img) == c0
    else:
        src, dst = _fill(pool, hw, g, "normal"), _nan_out(pool, hw)
        sums = [(t, _sum64(t)) for t in (img, src)]
        ws = pool.keep(torch.empty(ws_bytes, dtype=torch.uint8, device="cuda"))
        _ok(lib, lib.hrn_lanczos_shift_backward(_p(img), _p(sd), _p(src), 1, 1, H, W, _p(dst), NULL, _p(ws), ws_bytes, NULL))
        assert all(_sum64(t) == c for t, c in sums)
    assert _spare_ok(dst, hw), "a write past the output"
    strips = LC.frame_strips(1, H, W)
    tag = f"lanczos {which} {H}x{W} workspace {ws_bytes / GIB:.2f} GiB"
    _says(tag, "2^32B", tensors, strips)
    s64 = shift.double()
    worst = 0.0
    for _, y0, y1 in strips:
        a, b = LC.with_reach(H, y0, y1, reach)
        x = torch.from_numpy(_rows(src, 0, a, b, H, W)).double()[None, None]
        sl = slice(y0 - a, y1 - a)
        if which == "fwd":
            want, T = K.ref_lanczos_shift(x, s64), K.lanczos_shift_T(x, s64)
        else:
            want, T = K.ref_lanczos_grads(torch.zeros_like(x), s64, x)[0], K.lanczos_dimg_T(x, s64)
        got = torch.from_numpy(_rows(dst, 0, y0, y1, H, W))[None, None]
        worst = max(worst, _assert_close(f"{tag} rows {y0}..{y1}", "f32", got, want[:, :, sl], T[:, :, sl], layout="b c y x", c=C_TAIL))
    print(f"{tag}: {len(strips)} strips, max error / bound {worst:.3e}")


# ----------------------------------------------------------------------------------------------------------- B: the searched losses on one big frame
LOSS_B_IDS = [f"{a}-{b}x{c}-{'bwd-' if e else ''}{f}" for a, b, c, d, e, f in LC.LOSS_B]


@pytest.mark.parametrize("kind,H,W,option,backward,cross", LC.LOSS_B, ids=LOSS_B_IDS)
def test_searched_losses_big_frame(pool, kind, H, W, option, backward, cross):
    """hrn_shift_loss_*, hrn_cl1_loss_*, hrn_shift_cssim / hrn_cssim_loss_backward on B = 1 and one frame of 33000 x 33001 (past 2^32
    bytes in-plane), border 1, and hrn_shift_cssim at the int limit of cssim.hip, 46340 x 46340, whose last 64 rows reach within 2 W of
    pixel 2^31 (it fits the cap: three inputs of 8 GiB and 1.2 GiB of workspace).  The map is zero except in the checked strips, so every
    sum depends on those rows alone; the reference is the loss's own restatement on the stacked strips with their neighbour rows
    (shift_loss_ref.frame_of_row_ranges) under the small-shape tolerances.  cSSIM's map pixels over masked ground are exactly 1, so its
    score is 1 + (the stacked frame's score - 1) (stacked map pixels / the frame's map pixels), and its gradient scales alike.  d_srs is
    compared on the stacked rows and is exactly zero everywhere else.  Control: with srs in the strips past byte 2^32 read 2^32 bytes
    lower (what a wrapped offset would hit) the restatement must miss the output by more than the tolerance"""
    import shift_loss_ref as R
    import util
    border, hw = LC.LOSS_B_BORDER, H * W
    lib = _lib()
    if kind == "shift":
        ws_bytes = lib.hrn_shift_loss_workspace_bytes(1, H, W, border)
    elif kind == "cl1":
        ws_bytes = lib.hrn_cl1_loss_workspace_bytes(1, H, W, border)
    else:
        ws_bytes = max(lib.hrn_shift_cssim_workspace_bytes(1, H, W, border, option), lib.hrn_cssim_loss_backward_workspace_bytes(1, H, W, border, option))
    tensors = {k: hw for k in ["srs", "hrs", "maps"] + (["d_srs"] if backward else [])}
    _need(LC.gib(tensors, ws_bytes))
    g = _gen(441)
    srs, hrs, _ = _planted(pool, hw, W, border, False, g)
    _.untyped_storage().resize_(0)
    strips = LC.loss_b_strips(H, W)
    maps = pool.keep(torch.zeros(hw + SPARE, device="cuda"))
    maps[hw:] = float("nan")
    for y0, y1 in strips:
        maps[y0 * W:y1 * W].uniform_(generator=g).gt_(0.1)
    T = LC.CSSIM_TAPS[option] if kind == "cssim" else 1
    reach = 2 * border + T
    if kind == "cssim":
        # cssim_ref.scene's kind of frame in every row the sums can see: hr a smoothed field in [0.1, 0.9], sr = hr displaced by (1, -1),
        # x 0.9 + 0.03 plus N(0, 0.02^2).  CSSIM_GRAD_TOL is four times what the fp32 model of the kernel's algebra needs on such scenes
        # (1.5e-6 at most); on white noise under a strip map, whose edge windows are half masked, the model itself needs 2.1e-6 on the
        # CPU (and the kernel 6.4e-6 on the MI355X): outside what that bound was made for
        for y0, y1 in strips:
            a, b = max(0, y0 - reach), min(H, y1 + reach)
            big = torch.rand((b - a + 24, W + 24), device="cuda", generator=g)
            for _ in range(3):
                big = (big + big.roll(1, 0) + big.roll(-1, 0) + big.roll(1, 1) + big.roll(-1, 1)) / 5.0
            big = big[4:-4, 4:-4]
            big = 0.1 + 0.8 * (big - big.min()) / (big.max() - big.min())
            hrs[a * W:b * W].view(b - a, W).copy_(big[8:8 + b - a, 8:8 + W])
            noise = torch.randn((b - a, W), device="cuda", generator=g) * 0.02
            srs[a * W:b * W].view(b - a, W).copy_(big[9:9 + b - a, 7:7 + W] * 0.9 + 0.03 + noise)
    x = (srs, hrs, maps)
    d_out = torch.tensor([D_OUT[1]], device="cuda")
    d_srs = _nan_out(pool, hw) if backward else None
    sums = [(t, _sum64(t)) for t in x]
    if kind == "shift":
        out, stats = _loss(lib, *x, 1, H, W, border, "cPSNR", False, d_out, d_srs)
        scores = None
    else:
        out, stats, scores = _searched(lib, kind, x, 1, H, W, border, option, False, d_out, d_srs)
    assert all(_sum64(t) == c for t, c in sums) and (d_srs is None or _spare_ok(d_srs, hw)), "a launch wrote an input or past d_srs"
    tag = f"{kind} big frame {H}x{W} border {border} workspace {ws_bytes / GIB:.2f} GiB"
    got = crossed(hw, 4)
    print(f"{tag}: each of {list(tensors)} {hw * 4 / GIB:.2f} GiB {got}; the map is clear in rows {strips}")
    assert ("2^32B" in got and len(strips) >= 5) if cross == "2^32B" else (hw <= 2 ** 31 - 1 and hw + 2 * W > 1 << 31 and strips[-1] == (H - 64, H))
    rows_of = lambda lower=0: (lambda a, b: tuple(t[(a - lo) * W:(b - lo) * W].view(b - a, W).cpu() for t, lo in zip(x, (lower, 0, 0))))
    small, windows = R.frame_of_row_ranges(rows_of(), strips, H, reach)
    Hs = small[0].shape[1]
    scale = ((Hs - 2 * border - T + 1) / (H - 2 * border - T + 1)) if kind == "cssim" else 1.0

    def restated(frame, with_grad=backward):
        """-> (what `out` should be, the selected offset, d out / d srs on the stacked rows)"""
        if kind == "cssim":
            import cssim_grad_ref as G
            import cssim_ref as CR
            s, h, m = (t[0].numpy() for t in frame)
            sc, k, bias, n = CR.shift_cssim(s, h, m, border, WINDOWS[option], False, True, 1.0)
            full = 1.0 + (sc - 1.0) * scale
            if with_grad is not None:                        # (not for the control's frame) the best offset leads, stacked and in the frame's own score
                assert CR.gap(sc) >= 1e-3 and CR.gap(full) > 10 * 2e-6
            grad = G.grad(s, h, m, k, border, WINDOWS[option], False, True, 1.0) * scale if with_grad else None
            return full, k, grad
        s = frame[0].double().requires_grad_(True)
        if kind == "shift":
            want, k, cm = R.shift_loss(s, frame[1], frame[2], "cPSNR", border, False)
        else:
            import cl1_ref
            want, k, cm, _ = cl1_ref.cl1_loss(s, frame[1], frame[2], border, False, float(np.float32(option)))
        assert with_grad is None or float(R.top_two_gap(cm).min()) > 1e-6
        want.sum().backward()
        return want.detach().numpy(), int(k[0]), s.grad[0].numpy()

    def miss(want, k):
        """how far the device's result is from a restatement, in units of the tolerance"""
        if kind == "cssim":
            import cssim_cases as CC
            nk = (2 * border + 1) ** 2
            return float(np.abs(scores[:nk].cpu().numpy() - want).max()) / CC.TOL
        return util.rel_err(out[:1].cpu().numpy(), want) / R.TOL

    want, k, grad = restated(small)
    e = miss(want, k)
    print(f"{tag}: against the restatement of the stacked strips ({Hs} rows): error / tolerance {e:.3e}; offset {k}")
    assert e <= 1.0 and int(stats[3]) == k
    if backward:
        import cssim_grad_ref as G
        from cssim_loss_bounds import CSSIM_GRAD_TOL
        got_rows = torch.cat([d_srs[a * W:b * W].view(b - a, W).cpu() for a, b in windows]).double().numpy()
        eg = G.rel_err(got_rows, D_OUT[1] * grad)
        tol = CSSIM_GRAD_TOL if kind == "cssim" else R.GRAD_TOL
        inside = int(np.count_nonzero(got_rows))
        everywhere = int(torch.count_nonzero(d_srs[:hw]))
        print(f"{tag}: d_srs on the stacked rows: error / max |gradient| {eg:.3e} (tolerance {tol:g}); {inside} non-zero there, {everywhere} in the frame")
        assert eg <= tol and inside == everywhere and inside > 0
    # control: the strips past byte 2^32, restated on the rows 2^32 bytes lower
    lower = (1 << 30) // W
    wrong_parts, told = [], 0
    for (y0, y1), (a, b) in zip(sorted(strips), windows):
        wrapped = y1 * W > 1 << 30                          # wholly or partly past byte 2^32
        told += wrapped
        wrong_parts.append(rows_of(min(lower, a) if wrapped else 0)(a, b))
    if cross == "2^32B":
        assert told >= 2
        wrong = tuple(torch.cat([p[i] for p in wrong_parts])[None] for i in range(3))
        w_want, w_k, _ = restated(wrong, None)
        e = miss(w_want, w_k)
        print(f"{tag}: against the restatement with {told} strips read 2^32 bytes lower: error / tolerance {e:.3e}")
        assert e > 1.0, "the comparison does not tell a wrapped row offset"


# ----------------------------------------------------------------------------------------------------------- B: the scene kernels that sum over the frame
def _stack(t, base, blocks, W, lower=0):
    """the windows (block + SUM_REACH around it) of the plane that starts at element `base` of the flat device tensor t, stacked on the
    host; lower: elements to read below (the control)"""
    r = LC.SUM_REACH
    parts = []
    for y0, y1, x0, x1 in blocks:
        lo = base - (lower if base + (y0 - r) * W >= lower else 0)
        parts.append(torch.as_strided(t, (y1 - y0 + 2 * r, x1 - x0 + 2 * r), (W, 1), lo + (y0 - r) * W + x0 - r).cpu())
    return torch.cat(parts).numpy()


@pytest.mark.parametrize("masks,V,cross", LC.FRAME_B, ids=FRAME_IDS)
def test_scene_sums_big_frame(pool, masks, V, cross):
    """Regime B for hrn_mncc_grid_scene, hrn_mncc_search_scene and the d_shifts half of hrn_mncc_apply_backward on the 16002 x 16001
    stack: the mask that gates the sum - ref_mask for the scores, `valid` for d_shifts - is zero except in blocks of 24 x 256 pixels at the
    rows of every crossing and at the top, middle and bottom, so the results depend on those pixels alone.  The reference is the
    restatement on the stacked blocks, each with 8 pixels around it, under the small-shape bounds.  Control: with the last view's blocks
    past byte 2^32 read 2^32 bytes lower, the restated scores must miss the device's by more than the bound"""
    import registration_ref as R
    import warp_ref as WR
    from registration_cases import GRID_BOUND
    case = LC.frame_case(masks, V, cross)
    H, W = case["H"], case["W"]
    hw, n, P, levels = H * W, V * H * W, LC.MNCC_P, LC.MNCC_LEVELS
    lib = _lib()
    ws_bytes = lib.hrn_mncc_scene_workspace_bytes(1, V, H, W, P)
    _need(LC.gib({"views": n, "d_out": n, "valid": n}, ws_bytes))          # the d_shifts half holds the most
    blocks = LC.sum_blocks(V, H, W)
    g = _gen(451)
    ref, _, views, vm = _scene_inputs(pool, 1, V, H, W, False, g)
    if masks == "masks":
        vm = _fill(pool, n, g, "mask", 0.15)

    def sparse(planes):
        m = pool.keep(torch.zeros(planes * hw + SPARE, device="cuda"))
        m[planes * hw:] = float("nan")
        for p in range(planes):
            for y0, y1, x0, x1 in blocks:
                m[p * hw:(p + 1) * hw].view(H, W)[y0:y1, x0:x1].uniform_(generator=g).gt_(0.15)
        return m

    rm = sparse(1)
    centres = torch.tensor(GRID_CENTRES[:3], dtype=torch.float32)[torch.arange(V) % 3].reshape(1, V, 2).contiguous()
    cd = centres.cuda()
    sums = [(t, _sum64(t)) for t in (ref, rm, views, vm) if t is not None]
    scores, shifts, trace = _search_scene(lib, ref, rm, views, vm, cd, 1, V, H, W)
    assert all(_sum64(t) == c for t, c in sums), "a launch wrote one of its inputs"
    tag = f"scene sums {masks} V={V} {H}x{W} workspace {ws_bytes / GIB:.2f} GiB"
    _says(tag, cross, {"views": n, **({"view_masks": n} if vm is not None else {}), "ref": hw}, blocks)
    r_s, rm_s = _stack(ref, 0, blocks, W), _stack(rm, 0, blocks, W)
    got_scores = scores[:V * P * P].view(V, P, P).cpu().numpy().astype(np.float64)
    got_trace = trace[:V * levels * 3].view(V, levels, 3).cpu().numpy()
    assert np.array_equal(shifts[:V * 2].view(V, 2).cpu().numpy(), got_trace[:, -1, :2])
    widths = R.level_widths(P, levels, SEARCH_RADIUS)
    worst, told = 0.0, 0
    for v in range(V):
        v_s = _stack(views, v * hw, blocks, W)
        m_s = _stack(vm, v * hw, blocks, W) if vm is not None else None
        want = R.grid(r_s, rm_s, v_s, m_s, centres[0, v].numpy(), np.float32(GRID_WIDTH), P)[0]
        assert np.isfinite(want).all() and np.isfinite(got_scores[v]).all()
        worst = max(worst, float(np.abs(got_scores[v] - want).max()))
        centre = (np.float32(0.0), np.float32(0.0))
        for k in range(levels):
            lvl, dys, dxs = R.grid(r_s, rm_s, v_s, m_s, centre, widths[k], P)
            dy, dx, got = got_trace[v, k]
            i, j = np.flatnonzero(dys == dy), np.flatnonzero(dxs == dx)
            assert len(i) and len(j) and lvl.max() - lvl[i[0], j[0]] <= 2 * GRID_BOUND
            worst = max(worst, abs(got - lvl[i[0], j[0]]))
            centre = (dy, dx)
        if v == V - 1:
            wrong = R.grid(r_s, rm_s, _stack(views, v * hw, blocks, W, lower=1 << 30), m_s, centres[0, v].numpy(), np.float32(GRID_WIDTH), P)[0]
            miss = float(np.abs(got_scores[v] - wrong).max())
            print(f"{tag}: view {v} against the restatement of its blocks read 2^32 bytes lower: {miss / GRID_BOUND:.3e} bounds")
            assert miss > GRID_BOUND, "the comparison does not tell a wrapped offset"
            told += 1
    print(f"{tag}: grid_scene and search_scene against the restatement of {len(blocks)} stacked blocks: {worst:.3e}")
    assert worst <= GRID_BOUND and told == 1

    # d_shifts: `valid` clear in the same blocks of every view, d_out dense
    for t in (ref, rm, vm):
        if t is not None:
            t.untyped_storage().resize_(0)
    valid = sparse(V)
    d_out = _fill(pool, n, g, "normal")
    sh = torch.tensor(WR.SHIFTS[:5], dtype=torch.float32)[torch.arange(V) % 5].reshape(1, V, 2).contiguous()     # |whole part| + 3 <= SUM_REACH
    sd = sh.cuda()
    d_shifts = torch.full((2 * V + SPARE,), float("nan"), device="cuda")
    nbytes = lib.hrn_mncc_apply_backward_workspace_bytes(1, V, H, W)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    sums = [(t, _sum64(t)) for t in (views, valid, d_out)]
    _ok(lib, lib.hrn_mncc_apply_backward(_p(views), _p(sd), _p(valid), _p(d_out), 1, V, H, W, NULL, _p(d_shifts), _p(ws), nbytes, NULL))
    assert all(_sum64(t) == c for t, c in sums) and _spare_ok(d_shifts, 2 * V), "the launch wrote an input or past its output"
    got = d_shifts[:2 * V].view(V, 2).cpu().numpy().astype(np.float64)
    worst = 0.0
    for v in range(V):
        a = (_stack(views, v * hw, blocks, W), _stack(d_out, v * hw, blocks, W), _stack(valid, v * hw, blocks, W), sh[0, v].numpy())
        want, mag = WR.d_shifts(*a), WR.magnitudes(*a)[1]
        err, bound = np.abs(got[v] - want), 2.0 ** -24 * np.abs(want) + C * mag
        worst = max(worst, float((err / bound).max()))
        assert np.all(err <= bound) and np.abs(want).max() > 0, (tag, v, got[v], want, bound)
        if v == V - 1:
            w = WR.d_shifts(_stack(views, v * hw, blocks, W, lower=1 << 30), *a[1:])
            assert np.any(np.abs(got[v] - w) > 2.0 ** -24 * np.abs(w) + C * mag), "the comparison does not tell a wrapped offset"
    print(f"{tag}: d_shifts against the restatement of the stacked blocks: max error / bound {worst:.3e}")
