"""The cases of tests/test_gpu_large_offsets_scene.py (GPU) and what tests/test_large_offsets_host.py shows about them on the CPU: the
shapes, the batch that makes a tensor cross what the case id names, the tensors of each launch (name -> f32 elements) and the device
memory a case asks for before it allocates.  Every tensor here is f32, so 2^32 bytes is element 2^30.  Nothing here needs the GPU or the
compiled package.

A  deep batch   many small planes; B = TOP[cross] // per + 2, so one whole plane lies behind the crossing.
B  big frame    few planes near an entry point's own limit."""
GIB = 1 << 30
SHAPES = {"64x64": (64, 64), "33x50": (33, 50), "50x50": (50, 50), "192x192": (192, 192), "181x203": (181, 203), "128x256": (128, 256)}
TOP = {"2^31el": 1 << 31, "2^32B": 1 << 30}            # f32 elements a tensor must exceed
CAP_GIB = 32                                             # the `pool` fixture's cap on a test's peak device memory
LOSS_BATCH_MAX = 65535                                   # api.hip: "batch %d exceeds the grid limit"
SIDE_MAX = 16384                                         # the scene entry points' sides


def count(cross, per):
    """planes of `per` elements so that the tensor crosses `cross`, with one whole plane behind the crossing"""
    return TOP[cross] // per + 2


def gib(tensors, extra_bytes=0):
    """device memory asked for: the tensors, their spare words, the alone launches and the allocator's slack (2 GiB)"""
    return (4 * sum(tensors.values()) + extra_bytes) / GIB + 2


def checked_planes(*pairs):
    """the planes checked of a launch whose tensors are (M planes, elements per plane) pairs, all f32 and sharing the plane index: the union
    of kernel_bounds.boundary_images - plane 0, the last plane, the plane(s) at every crossing - and, where ragged planes straddle their
    crossings and that leaves fewer than five, the plane behind each crossing plane as well"""
    from kernel_bounds import boundary_images
    out = set()
    for M, per in pairs:
        out |= set(boundary_images(M, per, 4))
    M = min(m for m, _ in pairs)
    if len(out) < 5:
        out |= {m + 1 for m in out if 0 < m < M - 1}
    return sorted(out)


# ----------------------------------------------------------------------------------------------------------- hrn_mncc_apply_scene
V_APPLY = 2                                              # two views per sample: the plane base is (b V + v) H W
APPLY_A = [("masks", "64x64", "2^32B"), ("null", "64x64", "2^31el"), ("null", "33x50", "2^31el")]


def apply_case(masks, shape, cross):
    """with masks the launch has four tensors of one size: 4 x 8 GiB at 2^31 elements is the whole cap, so that case stops past 2^32 B"""
    H, W = SHAPES[shape]
    per = V_APPLY * H * W
    B = count(cross, per)
    names = ["views", "out", "out_valid"] + (["view_masks"] if masks == "masks" else [])
    return dict(B=B, V=V_APPLY, H=H, W=W, per=per, tensors={n: B * per for n in names})


# ----------------------------------------------------------------------------------------------------------- hrn_mncc_apply_backward
# "both": d_views and d_shifts with the view masks in the forward: views, masks, out (= d_out), valid, d_views: five tensors, past 2^32 B.
# "d_views": that half alone needs no `views`: the forward runs without masks, `views` is freed, `out` serves as d_out: 3 x 8 GiB at once.
BACKWARD_A = [("both", "64x64", "2^32B"), ("both", "33x50", "2^32B"), ("d_views", "64x64", "2^31el")]


def backward_case(which, shape, cross):
    H, W = SHAPES[shape]
    per = V_APPLY * H * W
    B = count(cross, per)
    names = ["views", "d_out", "valid", "d_views"] + (["view_masks"] if which == "both" else [])
    held = len(names) - (1 if which == "d_views" else 0)         # "d_views": views is gone before d_views exists
    return dict(B=B, V=V_APPLY, H=H, W=W, per=per, tensors={n: B * per for n in names}, held=held)


# ----------------------------------------------------------------------------------------------------------- hrn_mncc_grid_scene / _search_scene
# V = 2 views per sample, so ref [B][H][W] is half the views' size (its byte crossings fall on the samples of the views' next crossings):
# the union of both tensors' boundary samples is checked.  P is
# the smallest mncc_check_points allows, with two levels.
MNCC_P, MNCC_LEVELS = 3, 2
SEARCH_A = [("masks", "64x64", "2^31el"), ("masks", "33x50", "2^31el")]


def search_case(masks, shape, cross):
    H, W = SHAPES[shape]
    per = V_APPLY * H * W
    B = count(cross, per)
    t = {"views": B * per, "ref": B * H * W}
    if masks == "masks":
        t.update(view_masks=B * per, ref_mask=B * H * W)
    return dict(B=B, V=V_APPLY, H=H, W=W, per=per, tensors=t, tiles=B * V_APPLY * -(-H // 64) * -(-W // 64))


# ----------------------------------------------------------------------------------------------------------- hrn_mncc_search_local / _apply_field
# the smallest legal block, 64: one block on 64 x 64, two per axis on the ragged 100 x 130.  The search holds ref, ref_mask, views,
# view_masks; the resampling views, view_masks, out, out_valid: with masks four tensors of the views' size, past 2^32 B; without, the
# reference is freed before out and out_valid exist and the views pass 2^31 elements.
LOCAL_BLOCK = 64
SHAPES["100x130"] = (100, 130)
LOCAL_A = [("masks", "64x64", "2^32B"), ("null", "64x64", "2^31el"), ("masks", "100x130", "2^32B")]


def local_blocks(L, block=LOCAL_BLOCK):
    """hrn_mncc_local_blocks"""
    return max(1, (L + block // 2) // block)


def local_case(masks, shape, cross):
    H, W = SHAPES[shape]
    per = V_APPLY * H * W
    B = count(cross, per)
    t = {"views": B * per, "out": B * per, "out_valid": B * per}
    if masks == "masks":
        t.update(view_masks=B * per)
    search = {"ref": B * H * W, **({"ref_mask": B * H * W} if masks == "masks" else {})}
    return dict(B=B, V=V_APPLY, H=H, W=W, per=per, tensors=t, search=search, by=local_blocks(H), bx=local_blocks(W),
                tiles=B * V_APPLY * -(-H // 64) * -(-W // 64))


# ----------------------------------------------------------------------------------------------------------- hrn_mncc_reduce2
REDUCE_A = [("masks", "64x64", "2^31el"), ("masks", "33x50", "2^31el"), ("null", "33x50", "2^31el")]


def reduce_case(masks, shape, cross):
    H, W = SHAPES[shape]
    N = count(cross, H * W)
    t = {"x": N * H * W, "out": N * (H // 2) * (W // 2), "out_mask": N * (H // 2) * (W // 2)}
    if masks == "masks":
        t["mask"] = N * H * W
    return dict(N=N, H=H, W=W, tensors=t)


# ----------------------------------------------------------------------------------------------------------- hrn_shift_loss_*
# (shape, border, metric, clip, backward, cross).  The batch is capped at 65535, so the planes are 192 x 192 and a ragged 181 x 203; the
# three inputs at 2^31 elements are 24 GiB, and d_srs would be a fourth 8 GiB: the case past 2^31 elements runs the forward alone and the
# backward's cases stop past 2^32 B.  128 x 256 is the shape at which 2^32 bytes are a whole number of planes (the control).
LOSS_A = [("192x192", 1, "cMSE", False, False, "2^31el"), ("181x203", 3, "cPSNR", True, True, "2^32B"), ("128x256", 1, "cPSNR", False, True, "2^32B")]


def loss_case(shape, border, metric, clip, backward, cross):
    H, W = SHAPES[shape]
    B = count(cross, H * W)
    B += B & 1                                           # an even batch: the checksum reads pairs of words
    names = ["srs", "hrs", "maps"] + (["d_srs"] if backward else [])
    return dict(B=B, H=H, W=W, border=border, tensors={n: B * H * W for n in names})


# the other two searched losses: (kind, shape, border, option, clip, backward, cross); option is eps for cl1 (0: L1, 1e-3: Charbonnier) and
# the window for cssim (0 gaussian, 1 uniform).  Their inputs carry a planted offset (the SR crop is the HR window at PLANT plus noise), so
# that no checked sample is near a tie of its two best offsets; the forward's workspace is part of what a case asks for.
PLANT = (0, 2)                                           # (u, v), inside every border >= 1
SEARCHED_A = [("cl1", "192x192", 1, 0.0, False, False, "2^31el"), ("cl1", "181x203", 3, 1e-3, True, True, "2^32B"),
              ("cssim", "192x192", 1, 1, False, False, "2^31el"), ("cssim", "181x203", 3, 0, True, True, "2^32B")]


def searched_case(kind, shape, border, option, clip, backward, cross):
    return loss_case(shape, border, None, clip, backward, cross)


# ----------------------------------------------------------------------------------------------------------- hrn_lanczos_shift (+ backward)
# b = 1, c = planes (b c <= 65535, the grid limit of lanczos.hip and lanczos_bwd.hip).  The backward has img, d_out, d_img and a workspace
# as large as one of them: past 2^32 bytes.
LANCZOS_A = [("fwd", "192x192", "2^31el"), ("fwd", "181x203", "2^31el"), ("bwd", "192x192", "2^32B"), ("bwd", "181x203", "2^32B")]


def lanczos_case(which, shape, cross):
    H, W = SHAPES[shape]
    c = count(cross, H * W)
    c += c & 1
    names = ["img", "out"] if which == "fwd" else ["img", "d_out", "d_img"]
    return dict(c=c, H=H, W=W, tensors={n: c * H * W for n in names})


# ----------------------------------------------------------------------------------------------------------- hrn_dihedral_*
# (path, shape, codes): all eight members on square planes (W % 4 == 0: the 16-byte path; W = 50: per element), and the four codes that
# do not transpose on 33 x 50.  member_elems > 2^31 / K, so the last member of the (K, N, H, W) stack reaches past element 2^31.
DIHEDRAL = [("vec", "64x64", (2, 5, 0, 7, 1, 6, 3, 4)), ("elem", "50x50", (2, 5, 0, 7, 1, 6, 3, 4)), ("elem", "33x50", (2, 0, 3, 1))]
DIHEDRAL_TILE = 32
DIHEDRAL_MAX_TILES = (1 << 24) - 1                       # dihedral.hip kMaxTiles (16-byte path)


def dihedral_case(path, shape, codes):
    H, W = SHAPES[shape]
    K = len(codes)
    N = (1 << 31) // K // (H * W) + 2
    tiles = N * -(-H // DIHEDRAL_TILE) * -(-W // DIHEDRAL_TILE)
    return dict(N=N, K=K, H=H, W=W, member_elems=N * H * W, tiles=tiles, tensors={"x": N * H * W, "stack": K * N * H * W, "mean": N * H * W})


# ----------------------------------------------------------------------------------------------------------- hrn_collate_device(_m)
COLLATE_SIDE = 16                                        # stored LR images of 16 x 16 uint16: 256 elements, so every crossing is an image start
COLLATE_ODD = 13                                         # one odd stored side: 169 elements from a 4-aligned offset can end ONE element past
COLLATE_S = (4, 6)                                       # S % 4 == 0: the 16-byte path; 6: per element
COLLATE_CODES = (0, 3, 5)
COLLATE_CORNER = (5, 3)


def collate_case():
    """-> L (elements of the LR and QM arenas: 2^31 + four images) and the plan's rows as (side, [LR offsets], what) - offsets on either
    side of element 2^30 (byte 2^31), of element 2^31 (byte 2^32), at 0 and at the last image; the odd-sided rows at the very end: one
    that ends at L - 3 (good) and one that ends at L + 1 (NaN)"""
    v = COLLATE_SIDE * COLLATE_SIDE
    L = (1 << 31) + 4 * v
    rows = [(COLLATE_SIDE, [0, (1 << 30) - v], "good"), (COLLATE_SIDE, [1 << 30, (1 << 31) - v], "good"),
            (COLLATE_SIDE, [1 << 31, L - v], "good"), (COLLATE_SIDE, [(1 << 31) + v, -1], "good"),
            (COLLATE_ODD, [L - COLLATE_ODD * COLLATE_ODD - 3, 0], "good"), (COLLATE_ODD, [L - COLLATE_ODD * COLLATE_ODD + 1, 0], "slot 0 NaN")]
    return L, rows


# ----------------------------------------------------------------------------------------------------------- B: the local scene kernels
# hrn_mncc_apply_scene, hrn_mncc_apply_backward (d_views), hrn_mncc_reduce2, hrn_mncc_apply_field on B = 1 and V planes of 16002 x 16001
# (inside the 16384 limit, ragged, 64 divides neither side): V = 5 with masks passes 2^32 bytes (four tensors of 4.8 GiB), V = 9 without
# masks passes 2^31 elements (three of 8.6 GiB).  A strip is checked against the whole-frame restatement run on the strip plus as many real
# neighbour rows as the kernel reaches; only the strip's own rows are compared.
FRAME_H, FRAME_W, FRAME_BLOCK = 16002, 16001, 4096
FRAME_B = [("masks", 5, "2^32B"), ("null", 9, "2^31el")]
STRIP_ROWS = 24


def frame_case(masks, V, cross):
    n = V * FRAME_H * FRAME_W
    names = ["views", "out", "out_valid"] + (["view_masks"] if masks == "masks" else [])
    return dict(V=V, H=FRAME_H, W=FRAME_W, tensors={k: n for k in names},
                by=local_blocks(FRAME_H, FRAME_BLOCK), bx=local_blocks(FRAME_W, FRAME_BLOCK))


def frame_strips(V, H, W, rows=STRIP_ROWS):
    """(plane, y0, y1): top, middle and bottom strips of `rows` rows (even starts: reduce2 halves them) in plane 0, the last plane and
    every plane that holds a crossing of the (V, H, W) f32 tensor, and the strip around each crossing's row"""
    from kernel_bounds import crossings
    hw = H * W
    cross = crossings(V * hw, 4)
    planes = sorted({0, V - 1} | {e // hw for e in cross})
    mid = (H // 2) & ~1
    out = {(p, y0, y0 + rows) for p in planes for y0 in (0, mid, (H - rows) & ~1)}
    for e in cross:
        r = ((e % hw) // W) & ~1
        y0 = min(max(0, r - rows // 2), (H - rows) & ~1)
        out.add((e // hw, y0, y0 + rows))
    return sorted(out)


SUM_REACH, SUM_INSET, SUM_BAND = 8, 16, 256


def sum_blocks(V, H, W):
    """Regime B for the scene kernels whose result is a sum over the frame (grid_scene, search_scene, d_shifts): the gating mask is clear
    only in blocks - the rows of frame_strips (of every plane, so the rows of the view stack's crossings are among them) x three bands of
    256 columns (left, middle, right), all at least SUM_INSET pixels inside the frame, so that no clear pixel's footprint leaves it.
    -> [(y0, y1, x0, x1)]; a block's window, the block and SUM_REACH pixels around it, is what the restatement stacks"""
    rows = sorted({(max(SUM_INSET, y0), min(H - SUM_INSET, y1)) for _, y0, y1 in frame_strips(V, H, W)})
    mid = (W // 2) & ~1
    cols = [(SUM_INSET, SUM_INSET + SUM_BAND), (mid, mid + SUM_BAND), (W - SUM_INSET - SUM_BAND, W - SUM_INSET)]
    return [(y0, y1, x0, x1) for y0, y1 in rows for x0, x1 in cols]


def with_reach(H, y0, y1, reach):
    """the rows a strip's restatement is run on: the strip and `reach` real neighbour rows on either side, cut at the frame's edges"""
    return max(0, y0 - reach), min(H, y1 + reach)


# hrn_lanczos_shift forward and backward (d_img) on ONE plane of 33000 x 33001: past 2^32 bytes in-plane; 2^31 elements in one plane
# would be 8 GiB for each of img, d_out, d_img and the workspace
LANCZOS_B = dict(H=33000, W=33001, reach=4)


# The three searched losses on ONE frame of 33000 x 33001 (past 2^32 bytes in-plane; srs, hrs, maps and d_srs), border 1, and the score at
# the int limit of cssim.hip's in-plane indices, 46340 x 46340 (H W = 2 147 395 600 <= 2^31 - 1; srs, hrs, maps of 8 GiB and a workspace of
# 1.2 GiB).  The map is zero except in the checked strips, so the sums depend on those rows only: a kernel that reads a wrapped offset sees
# masked or different pixels.  (kind, H, W, option, backward, cross)
LOSS_B = [("shift", 33000, 33001, 2, True, "2^32B"), ("cl1", 33000, 33001, 1e-3, True, "2^32B"), ("cssim", 33000, 33001, 1, True, "2^32B"),
          ("cssim", 46340, 46340, 1, False, "2^31-1px")]
LOSS_B_BORDER = 1
LOSS_B_ROWS = 8                                          # rows per strip: the fp64 restatements of 33001-pixel rows are what a case's time goes to
CSSIM_TAPS = {0: 11, 1: 7}


def loss_b_strips(H, W):
    """the row ranges in which the map is clear: frame_strips' five (of LOSS_B_ROWS rows) for 33000 x 33001; a top strip and the last 64
    rows at the int limit"""
    if H * W > 1 << 31 - 1 and H == 46340:
        return [(0, STRIP_ROWS), (H - 64, H)]
    return [(y0, y1) for _, y0, y1 in frame_strips(1, H, W, LOSS_B_ROWS)]


# ----------------------------------------------------------------------------------------------------------- hrn_tile_gather / _scatter
TILE_T, TILE_LAYERS = 128, 2
TILE_MAX_ROWS = 1 << 31                                  # tile.hip kMaxRows, exclusive


def tile_halo(num_layers, V):
    """hrn_hrnet_halo / tiling.halo: 2 + 2 num_layers + 3 floor(log2 V)"""
    return 2 + 2 * num_layers + 3 * (V.bit_length() - 1)


def axis_count(L, t, R):
    return 1 if L == t else -(-(L - 2 * R) // (t - 2 * R))


def gather_case():
    """one scene of (1, 9) planes of 16002 x 16001 (inside 16384, ragged, 64 divides neither side): the planes pass 2^31 elements; every
    window of the plan in one launch, whose output passes 2^31 elements too"""
    B, V, H, W, t = 1, 9, 16002, 16001, TILE_T
    R = tile_halo(TILE_LAYERS, V)
    ny, nx = axis_count(H, t, R), axis_count(W, t, R)
    n = ny * nx
    return dict(B=B, V=V, H=H, W=W, t=t, R=R, ny=ny, nx=nx, windows=n, rows=n * B * V * t, tensors={"lrs": B * V * H * W, "out": n * B * V * t * t})


def scatter_case():
    """x3 into one plane of 36000 x 36003: 5.2e9 bytes, 1.296e9 pixels (under the INT32_MAX pixel guard); the windows in two launches
    around one band of window rows that is left out"""
    B, V, H, W, t, S = 1, 9, 12000, 12001, TILE_T, 3
    R = tile_halo(TILE_LAYERS, V)
    ny, nx = axis_count(H, t, R), axis_count(W, t, R)
    n = ny * nx
    skip = (ny // 3 * nx, (ny // 3 + 1) * nx)            # one whole row of windows, away from every crossing
    return dict(B=B, H=H, W=W, t=t, R=R, S=S, ny=ny, nx=nx, windows=n, skip=skip, rows=n * B * S * t,
                tensors={"srs": n * B * S * t * S * t, "out": B * S * H * S * W, "ref": B * S * H * S * W})


# the smallest refused shapes (square, scale 2 / any border): one pixel row and column beyond the last accepted square
SCATTER_REFUSED = dict(H=23171, W=23171, S=2)            # 4 x 23171^2 = 2 147 580 964 > 2^31 - 1 >= 4 x 23170^2
CSSIM_REFUSED = dict(H=46341, W=46341)                   # 46341^2 = 2 147 488 281 > 2^31 - 1 >= 46340^2
