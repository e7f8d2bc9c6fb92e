// Flip / rotate self-ensemble at inference (HRNet.forward_ensemble): the two steps around the K forwards.
//   hrn_dihedral_expand  x (N,H,W) -> out (K,N,H,W), out[k][n] = apply(x[n], codes[k])
//   hrn_dihedral_mean    y (K,N,H,W) -> out (N,H,W),  out[n] = r * ((..(m_0 + m_1)..) + m_{K-1}),  m_k = apply(y[k][n], inverse(codes[k]))
// with apply / inverse of hrnet_hip/augment.py (transpose if t & 4, then flip rows if t & 2, then flip columns if t & 1):
//     i' = t & 2 ? H-1-i : i,   j' = t & 1 ? W-1-j : j,   out[i][j] = in[t & 4 ? (j', i') : (i', j')].
// The member list is a host array, validated before any launch, and travels by value: eight 4-bit fields of one kernel argument
// (hrn_dihedral_mean is handed the inverse codes), so every branch on a code is uniform over the block.  Pure data movement: both
// kernels move (1 + K) N H W 4 bytes, one launch each, no atomics.  The sum is fp32 adds in list order and ONE fp32 multiply by
// r = (float)(1.0 / K) - nothing a compiler could contract into an fma, no division - so augment.mean_inverse restates it bit for bit.
//
// Vector path (W % 4 == 0, 16-byte aligned pointers): a block owns one kTile x kTile tile of a plane, a lane 4 consecutive elements of
// one of its rows (lane -> row lr = lane / 8, columns lq = 4 (lane % 8) .. lq + 3), moved by 16-byte global loads and stores.  Edge
// tiles are ragged in multiples of 4 columns (and, where a code transposes, of 4 rows: H == W then).
//   expand  owns a SOURCE tile: one load, then one store per member.  t in 0..3: a row flip is an address; a column flip mirrors the
//           column start (c -> W-4-c, still a multiple of 4) and reverses the lane's four values.  If any member transposes, the tile
//           also goes through LDS once (4 ds_write_b32 down a column, one barrier, one ds_read_b128 along a row) and every
//           transposing member stores that transposed copy, flips applied the same way.  x is read once, whatever K.
//   mean    owns an OUTPUT tile and loops over the members IN LIST ORDER with one f32x4 accumulator per lane.  A member whose inverse
//           code is in 0..3 is one mirrored 16-byte load; one in 4..7 is loaded along source rows, written down a column of an LDS
//           tile and read back along a row, into the same accumulator - the order of the adds never depends on the path.  Two tile
//           buffers alternate, so one barrier per transposing member suffices (a wave can only reach the write of its next-but-one
//           transposing member after every wave has finished reading this one's tile).
//   LDS tile: swizzle_tile.h, the layout and the access pattern of collate.hip's transposed tiles (column writes by 32-lane halves
//           that hold 4 tile columns x 8 row blocks; row reads of 16 bytes per lane).  Derived bank-conflict count, as derived in
//           collate.hip's header: 0 for the ds_write_b32 (the XOR with the row block spreads a half over 32 distinct banks;
//           unswizzled it would be 8-way), 0 for the ds_read_b128 (each 16-lane group reads 16 distinct 16-byte slots).
// Per-element path (W % 4 != 0 or unaligned pointers): one output element per thread and member through the index map above.
//
// Resources (gfx950, -Rpass-analysis=kernel-resource-usage):
//   expand_vec_kernel<true>  33 VGPRs, 4 KiB LDS (one tile)    <false>  20 VGPRs, no LDS    expand_elem_kernel  17 VGPRs, no LDS
//   mean_vec_kernel<true>    27 VGPRs, 8 KiB LDS (two tiles)   <false>  18 VGPRs, no LDS    mean_elem_kernel    20 VGPRs, no LDS
// No instance uses scratch (0 bytes / lane, no spills).  swizzle_tile.h was lifted out of collate.hip; its four kernels compile to
// the resource usage stated in its header, unchanged.
#include "../../../include/hrnet_hip.h"
#include "common.h"
#include "swizzle_tile.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxK = 8;
constexpr int kMaxSide = 1 << 15;                        // keeps H * W and every tile count inside int32
constexpr size_t kMaxTiles = ((size_t)1 << 24) - 1;      // vector path: blocks per launch; x 256 threads stays below 2^32, HIP's limit

__device__ __forceinline__ int code_at(unsigned codes, int k) { return (int)(codes >> (4 * k)) & 7; }
__device__ __forceinline__ f32x4 rev4_if(f32x4 v, bool reversed) { return reversed ? f32x4{v[3], v[2], v[1], v[0]} : v; }

// block -> (plane n, tile corner (r0, c0), tile extent (h, w)); tw tiles per row of tiles, tpp tiles per plane
struct TileOf {
    int n, r0, c0, h, w;
    __device__ __forceinline__ TileOf(int H, int W, int tw, int tpp) {
        n = (int)(blockIdx.x / (unsigned)tpp);
        const int t = (int)(blockIdx.x - (unsigned)n * (unsigned)tpp);
        r0 = (t / tw) * kTile;
        c0 = (t - (t / tw) * tw) * kTile;
        h = min(kTile, H - r0);
        w = min(kTile, W - c0);
    }
};

// ANY_T = false: no member transposes; the LDS tile, its barrier and the H == W assumption fold away.
template <bool ANY_T>
__global__ __launch_bounds__(kThreads) void expand_vec_kernel(const float* __restrict__ x, int H, int W, int tw, int tpp, unsigned codes, int K,
                                                              size_t member_elems, float* __restrict__ out) {
    const TileOf T(H, W, tw, tpp);
    const int lr = threadIdx.x >> 3, lq = (threadIdx.x & 7) << 2;
    const size_t plane = (size_t)T.n * H * W;
    const bool own = lr < T.h && lq < T.w;               // source element (r0 + lr, c0 + lq ..) exists
    const bool own_t = lr < T.w && lq < T.h;             // transposed copy: row lr <-> source column, columns lq .. <-> source rows
    f32x4 v = {0.f, 0.f, 0.f, 0.f}, tv = v;
    if (own) v = *(const f32x4*)(x + plane + (size_t)(T.r0 + lr) * W + T.c0 + lq);
    if constexpr (ANY_T) {
        __shared__ __attribute__((aligned(16))) float tile[kTile * kTile];
        if (own) {
#pragma unroll
            for (int m = 0; m < 4; ++m) tile[tile_at(lq + m, lr)] = v[m];
        }
        __syncthreads();
        if (own_t) tv = *(const f32x4*)(tile + tile_at(lr, lq));      // tv[m] = x[r0 + lq + m][c0 + lr]
    }
    for (int k = 0; k < K; ++k) {
        const int c = code_at(codes, k);
        const bool flip_i = c & 2, flip_j = c & 1;
        float* o = out + (size_t)k * member_elems + plane;
        if (ANY_T && (c & 4)) {                          // out[i][j] = x[j'][i']: source (r, c) lands at i = flip(c), j = flip(r); H == W
            if (own_t) {
                const int sc = T.c0 + lr, sr = T.r0 + lq;
                const int i = flip_i ? W - 1 - sc : sc, j = flip_j ? H - 4 - sr : sr;
                *(f32x4*)(o + (size_t)i * W + j) = rev4_if(tv, flip_j);
            }
        } else if (own) {                                // out[i][j] = x[i'][j']
            const int sr = T.r0 + lr, sc = T.c0 + lq;
            const int i = flip_i ? H - 1 - sr : sr, j = flip_j ? W - 4 - sc : sc;
            *(f32x4*)(o + (size_t)i * W + j) = rev4_if(v, flip_j);
        }
    }
}

// `inv`: the INVERSE codes of the members, in list order
template <bool ANY_T>
__global__ __launch_bounds__(kThreads) void mean_vec_kernel(const float* __restrict__ y, int H, int W, int tw, int tpp, unsigned inv, int K,
                                                            size_t member_elems, float r, float* __restrict__ out) {
    const TileOf T(H, W, tw, tpp);
    const int lr = threadIdx.x >> 3, lq = (threadIdx.x & 7) << 2;
    const size_t plane = (size_t)T.n * H * W;
    const bool own = lr < T.h && lq < T.w;               // output element (r0 + lr, c0 + lq ..) exists
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    int buf = 0;
    for (int k = 0; k < K; ++k) {
        const int c = code_at(inv, k);
        const bool flip_i = c & 2, flip_j = c & 1;
        const float* src = y + (size_t)k * member_elems + plane;
        f32x4 m = {0.f, 0.f, 0.f, 0.f};
        if (ANY_T && (c & 4)) {                          // m[i][j] = y[j'][i'], H == W
            if constexpr (ANY_T) {
                __shared__ __attribute__((aligned(16))) float lds[2 * kTile * kTile];
                float* tile = lds + buf * (kTile * kTile);
                buf ^= 1;
                if (lr < T.w && lq < T.h) {              // source row <-> output column j, 4 source columns <-> output rows i .. i+3
                    const int j = T.c0 + lr, i = T.r0 + lq;
                    const int sr = flip_j ? W - 1 - j : j, sc = flip_i ? H - 4 - i : i;
                    const f32x4 v = rev4_if(*(const f32x4*)(src + (size_t)sr * W + sc), flip_i);
#pragma unroll
                    for (int q = 0; q < 4; ++q) tile[tile_at(lq + q, lr)] = v[q];
                }
                __syncthreads();
                if (own) m = *(const f32x4*)(tile + tile_at(lr, lq));
            }
        } else if (own) {                                // m[i][j] = y[i'][j']
            const int i = T.r0 + lr, j = T.c0 + lq;
            const int sr = flip_i ? H - 1 - i : i, sc = flip_j ? W - 4 - j : j;
            m = rev4_if(*(const f32x4*)(src + (size_t)sr * W + sc), flip_j);
        }
        acc = k == 0 ? m : acc + m;                      // list order, whatever path the member took
    }
    if (own) *(f32x4*)(out + plane + (size_t)(T.r0 + lr) * W + T.c0 + lq) = acc * r;
}

// element e of a (.., H, W) stack -> its plane's first element and the source position inside the plane under code c
__device__ __forceinline__ size_t source_of(size_t e, int H, int W, int c, size_t& plane0) {
    const size_t hw = (size_t)H * W, p = e / hw;
    const int rem = (int)(e - p * hw), i = rem / W, j = rem - i * W;
    const int ip = c & 2 ? H - 1 - i : i, jp = c & 1 ? W - 1 - j : j;
    plane0 = p * hw;
    return c & 4 ? (size_t)jp * W + ip : (size_t)ip * W + jp;      // a transposing code comes with H == W
}

__global__ __launch_bounds__(kThreads) void expand_elem_kernel(const float* __restrict__ x, int H, int W, size_t member_elems, unsigned codes,
                                                               float* __restrict__ out) {
    const int k = blockIdx.y, c = code_at(codes, k);
    for (size_t e = (size_t)blockIdx.x * kThreads + threadIdx.x; e < member_elems; e += (size_t)gridDim.x * kThreads) {
        size_t plane0;
        const size_t s = source_of(e, H, W, c, plane0);
        out[(size_t)k * member_elems + e] = x[plane0 + s];
    }
}

__global__ __launch_bounds__(kThreads) void mean_elem_kernel(const float* __restrict__ y, int H, int W, size_t member_elems, unsigned inv, int K,
                                                             float r, float* __restrict__ out) {
    for (size_t e = (size_t)blockIdx.x * kThreads + threadIdx.x; e < member_elems; e += (size_t)gridDim.x * kThreads) {
        float acc = 0.f;
        for (int k = 0; k < K; ++k) {
            size_t plane0;
            const size_t s = source_of(e, H, W, code_at(inv, k), plane0);
            const float m = y[(size_t)k * member_elems + plane0 + s];
            acc = k == 0 ? m : acc + m;
        }
        out[e] = acc * r;
    }
}

int inverse_code(int c) { return c == 5 ? 6 : c == 6 ? 5 : c; }

// Everything that can be refused, before any launch.  -> packed codes (inverted for the mean), whether any member transposes.
int check_args(const char* fn, const void* in, const void* out, int N, int H, int W, const int32_t* codes, int K, bool invert,
               unsigned* packed, bool* any_t) {
    HRN_CHECK(in && out && codes, -2, "%s: null argument", fn);
    HRN_CHECK(K >= 1 && K <= kMaxK, -2, "%s: K must be in 1..8 (got %d)", fn, K);
    HRN_CHECK(N > 0 && H > 0 && W > 0 && H <= kMaxSide && W <= kMaxSide, -2, "%s: bad shape N=%d H=%d W=%d (sides up to %d)", fn, N, H, W,
              kMaxSide);
    unsigned seen = 0;
    *packed = 0;
    *any_t = false;
    for (int k = 0; k < K; ++k) {
        const int c = codes[k];
        HRN_CHECK(c >= 0 && c <= 7, -2, "%s: bad code %d at position %d (codes are 0..7)", fn, c, k);
        HRN_CHECK(!(seen >> c & 1u), -2, "%s: duplicate code %d at position %d", fn, c, k);
        HRN_CHECK(!(c & 4) || H == W, -2, "%s: code %d transposes, which needs a square plane (H=%d != W=%d)", fn, c, H, W);
        seen |= 1u << c;
        *any_t |= (c & 4) != 0;
        *packed |= (unsigned)(invert ? inverse_code(c) : c) << (4 * k);
    }
    return 0;
}

struct Geometry {
    bool vec;
    int tw, tpp;
    size_t member_elems;
    unsigned blocks;                                     // grid.x of the path taken
};

int geometry(const char* fn, const void* a, const void* b, int N, int H, int W, Geometry* g) {
    g->member_elems = (size_t)N * H * W;
    g->vec = W % 4 == 0 && ((uintptr_t)a | (uintptr_t)b) % 16 == 0;
    g->tw = (W + kTile - 1) / kTile;
    g->tpp = g->tw * ((H + kTile - 1) / kTile);
    if (g->vec) {
        const size_t tiles = (size_t)N * g->tpp;
        // a launch takes fewer than 2^32 threads = 2^24 blocks of 256: refused here, not left to fail at the launch
        HRN_CHECK(tiles <= kMaxTiles, -2, "%s: N=%d planes of %d x %d are more than %zu tiles of %d x %d, the grid limit", fn, N, H, W,
                  kMaxTiles, kTile, kTile);
        g->blocks = (unsigned)tiles;
    } else {
        const size_t want = (g->member_elems + kThreads - 1) / kThreads;
        g->blocks = (unsigned)(want < (1u << 20) ? want : (1u << 20));          // grid-stride beyond 2^28 elements
    }
    return 0;
}

}  // namespace

extern "C" int hrn_dihedral_expand(const float* x, int N, int H, int W, const int32_t* codes, int K, float* out, void* stream) {
    unsigned packed;
    bool any_t;
    Geometry g;
    if (int rc = check_args("hrn_dihedral_expand", x, out, N, H, W, codes, K, false, &packed, &any_t)) return rc;
    if (int rc = geometry("hrn_dihedral_expand", x, out, N, H, W, &g)) return rc;
    if (g.vec)
        hipLaunchKernelGGL(any_t ? expand_vec_kernel<true> : expand_vec_kernel<false>, dim3(g.blocks), dim3(kThreads), 0, (hipStream_t)stream, x,
                           H, W, g.tw, g.tpp, packed, K, g.member_elems, out);
    else
        hipLaunchKernelGGL(expand_elem_kernel, dim3(g.blocks, (unsigned)K), dim3(kThreads), 0, (hipStream_t)stream, x, H, W, g.member_elems,
                           packed, out);
    HRN_LAUNCH_CHECK();
    return 0;
}

extern "C" int hrn_dihedral_mean(const float* y, int N, int H, int W, const int32_t* codes, int K, float* out, void* stream) {
    unsigned inv;
    bool any_t;
    Geometry g;
    if (int rc = check_args("hrn_dihedral_mean", y, out, N, H, W, codes, K, true, &inv, &any_t)) return rc;
    if (int rc = geometry("hrn_dihedral_mean", y, out, N, H, W, &g)) return rc;
    const float r = (float)(1.0 / K);
    if (g.vec)
        hipLaunchKernelGGL(any_t ? mean_vec_kernel<true> : mean_vec_kernel<false>, dim3(g.blocks), dim3(kThreads), 0, (hipStream_t)stream, y, H,
                           W, g.tw, g.tpp, inv, K, g.member_elems, r, out);
    else
        hipLaunchKernelGGL(mean_elem_kernel, dim3(g.blocks), dim3(kThreads), 0, (hipStream_t)stream, y, H, W, g.member_elems, inv, K, r, out);
    HRN_LAUNCH_CHECK();
    return 0;
}
