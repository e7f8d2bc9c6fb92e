// A shift per block of tiles of every view - a shift FIELD for scenes - and the views resampled by it, on the
// tiles, the window and the sums of registration_scene.hip (section 7g).
//
// An axis of length L has n = max(1, (L + block / 2) / block) blocks of `block` pixels, a multiple of 64; the last block runs to L, so a
// remainder below half a block joins its neighbour and every block is a union of whole 64-pixel tiles.  The score of a block at a shift
// is section 7f's score with the reference mask set to zero outside the block: the level kernel is scene_level_kernel's function
// (mncc_scene.h: scene_level) with the centre of the grid read per (view, block of this tile), and the finishing kernel calls
// scene_finish_kernel's (finish_tiles) on the block's rectangle of tiles instead of all tiles of a view.  Both images stay centred
// on their WHOLE-FRAME means.  A search is 1 + 2 levels launches; `init` and every centre are read from device memory, and nothing returns to the host.  No atomics: bit-reproducible.
//
// The field at a pixel is bilinear between the blocks' centres (the nodes) and constant beyond the outer ones, in fp64 in a fixed
// order, rounded to fp32.  The resampler splits every pixel's own shift into whole pixels, fraction and taps and reads the pixel's 6 x 6
// neighbourhood through the caches: the same fp32 operations in the same order as scene_apply_kernel's two passes, so a constant field
// gives hrn_mncc_apply_scene's bits.  A pixel whose footprint leaves the frame reads nothing.
#include "mncc_scene.h"

namespace {

// the block of an axis that holds tile `t` of it: bt tiles a block, the last block takes the rest
__device__ __forceinline__ unsigned block_of_tile(unsigned t, unsigned bt, unsigned n) {
    const unsigned b = t / bt;
    return b < n - 1 ? b : n - 1;
}

// ----------------------------------------------------------------------------- one grid level: the tiles' sums
// scene_level_kernel around centres[view * nby * nbx + the block of this tile] (per_block) or centres[view] (the first level, which
// starts every block of a view from `init`); (0, 0) where `centres` is null.  grid (B V tiles)
__global__ __launch_bounds__(SC_THREADS) void local_level_kernel(const float* __restrict__ ref, const float* __restrict__ ref_mask,
                                                                 const float* __restrict__ views, const float* __restrict__ view_masks,
                                                                 const float* __restrict__ centres, const double* __restrict__ means,
                                                                 unsigned chunks, unsigned BV, int V, int H, int W, int P, double width,
                                                                 unsigned tiles_x, unsigned tiles, double* __restrict__ sums, int per_block,
                                                                 unsigned bt, unsigned nby, unsigned nbx) {
    scene_level(ref, ref_mask, views, view_masks, centres, means, chunks, BV, V, H, W, P, width, tiles_x, tiles, sums,
                [=](size_t view, unsigned tile) {
                    return per_block ? view * nby * nbx + block_of_tile(tile / tiles_x, bt, nby) * nbx + block_of_tile(tile % tiles_x, bt, nbx)
                                     : view;
                });
}

// ----------------------------------------------------------------------------- one grid level: the finish
// Per (view, block): the sums of the block's tiles added in tile-index order, the P^2 scores, the first maximum: centres_out[view, block]
// = the best point and trace_k[(view, block) * trace_stride] = (dy, dx, score).  centres_in is read per block (per_block) or per view, and
// is (0, 0) when null; centres_out may be centres_in.  After the last level (`field` not null): n is the count of common valid pixels
// at the chosen point, the block is ok when the score is finite and n >= min_valid * the block's area (fp64), field[view, block] = the
// best point when ok and init[view] ((0, 0) when null) otherwise, ok[view, block] = 1 / 0 (may be null).  grid (B V nby nbx),
// SC_FINISH_THREADS threads
__global__ __launch_bounds__(SC_FINISH_THREADS) void local_finish_kernel(const double* __restrict__ sums, const float* centres_in,
                                                                         int per_block, const float* __restrict__ init, int P, double width,
                                                                         unsigned tiles_x, unsigned tiles_y, unsigned bt, unsigned nby,
                                                                         unsigned nbx, int H, int W, int block, float* centres_out,
                                                                         float* __restrict__ trace_k, int trace_stride,
                                                                         float* __restrict__ field, float* __restrict__ ok, double min_valid) {
    __shared__ FinishShared F;
    const int tid = threadIdx.x, pp = P * P;
    const unsigned blocks = nby * nbx;
    const size_t vb = blockIdx.x, view = vb / blocks;
    const unsigned blk = (unsigned)(vb - view * blocks), by = blk / nbx, bx = blk - by * nbx;
    const size_t c = per_block ? vb : view;
    float cy = centres_in ? centres_in[2 * c] : 0.f, cx = centres_in ? centres_in[2 * c + 1] : 0.f;
    const unsigned ty1 = by == nby - 1 ? tiles_y : (by + 1) * bt, tx1 = bx == nbx - 1 ? tiles_x : (bx + 1) * bt;
    const float best = finish_tiles(F, sums + view * tiles_y * tiles_x * pp * RG_NSUM, tiles_x, by * bt, ty1, bx * bt, tx1, P, width, cy, cx,
                                    true, centres_out + 2 * vb, trace_k ? trace_k + vb * trace_stride : nullptr, tid);
    if (tid == 0 && field) {
        bool good = false;
        if (best > -INFINITY) {
            int at = 0;
            while (at < pp - 1 && !(F.score[at] == best)) ++at;             // the first maximum is the first point with its score
            const int r0 = (int)by * block, r1 = by == nby - 1 ? H : r0 + block, c0 = (int)bx * block, c1 = bx == nbx - 1 ? W : c0 + block;
            good = F.count[at] >= min_valid * ((double)(r1 - r0) * (double)(c1 - c0));
        }
        field[2 * vb] = good ? cy : (init ? init[2 * view] : 0.f);
        field[2 * vb + 1] = good ? cx : (init ? init[2 * view + 1] : 0.f);
        if (ok) ok[vb] = good ? 1.f : 0.f;
    }
}

// ----------------------------------------------------------------------------- the field at a pixel
// Pixel p of an axis of length L in n blocks: k = the last node at or before p, within [0, n - 2], and t = (p - node_k) / (node_{k+1} -
// node_k) within [0, 1]; the node of block i is the centre (r0 + r1 - 1) / 2 of its pixels.  One block: k = 0, t = 0.
__device__ __forceinline__ void field_axis(int p, int L, int block, int n, int* k, double* t) {
    *k = 0;
    *t = 0.0;
    if (n < 2) return;
    const int twice = 2 * p - (block - 1);                             // 2 (p - node_0)
    int kk = twice < 0 ? 0 : twice / (2 * block);
    kk = kk < n - 2 ? kk : n - 2;
    const double a = (double)(kk * block) + (double)(block - 1) / 2.0;
    const int r0 = (kk + 1) * block, r1 = kk + 1 == n - 1 ? L : r0 + block;
    const double b = (double)(r0 + r1 - 1) / 2.0;
    const double v = ((double)p - a) / (b - a);
    *k = kk;
    *t = v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v);
}

// ----------------------------------------------------------------------------- the resampler by a field
// out = S(view, the field at the pixel), out_valid = V(mask, the same) pixel by pixel; field (B V, nby, nbx, 2).  A thread takes
// scene_apply_kernel's pixels: column `lane` of its tile, two runs of RG_RUN rows.  grid (B V tiles)
__global__ __launch_bounds__(SC_THREADS) void field_apply_kernel(const float* __restrict__ views, const float* __restrict__ view_masks,
                                                                 const float* __restrict__ field, int H, int W, int block, int nby, int nbx,
                                                                 unsigned tiles_x, unsigned tiles, float* __restrict__ out,
                                                                 float* __restrict__ out_valid) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t view = blockIdx.x / tiles, hw = (size_t)H * W;
    const unsigned tile = blockIdx.x - (unsigned)view * tiles;
    const int ty0 = (int)(tile / tiles_x) * SC_TILE, tx0 = (int)(tile % tiles_x) * SC_TILE;
    const int gx = tx0 + lane;
    if (gx >= W) return;                                               // no barrier below
    const float* img = views + view * hw;
    const float* msk = view_masks ? view_masks + view * hw : nullptr;
    const float* nodes = field + view * (size_t)(nby * nbx) * 2;
    int kx;
    double tx;
    field_axis(gx, W, block, nbx, &kx, &tx);
    const int kx1 = nbx > 1 ? kx + 1 : kx;
#pragma unroll 1
    for (int k = 0; k < SC_ITEMS; ++k) {
#pragma unroll 1
        for (int p = 0; p < RG_RUN; ++p) {
            const int gy = ty0 + (wave + k * SC_WAVES) * RG_RUN + p;
            if (gy >= H) break;
            int ky;
            double ty;
            field_axis(gy, H, block, nby, &ky, &ty);
            const int ky1 = nby > 1 ? ky + 1 : ky;
            float d[2];
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const double n00 = (double)nodes[(ky * nbx + kx) * 2 + c], n01 = (double)nodes[(ky * nbx + kx1) * 2 + c];
                const double n10 = (double)nodes[(ky1 * nbx + kx) * 2 + c], n11 = (double)nodes[(ky1 * nbx + kx1) * 2 + c];
                d[c] = (float)((1.0 - ty) * ((1.0 - tx) * n00 + tx * n01) + ty * ((1.0 - tx) * n10 + tx * n11));
            }
            int ny, nx;
            double fy, fx;
            float tapy[6], tapx[6];
            split_and_taps(d[0], &ny, &fy, tapy);
            split_and_taps(d[1], &nx, &fx, tapx);
            float value = 0.f;
            bool on = gx + nx - 2 >= 0 && gx + nx + 3 <= W - 1 && gy + ny - 2 >= 0 && gy + ny + 3 <= H - 1;
            if (on) {                                                  // every address below lies inside the frame
                const size_t at = (size_t)(gy + ny) * W + (size_t)(gx + nx);
                double q0 = 1.0, q1 = 1.0, q2 = 1.0, q3 = 1.0;
                if (msk) {
                    q0 = msk[at] != 0.f; q1 = msk[at + 1] != 0.f; q2 = msk[at + W] != 0.f; q3 = msk[at + W + 1] != 0.f;
                }
                on = mask_sample(fy, fx, q0, q1, q2, q3);
            }
            if (on) {
                float a[6];
#pragma unroll
                for (int m = 0; m < 6; ++m) {                          // scene_row_pass on the six rows of the footprint
                    const float* row = img + (size_t)(gy + ny - 2 + m) * W + (size_t)(gx + nx - 2);
                    float s = tapx[0] * row[0];
#pragma unroll
                    for (int o = 1; o < 6; ++o) s = fmaf(tapx[o], row[o], s);
                    a[m] = s;
                }
                value = tapy[0] * a[0];                                // scene_column_run
#pragma unroll
                for (int o = 1; o < 6; ++o) value = fmaf(tapy[o], a[o], value);
            }
            const size_t i = view * hw + (size_t)gy * W + gx;
            out[i] = on ? value : 0.f;
            out_valid[i] = on ? 1.f : 0.f;
        }
    }
}

// the scene search's plan, with the blocks of the two axes and a centre per block
struct LocalPlan : ScenePlan {
    unsigned bt, nby, nbx;
};

LocalPlan plan(int B, int V, int H, int W, int P, int block) {
    LocalPlan p{plan(B, V, H, W, P)};
    p.bt = (unsigned)(block / SC_TILE);
    p.nby = (unsigned)hrn_mncc_local_blocks_impl(H, block);
    p.nbx = (unsigned)hrn_mncc_local_blocks_impl(W, block);
    p.centres_bytes *= (size_t)p.nby * p.nbx;
    return p;
}

}  // namespace

int hrn_mncc_local_blocks_impl(int L, int block) {
    const int n = (L + block / 2) / block;
    return n > 1 ? n : 1;
}

size_t hrn_mncc_local_workspace_bytes_impl(int B, int V, int H, int W, int P, int block) {
    return plan(B, V, H, W, P, block).bytes();
}

// B V tiles is the grid of the level and of the resampler, B V blocks that of the finish
bool hrn_mncc_local_grid_fits(int B, int V, int H, int W, int block) {
    const LocalPlan p = plan(B, V, H, W, HRN_MNCC_MIN_POINTS, block);
    return hrn_mncc_scene_grid_fits(B, V, H, W) && (double)B * V * p.nby * p.nbx <= 2147483647.0;
}

int hrn_launch_mncc_search_local(const float* ref, const float* ref_mask, const float* views, const float* view_masks, const float* init,
                                 int B, int V, int H, int W, int P, int levels, float radius, int block, float min_valid, float* field,
                                 float* trace, float* ok, void* workspace, hipStream_t stream) {
    const LocalPlan p = plan(B, V, H, W, P, block);
    const SceneWorkspace w = carve(workspace, p);
    const unsigned bv = (unsigned)(B * V);
    HrnProfScope prof("mncc_search_local", level_flops(P) * levels * B * V * H * W, 4.0 * B * V * (2.0 + 2.0 * levels) * H * W, stream);
    hrn_launch_mncc_scene_means(ref, ref_mask, views, view_masks, B, V, H, W, w.means, stream);
    HRN_LAUNCH_CHECK();
    double width = (double)(2.f * radius);
    const double ratio = level_ratio(P);
    for (int k = 0; k < levels; ++k) {
        const float* from = k ? w.centres : init;                        // the first centre of every block of a view is init[view]
        const bool last = k == levels - 1;
        hipLaunchKernelGGL(local_level_kernel, dim3(bv * p.tiles), dim3(SC_THREADS), 0, stream, ref, ref_mask, views, view_masks, from,
                           (const double*)w.means, p.chunks, bv, V, H, W, P, width, p.tiles_x, p.tiles, w.sums, k ? 1 : 0, p.bt, p.nby, p.nbx);
        HRN_LAUNCH_CHECK();
        hipLaunchKernelGGL(local_finish_kernel, dim3(bv * p.nby * p.nbx), dim3(SC_FINISH_THREADS), 0, stream, (const double*)w.sums, from,
                           k ? 1 : 0, init, P, width, p.tiles_x, p.tiles_y, p.bt, p.nby, p.nbx, H, W, block, w.centres,
                           trace ? trace + 3 * k : (float*)nullptr, 3 * levels, last ? field : (float*)nullptr, last ? ok : (float*)nullptr,
                           (double)min_valid);
        HRN_LAUNCH_CHECK();
        width = width * ratio;
    }
    return 0;
}

int hrn_launch_mncc_apply_field(const float* views, const float* view_masks, const float* field, int B, int V, int H, int W, int block,
                                float* out, float* out_valid, hipStream_t stream) {
    const LocalPlan p = plan(B, V, H, W, HRN_MNCC_MIN_POINTS, block);
    HrnProfScope prof("mncc_apply_field", 2.0 * 42.0 * B * V * H * W, 4.0 * B * V * (4.0 * H * W + 2.0 * p.nby * p.nbx), stream);
    hipLaunchKernelGGL(field_apply_kernel, dim3((unsigned)(B * V) * p.tiles), dim3(SC_THREADS), 0, stream, views, view_masks, field, H, W, block,
                       (int)p.nby, (int)p.nbx, p.tiles_x, p.tiles, out, out_valid);
    HRN_LAUNCH_CHECK();
    return 0;
}
