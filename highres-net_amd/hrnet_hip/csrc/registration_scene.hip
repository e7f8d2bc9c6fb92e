// The masked-NCC registration search and resampling for frames of any size: the definitions of
// include/hrnet_hip.h and the arithmetic of registration.hip, with a frame cut into tiles instead of held in one CU's LDS.
//
// A workgroup owns a core tile of SC_TILE x SC_TILE pixels of the reference for one view.  Per level it stages a window of the view from
// HBM into LDS: the core plus a halo for the span of whole-pixel offsets the level's P coordinates reach (at most SC_SPAN, see below)
// plus the six-tap footprint.  The window's origin is the tile's origin plus the smallest whole-pixel offset of the level minus 2, so a
// centre far from (0, 0) costs no LDS.  Then the structure of registration.hip: the pass along rows once per dx into the LDS buffer A
// (window rows x core columns), the pass along columns per dy out of registers, a lane per column.  Nothing is clamped at a window
// edge: every address the two passes form lies inside the window by construction, and whether a footprint is valid is tested against
// the FRAME.  Window pixels outside the frame are staged as zeros with a set mask; no valid pixel reads them.
//
// A score's sums are taken on images centred by WHOLE-FRAME means (a pre-pass: fixed-order fp64 sums per chunk, the chunks added in
// order, the quotient rounded to fp32), never per tile.  A thread adds its 16 pixels in fp64 - a tile need not have the frame's mean
// ("Sums") - and the wave (WaveSums), the waves in order and - in the finishing kernel of a level - the tiles in
// index order are added in fp64 too.  A workgroup writes its 6 P^2 sums to the
// workspace; there is no atomic anywhere.  The finishing kernel forms the scores, takes the first maximum and writes the next centre to
// device memory, where the next level's launch reads it: nothing returns to the host between levels.  hrn_mncc_grid_scene and a level of
// hrn_mncc_search_scene are the same two kernels on the same partition, so their scores agree bit for bit.
//
// The span: a level's coordinates are d_0 <= ... <= d_{P-1} with d_{P-1} - d_0 <= 8 before the rounding to fp32 (width <= 8), so
// floor(d_{P-1}) - floor(d_0) <= 9.  A coordinate further than SC_SPAN whole pixels from the smallest cannot occur; the kernels skip it
// (its score would be -inf) rather than read outside the window.
#include "mncc_scene.h"

namespace {

// ----------------------------------------------------------------------------- the means
// partial[(plane * chunks + chunk) * 2] = {sum, count} of the clear pixels of one chunk of one plane; planes 0 .. BV - 1 are the views,
// BV .. BV + B - 1 the references.  grid (planes * chunks)
__global__ __launch_bounds__(SC_THREADS) void scene_mean_kernel(const float* __restrict__ ref, const float* __restrict__ ref_mask,
                                                                const float* __restrict__ views, const float* __restrict__ view_masks,
                                                                unsigned BV, size_t hw, unsigned chunks, double* __restrict__ partial) {
    __shared__ double red[SC_WAVES][2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned plane = blockIdx.x / chunks, chunk = blockIdx.x - plane * chunks;
    const bool is_ref = plane >= BV;
    const size_t base = (size_t)(is_ref ? plane - BV : plane) * hw;
    const float* img = (is_ref ? ref : views) + base;
    const float* msk = is_ref ? ref_mask : view_masks;
    if (msk) msk += base;
    const size_t len = (hw + chunks - 1) / chunks, lo = (size_t)chunk * len, hi = lo + len < hw ? lo + len : hw;
    double v[2] = {0.0, 0.0};
    for (size_t i = lo + tid; i < hi; i += SC_THREADS)
        if (msk ? msk[i] != 0.f : true) { v[0] += (double)img[i]; v[1] += 1.0; }
    WaveSums<2, 0>::run(v, lane);
    if (lane < 2) red[wave][wave_sums_index<2>(lane)] = v[0];
    __syncthreads();
    if (tid < 2) {
        double s = 0.0;
        for (int w = 0; w < SC_WAVES; ++w) s += red[w][tid];
        partial[((size_t)plane * chunks + chunk) * 2 + tid] = s;
    }
}

// ----------------------------------------------------------------------------- one grid level: the tiles' sums
// sums[((view * tiles + tile) * P^2 + i P + j) * 6 + q]: the six sums of tile `tile` of view `view` at (dy_i, dx_j) of the P x P grid
// of `width` around centres[view] ((0, 0) where `centres` is null).  grid (B V tiles), tiles = tiles_x * tiles_y
__global__ __launch_bounds__(SC_THREADS) void scene_level_kernel(const float* __restrict__ ref, const float* __restrict__ ref_mask,
                                                                 const float* __restrict__ views, const float* __restrict__ view_masks,
                                                                 const float* __restrict__ centres, const double* __restrict__ means,
                                                                 unsigned chunks, unsigned BV, int V, int H, int W, int P, double width,
                                                                 unsigned tiles_x, unsigned tiles, double* __restrict__ sums) {
    scene_level(ref, ref_mask, views, view_masks, centres, means, chunks, BV, V, H, W, P, width, tiles_x, tiles, sums,
                [](size_t view, unsigned) { return view; });
}

// ----------------------------------------------------------------------------- one grid level: the finish
// Per view: the tiles' sums added in index order, the P^2 scores, and - for the search - the first maximum: centres_out[view] = the
// best point, trace_k[view * trace_stride] = (dy, dx, score), shifts[view] = the best point (each may be null).  centres_in null: (0, 0).
// centres_out may be centres_in.  grid (B V), SC_FINISH_THREADS threads
__global__ __launch_bounds__(SC_FINISH_THREADS) void scene_finish_kernel(const double* __restrict__ sums, const float* centres_in, int P,
                                                                         double width, unsigned tiles, float* __restrict__ scores,
                                                                         float* centres_out, float* __restrict__ trace_k,
                                                                         int trace_stride, float* __restrict__ shifts) {
    __shared__ FinishShared F;
    const int tid = threadIdx.x, pp = P * P;
    const size_t view = blockIdx.x;
    float cy = centres_in ? centres_in[2 * view] : 0.f, cx = centres_in ? centres_in[2 * view + 1] : 0.f;
    // all tiles of the view as one row: the row-major order of the rectangle is the tiles' index order
    finish_tiles(F, sums + view * tiles * pp * RG_NSUM, tiles, 0, 1, 0, tiles, P, width, cy, cx, centres_out || trace_k || shifts,
                 centres_out ? centres_out + 2 * view : nullptr, trace_k ? trace_k + view * trace_stride : nullptr, tid);
    if (scores && tid < pp) scores[view * pp + tid] = F.score[tid];
    if (tid == 0 && shifts) { shifts[2 * view] = cy; shifts[2 * view + 1] = cx; }
}

// ----------------------------------------------------------------------------- the resampler
// out = S(view, shift), out_valid = V(mask, shift), tile by tile: the window is the core plus the footprint at the one offset.  The
// operations on a pixel and their order are mncc_apply_kernel's, so the two agree bit for bit.  grid (B V tiles)
__global__ __launch_bounds__(SC_THREADS) void scene_apply_kernel(const float* __restrict__ views, const float* __restrict__ view_masks,
                                                                 const float* __restrict__ shifts, int H, int W, unsigned tiles_x,
                                                                 unsigned tiles, float* __restrict__ out, float* __restrict__ out_valid) {
    __shared__ SceneShared S;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t view = blockIdx.x / tiles, hw = (size_t)H * W;
    const unsigned tile = blockIdx.x - (unsigned)view * tiles;
    const int ty0 = (int)(tile / tiles_x) * SC_TILE, tx0 = (int)(tile % tiles_x) * SC_TILE;
    if (tid < 2) split_and_taps(shifts[2 * view + tid], &S.whole[tid][0], &S.frac[tid][0], S.tap[tid][0]);
    __syncthreads();
    if (tid == 0) S.table[0] = mask_table(S.frac[0][0], S.frac[1][0]);
    const int ny = S.whole[0][0], nx = S.whole[1][0];
    constexpr int ROWS = SC_TILE + 5;
    stage_window<ROWS, ROWS>(views + view * hw, view_masks ? view_masks + view * hw : nullptr, S, ty0 + ny - 2, tx0 + nx - 2, H, W, 0.f, tid);
    scene_row_pass(S, S.tap[1][0], 0, ROWS, tid);
    __syncthreads();
    const unsigned table = S.table[0];
    float ky[6];
#pragma unroll
    for (int o = 0; o < 6; ++o) ky[o] = S.tap[0][0][o];
    const int x = lane, gx = tx0 + x;
#pragma unroll
    for (int k = 0; k < SC_ITEMS; ++k) {
        const int yl = (wave + k * SC_WAVES) * RG_RUN, gy = ty0 + yl;
        float t[RG_RUN];
        const unsigned c = scene_column_run(S, ky, ny, nx, 0, 0, table, x, yl, gy, gx, H, W, t);
        if (gx >= W) continue;
#pragma unroll
        for (int p = 0; p < RG_RUN; ++p) {
            if (gy + p >= H) break;
            const bool on = (c >> p) & 1u;
            const size_t i = view * hw + (size_t)(gy + p) * W + gx;
            out[i] = on ? t[p] : 0.f;
            out_valid[i] = on ? 1.f : 0.f;
        }
    }
}

void launch_means(const float* ref, const float* ref_mask, const float* views, const float* view_masks, int B, int V, int H, int W,
                  const ScenePlan& p, double* means, hipStream_t stream) {
    const unsigned bv = (unsigned)(B * V);
    hipLaunchKernelGGL(scene_mean_kernel, dim3((bv + (unsigned)B) * p.chunks), dim3(SC_THREADS), 0, stream, ref, ref_mask, views, view_masks,
                       bv, (size_t)H * W, p.chunks, means);
}

}  // namespace

// the means pre-pass for registration_local.hip, whose workspace begins as this file's does
void hrn_launch_mncc_scene_means(const float* ref, const float* ref_mask, const float* views, const float* view_masks, int B, int V, int H,
                                 int W, double* means, hipStream_t stream) {
    launch_means(ref, ref_mask, views, view_masks, B, V, H, W, plan(B, V, H, W, HRN_MNCC_MIN_POINTS), means, stream);
}

size_t hrn_mncc_scene_workspace_bytes_impl(int B, int V, int H, int W, int P) {
    return plan(B, V, H, W, P).bytes();
}

// B V tiles is the grid of the level and of the resampler
bool hrn_mncc_scene_grid_fits(int B, int V, int H, int W) {
    const ScenePlan p = plan(B, V, H, W, HRN_MNCC_MIN_POINTS);
    return (double)B * V * p.tiles <= 2147483647.0 && (double)(B * (double)V + B) * p.chunks <= 2147483647.0;
}

int hrn_launch_mncc_grid_scene(const float* ref, const float* ref_mask, const float* views, const float* view_masks, const float* centres,
                               int B, int V, int H, int W, int P, float width, float* scores, void* workspace, hipStream_t stream) {
    const ScenePlan p = plan(B, V, H, W, P);
    const SceneWorkspace w = carve(workspace, p);
    const unsigned bv = (unsigned)(B * V);
    HrnProfScope prof("mncc_grid_scene", level_flops(P) * B * V * H * W, 4.0 * B * V * (4.0 * H * W + P * P), stream);
    launch_means(ref, ref_mask, views, view_masks, B, V, H, W, p, w.means, stream);
    HRN_LAUNCH_CHECK();
    hipLaunchKernelGGL(scene_level_kernel, dim3(bv * p.tiles), dim3(SC_THREADS), 0, stream, ref, ref_mask, views, view_masks, centres,
                       (const double*)w.means, p.chunks, bv, V, H, W, P, (double)width, p.tiles_x, p.tiles, w.sums);
    HRN_LAUNCH_CHECK();
    hipLaunchKernelGGL(scene_finish_kernel, dim3(bv), dim3(SC_FINISH_THREADS), 0, stream, (const double*)w.sums, centres, P, (double)width,
                       p.tiles, scores, (float*)nullptr, (float*)nullptr, 0, (float*)nullptr);
    HRN_LAUNCH_CHECK();
    return 0;
}

// The search with its first centre read from init (B,V,2); null: (0, 0).  last_trace (used where `trace` is null; may be null): the last
// level's (dy, dx, score) of view v goes to last_trace[v * last_stride] (registration_pyramid.hip: one row per octave).
int hrn_launch_mncc_search_scene_from(const float* ref, const float* ref_mask, const float* views, const float* view_masks, const float* init,
                                      int B, int V, int H, int W, int P, int levels, float radius, float* shifts, float* trace,
                                      float* last_trace, int last_stride, void* workspace, hipStream_t stream) {
    const ScenePlan p = plan(B, V, H, W, P);
    const SceneWorkspace w = carve(workspace, p);
    const unsigned bv = (unsigned)(B * V);
    HrnProfScope prof("mncc_search_scene", level_flops(P) * levels * B * V * H * W, 4.0 * B * V * (2.0 + 2.0 * levels) * H * W, stream);
    launch_means(ref, ref_mask, views, view_masks, B, V, H, W, p, w.means, stream);
    HRN_LAUNCH_CHECK();
    double width = (double)(2.f * radius);
    const double ratio = level_ratio(P);
    for (int k = 0; k < levels; ++k) {
        const float* centres = k ? w.centres : init;             // the first centre is init's, (0, 0) without one
        const bool last = k == levels - 1;
        hipLaunchKernelGGL(scene_level_kernel, dim3(bv * p.tiles), dim3(SC_THREADS), 0, stream, ref, ref_mask, views, view_masks, centres,
                           (const double*)w.means, p.chunks, bv, V, H, W, P, width, p.tiles_x, p.tiles, w.sums);
        HRN_LAUNCH_CHECK();
        hipLaunchKernelGGL(scene_finish_kernel, dim3(bv), dim3(SC_FINISH_THREADS), 0, stream, (const double*)w.sums, centres, P, width, p.tiles,
                           (float*)nullptr, w.centres, trace ? trace + 3 * k : (last ? last_trace : (float*)nullptr),
                           trace ? 3 * levels : last_stride, last ? shifts : (float*)nullptr);
        HRN_LAUNCH_CHECK();
        width = width * ratio;
    }
    return 0;
}

int hrn_launch_mncc_apply_scene(const float* views, const float* view_masks, const float* shifts, int B, int V, int H, int W, float* out,
                                float* out_valid, hipStream_t stream) {
    const ScenePlan p = plan(B, V, H, W, HRN_MNCC_MIN_POINTS);
    HrnProfScope prof("mncc_apply_scene", 2.0 * 12.0 * B * V * H * W, 4.0 * B * V * (4.0 * H * W + 2), stream);
    hipLaunchKernelGGL(scene_apply_kernel, dim3((unsigned)(B * V) * p.tiles), dim3(SC_THREADS), 0, stream, views, view_masks, shifts, H, W,
                       p.tiles_x, p.tiles, out, out_valid);
    HRN_LAUNCH_CHECK();
    return 0;
}
