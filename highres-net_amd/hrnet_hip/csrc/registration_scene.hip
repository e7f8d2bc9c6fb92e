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
// order, the quotient rounded to fp32), never per tile.  A thread adds its 16 pixels in fp32; the wave (WaveSums), the waves in order
// and - in the finishing kernel of a level - the tiles in index order are added in fp64.  A workgroup writes its 6 P^2 sums to the
// workspace; there is no atomic anywhere.  The finishing kernel forms the scores, takes the first maximum and writes the next centre to
// device memory, where the next level's launch reads it: nothing returns to the host between levels.  hrn_mncc_grid_scene and a level of
// hrn_mncc_search_scene are the same two kernels on the same partition, so their scores agree bit for bit.
//
// The span: a level's coordinates are d_0 <= ... <= d_{P-1} with d_{P-1} - d_0 <= 8 before the rounding to fp32 (width <= 8), so
// floor(d_{P-1}) - floor(d_0) <= 9.  A coordinate further than SC_SPAN whole pixels from the smallest cannot occur; the kernels skip it
// (its score would be -inf) rather than read outside the window.
#include "kernels.h"
#include "wave_sums.h"
#include "mncc_common.h"            // also turns fp contraction off

namespace {

constexpr int SC_PMAX = HRN_MNCC_MAX_POINTS;
constexpr int SC_TILE = HRN_MNCC_SCENE_TILE;    // the core: 64 columns = one lane per column of a wave
constexpr int SC_THREADS = 256, SC_WAVES = SC_THREADS / 64;
constexpr int SC_RUN = 8;                       // rows of one column that a thread takes at a time
constexpr int SC_ITEMS = (SC_TILE / SC_RUN) * SC_TILE / SC_THREADS;     // 2 runs a thread: 16 pixels
constexpr int SC_SPAN = 9;                      // the whole-pixel offsets of one level, less the smallest: 0..SC_SPAN
constexpr int SC_WIN = SC_TILE + SC_SPAN + 5;   // window rows and columns: offset - 2 .. offset + 3 around every core pixel
constexpr int SC_MEAN_CHUNK = HRN_MNCC_SCENE_MEAN_CHUNK, SC_MEAN_CHUNKS = HRN_MNCC_SCENE_MEAN_CHUNKS;

static_assert(SC_TILE == 64, "a lane owns a column of the core");
static_assert(SC_ITEMS * SC_RUN <= 32, "a thread adds at most 32 pixels in fp32, and rbits is one 32-bit word");
static_assert(SC_ITEMS * SC_THREADS * SC_RUN == SC_TILE * SC_TILE, "the runs cover the core exactly");

struct SceneShared {
    float T[SC_WIN * SC_WIN];                   // the window of the view, minus the view's mean (the search) or as it is (the resampler)
    float A[SC_WIN * SC_TILE];                  // the pass along rows for the current dx
    unsigned char pat[SC_WIN * SC_WIN];         // the four mask bits of the 2 x 2 neighbourhood of every window pixel
    double red[SC_PMAX][SC_WAVES][8];
    double tot[SC_PMAX * SC_PMAX][RG_NSUM];
    double frac[2][SC_PMAX];                    // f per grid coordinate, axis 0 = y
    float tap[2][SC_PMAX][6];
    int whole[2][SC_PMAX];                      // n per grid coordinate
    unsigned table[SC_PMAX * SC_PMAX];          // bit q: the bilinear sample of the 2 x 2 mask pattern q exceeds 0.5
    float mean[2];                              // of the view, of the reference
};
static_assert(sizeof(SceneShared) <= 64 * 1024, "two workgroups per CU");
static_assert(sizeof(float) * SC_WIN * SC_TILE >= SC_WIN * SC_WIN, "A holds the window's mask bytes while the patterns are formed");

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

// the mean of a plane out of its chunks, in their order, rounded to fp32 as registration.hip rounds it; 0 without a clear pixel
__device__ float plane_mean(const double* __restrict__ partial, size_t plane, unsigned chunks) {
    double s = 0.0, n = 0.0;
    for (unsigned c = 0; c < chunks; ++c) { s += partial[(plane * chunks + c) * 2]; n += partial[(plane * chunks + c) * 2 + 1]; }
    return n > 0.0 ? (float)(s / n) : 0.f;
}

// ----------------------------------------------------------------------------- the window
// Rows 0 .. ROWS - 1 and columns 0 .. COLS - 1 of the window whose pixel (0, 0) is the frame's (oy, ox): T = view - mean inside the
// frame and 0 outside, pat = the 2 x 2 mask patterns (a pixel outside the frame, or beyond the staged part, counts as masked).  S.A is
// scratch here.  Ends with a barrier.
template <int ROWS, int COLS>
__device__ void stage_window(const float* __restrict__ view, const float* __restrict__ mask, SceneShared& S, int oy, int ox, int H, int W,
                             float mean, int tid) {
    static_assert(ROWS <= SC_WIN && COLS <= SC_WIN, "inside the window");
    unsigned char* mb = reinterpret_cast<unsigned char*>(S.A);
    constexpr int n = ROWS * COLS, rows = ROWS, cols = COLS;
    for (int i = tid; i < n; i += SC_THREADS) {
        const int wy = i / cols, wx = i - wy * cols;
        const int y = oy + wy, x = ox + wx;
        const bool in = y >= 0 && y < H && x >= 0 && x < W;
        const size_t g = in ? (size_t)y * W + x : 0;
        S.T[wy * SC_WIN + wx] = in ? view[g] - mean : 0.f;
        mb[wy * SC_WIN + wx] = in && (mask ? mask[g] != 0.f : true);
    }
    __syncthreads();
    for (int i = tid; i < n; i += SC_THREADS) {
        const int wy = i / cols, wx = i - wy * cols, w = wy * SC_WIN + wx;
        const bool right = wx + 1 < cols, down = wy + 1 < rows;
        unsigned q = mb[w];
        if (right) q |= mb[w + 1] << 1;
        if (down) q |= mb[w + SC_WIN] << 2;
        if (right && down) q |= mb[w + SC_WIN + 1] << 3;
        S.pat[w] = (unsigned char)q;
    }
    __syncthreads();
}

// the pass along rows for one dx over `rows` window rows: A[wy][x] = sum_o tap[o] T[wy][x + off + o], off = n_x less the level's
// smallest, 0..SC_SPAN: the last column read is 63 + 9 + 5 < SC_WIN.  The operations and their order are registration.hip's row_pass.
__device__ void scene_row_pass(SceneShared& S, const float* tap, int off, int rows, int tid) {
    float k[6];
#pragma unroll
    for (int o = 0; o < 6; ++o) k[o] = tap[o];
    const int x = tid & 63;
    for (int wy = tid >> 6; wy < rows; wy += SC_WAVES) {
        const float* row = S.T + wy * SC_WIN + x + off;
        float a = k[0] * row[0];
#pragma unroll
        for (int o = 1; o < 6; ++o) a = fmaf(k[o], row[o], a);
        S.A[wy * SC_TILE + x] = a;
    }
}

// One run of one column for one (dy, dx): the six taps down SC_RUN + 5 rows of A, and which of the run's pixels are valid - inside the
// frame, footprint inside the frame, and the bilinear mask sample above 0.5.  yl: the run's first row in the core; (gy, gx): the same
// pixel in the frame; offy / offx: n_y / n_x less the level's smallest.  t[p] is defined only where bit p of the result is set.
__device__ __forceinline__ unsigned scene_column_run(const SceneShared& S, const float* ky, int ny, int nx, int offy, int offx,
                                                     unsigned table, int x, int yl, int gy, int gx, int H, int W, float* t) {
    float a[SC_RUN + 5];
#pragma unroll
    for (int m = 0; m < SC_RUN + 5; ++m) a[m] = S.A[(yl + offy + m) * SC_TILE + x];           // the last row: 56 + 9 + 12 < SC_WIN
    const bool xin = gx < W && gx + nx - 2 >= 0 && gx + nx + 3 <= W - 1;
    const unsigned char* pat = S.pat + (yl + offy + 2) * SC_WIN + x + offx + 2;               // the window's pixel (gy + n_y, gx + n_x)
    unsigned valid = 0;
#pragma unroll
    for (int p = 0; p < SC_RUN; ++p) {
        float s = ky[0] * a[p];
#pragma unroll
        for (int o = 1; o < 6; ++o) s = fmaf(ky[o], a[p + o], s);
        t[p] = s;
        const int y = gy + p;
        const bool yin = y < H && y + ny - 2 >= 0 && y + ny + 3 <= H - 1;
        const unsigned q = pat[p * SC_WIN];
        valid |= (unsigned)(xin && yin && ((table >> q) & 1u)) << p;
    }
    return valid;
}

__device__ __forceinline__ int min_whole(const int* whole, int P) {
    int m = whole[0];
    for (int i = 1; i < P; ++i) m = whole[i] < m ? whole[i] : m;
    return m;
}

// ----------------------------------------------------------------------------- one grid level: the tiles' sums
// sums[((view * tiles + tile) * P^2 + i P + j) * 6 + q]: the six sums of tile `tile` of view `view` at (dy_i, dx_j) of the P x P grid
// of `width` around centres[view] ((0, 0) where `centres` is null).  grid (B V tiles), tiles = tiles_x * tiles_y
__global__ __launch_bounds__(SC_THREADS) void scene_level_kernel(const float* __restrict__ ref, const float* __restrict__ ref_mask,
                                                                 const float* __restrict__ views, const float* __restrict__ view_masks,
                                                                 const float* __restrict__ centres, const double* __restrict__ means,
                                                                 unsigned chunks, unsigned BV, int V, int H, int W, int P, double width,
                                                                 unsigned tiles_x, unsigned tiles, double* __restrict__ sums) {
    __shared__ SceneShared S;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t view = blockIdx.x / tiles, b = view / V, hw = (size_t)H * W;
    const unsigned tile = blockIdx.x - (unsigned)view * tiles;
    const int ty0 = (int)(tile / tiles_x) * SC_TILE, tx0 = (int)(tile % tiles_x) * SC_TILE;

    if (tid < 2 * P) {
        const int axis = tid / P, i = tid - axis * P;
        const double c = centres ? (double)centres[2 * view + axis] : 0.0;
        split_and_taps(grid_coord(c, width, i, P), &S.whole[axis][i], &S.frac[axis][i], S.tap[axis][i]);
    }
    if (tid == 64) S.mean[0] = plane_mean(means, view, chunks);
    if (tid == 128) S.mean[1] = plane_mean(means, (size_t)BV + b, chunks);
    __syncthreads();
    if (tid < P * P) S.table[tid] = mask_table(S.frac[0][tid / P], S.frac[1][tid % P]);
    const int ny0 = min_whole(S.whole[0], P), nx0 = min_whole(S.whole[1], P);
    stage_window<SC_WIN, SC_WIN>(views + view * hw, view_masks ? view_masks + view * hw : nullptr, S, ty0 + ny0 - 2, tx0 + nx0 - 2, H, W,
                                 S.mean[0], tid);

    // this thread's pixels of the reference, centred on the reference's mean under its own mask and zero where that mask is set
    float r[SC_ITEMS][SC_RUN];
    unsigned rbits = 0;
    const int x = lane, gx = tx0 + x;
    {
        const float* rp = ref + b * hw;
        const float* rm = ref_mask ? ref_mask + b * hw : nullptr;
        const float mean = S.mean[1];
#pragma unroll
        for (int k = 0; k < SC_ITEMS; ++k)
#pragma unroll
            for (int p = 0; p < SC_RUN; ++p) {
                const int gy = ty0 + (wave + k * SC_WAVES) * SC_RUN + p;
                const bool in = gy < H && gx < W;
                const size_t g = in ? (size_t)gy * W + gx : 0;
                const bool m = in && (rm ? rm[g] != 0.f : true);
                r[k][p] = m ? rp[g] - mean : 0.f;
                rbits |= (unsigned)m << (SC_RUN * k + p);
            }
    }

#pragma unroll 1
    for (int j = 0; j < P; ++j) {
        const int nx = S.whole[1][j], offx = nx - nx0;
        const bool jok = offx <= SC_SPAN;
        if (jok) scene_row_pass(S, S.tap[1][j], offx, SC_WIN, tid);
        __syncthreads();
#pragma unroll 1
        for (int i = 0; i < P; ++i) {
            const int ny = S.whole[0][i], offy = ny - ny0;
            const unsigned table = S.table[i * P + j];
            float ky[6];
#pragma unroll
            for (int o = 0; o < 6; ++o) ky[o] = S.tap[0][i][o];
            int n = 0;
            float st = 0.f, sr = 0.f, stt = 0.f, srr = 0.f, srt = 0.f;
            if (jok && offy <= SC_SPAN) {
#pragma unroll
                for (int k = 0; k < SC_ITEMS; ++k) {
                    const int yl = (wave + k * SC_WAVES) * SC_RUN;
                    float t[SC_RUN];
                    const unsigned c = scene_column_run(S, ky, ny, nx, offy, offx, table, x, yl, ty0 + yl, gx, H, W, t) & (rbits >> (SC_RUN * k));
#pragma unroll
                    for (int p = 0; p < SC_RUN; ++p) {
                        const bool on = (c >> p) & 1u;
                        const float tm = on ? t[p] : 0.f, rm = on ? r[k][p] : 0.f;
                        n += on;
                        st += tm; sr += rm;
                        stt = fmaf(tm, tm, stt); srr = fmaf(rm, rm, srr); srt = fmaf(rm, tm, srt);
                    }
                }
            }
            double v[8] = {(double)n, (double)st, (double)sr, (double)stt, (double)srr, (double)srt, 0.0, 0.0};
            WaveSums<8, 0>::run(v, lane);
            if (lane < 8) S.red[i][wave][wave_sums_index<8>(lane)] = v[0];
        }
        __syncthreads();                         // A and S.red are free again after this
        if (tid < P * RG_NSUM) {
            const int i = tid / RG_NSUM, q = tid - i * RG_NSUM;
            double s = 0.0;
            for (int w = 0; w < SC_WAVES; ++w) s += S.red[i][w][q];
            S.tot[i * P + j][q] = s;
        }
    }
    __syncthreads();
    double* out = sums + (size_t)blockIdx.x * (P * P * RG_NSUM);
    const double* tot = &S.tot[0][0];
    for (int i = tid; i < P * P * RG_NSUM; i += SC_THREADS) out[i] = tot[i];
}

// ----------------------------------------------------------------------------- one grid level: the finish
// Per view: the tiles' sums added in index order, the P^2 scores, and - for the search - the first maximum: centres_out[view] = the
// best point, trace_k[view * trace_stride] = (dy, dx, score), shifts[view] = the best point (each may be null).  centres_in null: (0, 0).
// centres_out may be centres_in.  grid (B V), 128 threads
constexpr int SC_FINISH_THREADS = 128;
static_assert(SC_FINISH_THREADS >= SC_PMAX * SC_PMAX, "a thread per grid point");

__global__ __launch_bounds__(SC_FINISH_THREADS) void scene_finish_kernel(const double* __restrict__ sums, const float* centres_in, int P,
                                                                         double width, unsigned tiles, float* __restrict__ scores,
                                                                         float* centres_out, float* __restrict__ trace_k,
                                                                         int trace_stride, float* __restrict__ shifts) {
    __shared__ float score[SC_PMAX * SC_PMAX];
    __shared__ float coord[2][SC_PMAX];
    const int tid = threadIdx.x, pp = P * P;
    const size_t view = blockIdx.x;
    float cy = centres_in ? centres_in[2 * view] : 0.f, cx = centres_in ? centres_in[2 * view + 1] : 0.f;
    if (tid < 2 * P) {
        const int axis = tid / P, i = tid - axis * P;
        coord[axis][i] = grid_coord((double)(axis ? cx : cy), width, i, P);
    }
    if (tid < pp) {
        double s[RG_NSUM] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        const double* in = sums + (view * tiles * pp + tid) * RG_NSUM;
        for (unsigned t = 0; t < tiles; ++t, in += (size_t)pp * RG_NSUM)
#pragma unroll
            for (int q = 0; q < RG_NSUM; ++q) s[q] += in[q];
        float sc;
        MNCC_SCORE(s, sc);
        score[tid] = sc;
        if (scores) scores[view * pp + tid] = sc;
    }
    __syncthreads();
    if (tid == 0 && (centres_out || trace_k || shifts)) {
        float best;
        MNCC_FIRST_MAXIMUM(score, coord[0], coord[1], P, best, cy, cx);
        if (centres_out) { centres_out[2 * view] = cy; centres_out[2 * view + 1] = cx; }
        if (trace_k) {
            float* tr = trace_k + view * trace_stride;
            tr[0] = cy; tr[1] = cx; tr[2] = best;
        }
        if (shifts) { shifts[2 * view] = cy; shifts[2 * view + 1] = cx; }
    }
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
        const int yl = (wave + k * SC_WAVES) * SC_RUN, gy = ty0 + yl;
        float t[SC_RUN];
        const unsigned c = scene_column_run(S, ky, ny, nx, 0, 0, table, x, yl, gy, gx, H, W, t);
        if (gx >= W) continue;
#pragma unroll
        for (int p = 0; p < SC_RUN; ++p) {
            if (gy + p >= H) break;
            const bool on = (c >> p) & 1u;
            const size_t i = view * hw + (size_t)(gy + p) * W + gx;
            out[i] = on ? t[p] : 0.f;
            out_valid[i] = on ? 1.f : 0.f;
        }
    }
}

double level_ratio(int P) {                      // as registration.hip: 1 / (P - 2), at least 0.25, and 0.9 where that is not below 1
    const double s = 1.0 / (double)(P - 2);
    return s >= 1.0 ? 0.9 : (s < 0.25 ? 0.25 : s);
}

// the counted arithmetic of one level, per pixel, as registration.hip counts it
double level_flops(int P) { return P * 12.0 + (double)P * P * 32.0; }

struct ScenePlan {
    unsigned tiles_x, tiles, chunks;
    size_t means_bytes, centres_bytes, sums_bytes;
};

ScenePlan plan(int B, int V, int H, int W, int P) {
    ScenePlan p;
    p.tiles_x = (unsigned)((W + SC_TILE - 1) / SC_TILE);
    p.tiles = p.tiles_x * (unsigned)((H + SC_TILE - 1) / SC_TILE);
    const size_t hw = (size_t)H * W, chunks = (hw + SC_MEAN_CHUNK - 1) / SC_MEAN_CHUNK;
    p.chunks = (unsigned)(chunks < (size_t)SC_MEAN_CHUNKS ? chunks : (size_t)SC_MEAN_CHUNKS);
    const size_t bv = (size_t)B * V;
    p.means_bytes = 16 * (bv + (size_t)B) * p.chunks;
    p.sums_bytes = 8 * (size_t)RG_NSUM * P * P * bv * p.tiles;
    p.centres_bytes = 8 * bv;
    return p;
}

struct SceneWorkspace {
    double* means;
    double* sums;
    float* centres;
};

SceneWorkspace carve(void* workspace, const ScenePlan& p) {
    SceneWorkspace w;
    unsigned char* base = static_cast<unsigned char*>(workspace);
    w.means = reinterpret_cast<double*>(base);
    w.sums = reinterpret_cast<double*>(base + p.means_bytes);
    w.centres = reinterpret_cast<float*>(base + p.means_bytes + p.sums_bytes);
    return w;
}

void launch_means(const float* ref, const float* ref_mask, const float* views, const float* view_masks, int B, int V, int H, int W,
                  const ScenePlan& p, double* means, hipStream_t stream) {
    const unsigned bv = (unsigned)(B * V);
    hipLaunchKernelGGL(scene_mean_kernel, dim3((bv + (unsigned)B) * p.chunks), dim3(SC_THREADS), 0, stream, ref, ref_mask, views, view_masks,
                       bv, (size_t)H * W, p.chunks, means);
}

}  // namespace

size_t hrn_mncc_scene_workspace_bytes_impl(int B, int V, int H, int W, int P) {
    const ScenePlan p = plan(B, V, H, W, P);
    return p.means_bytes + p.sums_bytes + p.centres_bytes;
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

int hrn_launch_mncc_search_scene(const float* ref, const float* ref_mask, const float* views, const float* view_masks, int B, int V, int H,
                                 int W, int P, int levels, float radius, float* shifts, float* trace, void* workspace, hipStream_t stream) {
    const ScenePlan p = plan(B, V, H, W, P);
    const SceneWorkspace w = carve(workspace, p);
    const unsigned bv = (unsigned)(B * V);
    HrnProfScope prof("mncc_search_scene", level_flops(P) * levels * B * V * H * W, 4.0 * B * V * (2.0 + 2.0 * levels) * H * W, stream);
    launch_means(ref, ref_mask, views, view_masks, B, V, H, W, p, w.means, stream);
    HRN_LAUNCH_CHECK();
    double width = (double)(2.f * radius);
    const double ratio = level_ratio(P);
    for (int k = 0; k < levels; ++k) {
        const float* centres = k ? w.centres : nullptr;          // the first centre is (0, 0)
        hipLaunchKernelGGL(scene_level_kernel, dim3(bv * p.tiles), dim3(SC_THREADS), 0, stream, ref, ref_mask, views, view_masks, centres,
                           (const double*)w.means, p.chunks, bv, V, H, W, P, width, p.tiles_x, p.tiles, w.sums);
        HRN_LAUNCH_CHECK();
        hipLaunchKernelGGL(scene_finish_kernel, dim3(bv), dim3(SC_FINISH_THREADS), 0, stream, (const double*)w.sums, centres, P, width, p.tiles,
                           (float*)nullptr, w.centres, trace ? trace + 3 * k : (float*)nullptr, 3 * levels,
                           k == levels - 1 ? shifts : (float*)nullptr);
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
