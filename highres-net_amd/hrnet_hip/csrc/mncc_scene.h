// What the kernels of the tiled masked-NCC registration share (DESIGN.md sections 7g and 7i): registration_scene.hip, one shift per view,
// and registration_local.hip, a shift per block of tiles.  The tile, the LDS window and its staging, the two passes of the sampler, a
// grid level of a tile (scene_level) and the finish of a level over a rectangle of tiles (finish_tiles) are written once here, and so is
// the host's plan of the tiles and the workspace.
#pragma once
#include "kernels.h"
#include "mncc_common.h"            // also turns fp contraction off

namespace {

constexpr int SC_PMAX = HRN_MNCC_MAX_POINTS;
constexpr int SC_TILE = HRN_MNCC_SCENE_TILE;    // the core: 64 columns = one lane per column of a wave
constexpr int SC_THREADS = 256, SC_WAVES = SC_THREADS / 64;
constexpr int SC_ITEMS = (SC_TILE / RG_RUN) * SC_TILE / SC_THREADS;     // 2 runs a thread: 16 pixels
constexpr int SC_SPAN = 9;                      // the whole-pixel offsets of one level, less the smallest: 0..SC_SPAN
constexpr int SC_WIN = SC_TILE + SC_SPAN + 5;   // window rows and columns: offset - 2 .. offset + 3 around every core pixel
constexpr int SC_MEAN_CHUNK = HRN_MNCC_SCENE_MEAN_CHUNK, SC_MEAN_CHUNKS = HRN_MNCC_SCENE_MEAN_CHUNKS;

static_assert(SC_TILE == 64, "a lane owns a column of the core");
static_assert(SC_ITEMS * RG_RUN <= 32, "rbits is one 32-bit word");
static_assert(SC_ITEMS * SC_THREADS * RG_RUN == SC_TILE * SC_TILE, "the runs cover the core exactly");

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

// One run of one column for one (dy, dx): the six taps down RG_RUN + 5 rows of A, and which of the run's pixels are valid - inside the
// frame, footprint inside the frame, and the bilinear mask sample above 0.5.  yl: the run's first row in the core; (gy, gx): the same
// pixel in the frame; offy / offx: n_y / n_x less the level's smallest.  t[p] is defined only where bit p of the result is set.
__device__ __forceinline__ unsigned scene_column_run(const SceneShared& S, const float* ky, int ny, int nx, int offy, int offx,
                                                     unsigned table, int x, int yl, int gy, int gx, int H, int W, float* t) {
    float a[RG_RUN + 5];
#pragma unroll
    for (int m = 0; m < RG_RUN + 5; ++m) a[m] = S.A[(yl + offy + m) * SC_TILE + x];           // the last row: 56 + 9 + 12 < SC_WIN
    column_taps(ky, a, t);
    const bool xin = gx < W && gx + nx - 2 >= 0 && gx + nx + 3 <= W - 1;
    const unsigned char* pat = S.pat + (yl + offy + 2) * SC_WIN + x + offx + 2;               // the window's pixel (gy + n_y, gx + n_x)
    unsigned q[RG_RUN];
#pragma unroll
    for (int p = 0; p < RG_RUN; ++p) q[p] = pat[p * SC_WIN];
    return run_valid(xin, gy, ny, H, table, q);
}

__device__ __forceinline__ int min_whole(const int* whole, int P) {
    int m = whole[0];
    for (int i = 1; i < P; ++i) m = whole[i] < m ? whole[i] : m;
    return m;
}

// ----------------------------------------------------------------------------- one grid level of a tile
// The body of a level kernel: workgroup blockIdx.x owns tile `tile` of view `view` and writes its six sums at the P x P grid points of
// `width` around the centre pair number centre(view, tile) of `centres` ((0, 0) where `centres` is null) to
// sums[(blockIdx.x * P^2 + i P + j) * 6 + q].  The parameters are scene_level_kernel's, qualifiers included.
template <class Centre>
__device__ __forceinline__ void scene_level(const float* __restrict__ ref, const float* __restrict__ ref_mask, const float* __restrict__ views,
                                            const float* __restrict__ view_masks, const float* __restrict__ centres,
                                            const double* __restrict__ means, unsigned chunks, unsigned BV, int V, int H, int W, int P,
                                            double width, unsigned tiles_x, unsigned tiles, double* __restrict__ sums, Centre centre) {
    __shared__ SceneShared S;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t view = blockIdx.x / tiles, b = view / V, hw = (size_t)H * W;
    const unsigned tile = blockIdx.x - (unsigned)view * tiles;
    const int ty0 = (int)(tile / tiles_x) * SC_TILE, tx0 = (int)(tile % tiles_x) * SC_TILE;

    if (tid < 2 * P) {
        const int axis = tid / P, i = tid - axis * P;
        const double c = centres ? (double)centres[2 * centre(view, tile) + axis] : 0.0;
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
    float r[SC_ITEMS][RG_RUN];
    unsigned rbits = 0;
    const int x = lane, gx = tx0 + x;
    {
        const float* rp = ref + b * hw;
        const float* rm = ref_mask ? ref_mask + b * hw : nullptr;
        const float mean = S.mean[1];
#pragma unroll
        for (int k = 0; k < SC_ITEMS; ++k)
#pragma unroll
            for (int p = 0; p < RG_RUN; ++p) {
                const int gy = ty0 + (wave + k * SC_WAVES) * RG_RUN + p;
                const bool in = gy < H && gx < W;
                const size_t g = in ? (size_t)gy * W + gx : 0;
                const bool m = in && (rm ? rm[g] != 0.f : true);
                r[k][p] = m ? rp[g] - mean : 0.f;
                rbits |= (unsigned)m << (RG_RUN * k + p);
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
            PointSums sum;
            if (jok && offy <= SC_SPAN) {
#pragma unroll
                for (int k = 0; k < SC_ITEMS; ++k) {
                    const int yl = (wave + k * SC_WAVES) * RG_RUN;
                    float t[RG_RUN];
                    const unsigned c = scene_column_run(S, ky, ny, nx, offy, offx, table, x, yl, ty0 + yl, gx, H, W, t) & (rbits >> (RG_RUN * k));
                    sum.add(c, t, r[k]);
                }
            }
            sum.to_wave(S.red[i][wave], lane);
        }
        __syncthreads();                         // A and S.red are free again after this
        add_waves<SC_WAVES>(S.red, S.tot, P, j, tid);
    }
    __syncthreads();
    double* out = sums + (size_t)blockIdx.x * (P * P * RG_NSUM);
    const double* tot = &S.tot[0][0];
    for (int i = tid; i < P * P * RG_NSUM; i += SC_THREADS) out[i] = tot[i];
}

// ----------------------------------------------------------------------------- the finish of a level
constexpr int SC_FINISH_THREADS = 128;
static_assert(SC_FINISH_THREADS >= SC_PMAX * SC_PMAX, "a thread per grid point");

struct FinishShared {
    float score[SC_PMAX * SC_PMAX];
    double count[SC_PMAX * SC_PMAX];            // n, the first of the six sums
    float coord[2][SC_PMAX];
};

// The P x P grid of `width` around (cy, cx) over the tiles [ty0, ty1) x [tx0, tx1) of a view, tiles_x a row, whose sums begin at
// `sums`: the six sums of the tiles added in row-major order per grid point, then F.score and F.count.  With `search`, thread 0 then
// takes the first maximum: (cy, cx) becomes its point, its score is returned, centre_out = the point and trace = (dy, dx, score)
// (each may be null).  All SC_FINISH_THREADS threads call it; it holds one barrier, after F is written.
__device__ __forceinline__ float finish_tiles(FinishShared& F, const double* __restrict__ sums, unsigned tiles_x, unsigned ty0, unsigned ty1,
                                              unsigned tx0, unsigned tx1, int P, double width, float& cy, float& cx, bool search,
                                              float* centre_out, float* trace, int tid) {
    const int pp = P * P;
    if (tid < 2 * P) {
        const int axis = tid / P, i = tid - axis * P;
        F.coord[axis][i] = grid_coord((double)(axis ? cx : cy), width, i, P);
    }
    if (tid < pp) {
        double s[RG_NSUM] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (unsigned ty = ty0; ty < ty1; ++ty)
            for (unsigned tx = tx0; tx < tx1; ++tx) {
                const double* in = sums + (((size_t)ty * tiles_x + tx) * pp + tid) * RG_NSUM;
#pragma unroll
                for (int q = 0; q < RG_NSUM; ++q) s[q] += in[q];
            }
        F.score[tid] = mncc_score(s);
        F.count[tid] = s[0];
    }
    __syncthreads();
    float best = -INFINITY;
    if (tid == 0 && search) {
        best = mncc_first_maximum(F.score, F.coord[0], F.coord[1], P, cy, cx);
        if (centre_out) { centre_out[0] = cy; centre_out[1] = cx; }
        if (trace) { trace[0] = cy; trace[1] = cx; trace[2] = best; }
    }
    return best;
}

// ----------------------------------------------------------------------------- the workspace of a tiled search
// the tiles of a frame, the chunks of its mean, and the three parts of the workspace in their order: the chunks' {sum, count} of every
// plane, the six sums of every tile at every grid point, the centres that a level hands to the next
struct ScenePlan {
    unsigned tiles_x, tiles_y, tiles, chunks;
    size_t means_bytes, sums_bytes, centres_bytes;
    size_t bytes() const { return means_bytes + sums_bytes + centres_bytes; }
};

ScenePlan plan(int B, int V, int H, int W, int P) {
    ScenePlan p;
    p.tiles_x = (unsigned)((W + SC_TILE - 1) / SC_TILE);
    p.tiles_y = (unsigned)((H + SC_TILE - 1) / SC_TILE);
    p.tiles = p.tiles_x * p.tiles_y;
    const size_t hw = (size_t)H * W, chunks = (hw + SC_MEAN_CHUNK - 1) / SC_MEAN_CHUNK;
    p.chunks = (unsigned)(chunks < (size_t)SC_MEAN_CHUNKS ? chunks : (size_t)SC_MEAN_CHUNKS);
    const size_t bv = (size_t)B * V;
    p.means_bytes = 16 * (bv + (size_t)B) * p.chunks;
    p.sums_bytes = 8 * (size_t)RG_NSUM * P * P * bv * p.tiles;
    p.centres_bytes = 8 * bv;                    // one (dy, dx) a view; registration_local.hip: one a block
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

}  // namespace
