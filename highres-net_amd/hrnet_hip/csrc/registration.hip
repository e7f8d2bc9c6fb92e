// Sub-pixel registration of LR views by a masked-NCC grid search (the method of the reference fork's
// registration_search.py - recursive_mncc_search over compute_grid_mncc - on this project's own definitions, include/hrnet_hip.h).
//
// A workgroup owns one view.  It keeps three planes in LDS for the whole search: the view T, minus its masked mean, as fp32; the buffer
// A of the pass along rows; and, per pixel, the four mask bits of the 2 x 2 neighbourhood the bilinear mask sample reads.  The pass
// along rows depends on dx alone, so a level does it P times into A, not P^2 times; for each dy the pass along columns then reads a
// thread's 8 + 5 rows of one column out of A and slides the six taps down them in registers.  A lane owns a column, so a wave reads
// consecutive floats of one LDS row: conflict-free at any frame width.  The thread's pixels of the masked, centred reference stay in
// VGPRs from the first level to the last.
//
// The bilinear sample of a 0/1 mask takes one of 16 values per grid point, so whether it exceeds 0.5 is a 16-bit table per grid point,
// computed once in fp64 exactly as the definition writes it: the per-pixel test is a byte read and a shift, and it cannot fall on the
// other side of 0.5 than the fp64 restatement does.  The taps are computed in fp64 and rounded to fp32 once per grid coordinate.
//
// Sums: a thread adds its (at most 32) pixels in fp64, and the workgroup adds the threads in fp64 in a fixed order (WaveSums, then the
// waves in order).  The images are centred on whole-frame means, which keeps sum t^2 / n - mu^2 from cancelling only where the scored
// pixels have those means; under a mask that hides a bright region in one image they do not, and fp32 sums of a thread then cost a
// score of contrast 0.01 up to 2e-5 ("Sums").  No atomics: the result is bit-reproducible, and
// hrn_mncc_grid and a level of hrn_mncc_search are the same device function, so their scores agree bit for bit.
#include "kernels.h"
#include "mncc_common.h"            // what the tiled paths share with this one, a thread's sums and the end of a level among it; it also
                                    // turns fp contraction off

namespace {

constexpr int RG_MAX = HRN_MNCC_MAX_SIDE, RG_PMAX = HRN_MNCC_MAX_POINTS;
constexpr int RG_THREADS = 512, RG_WAVES = RG_THREADS / 64;
constexpr int RG_ITEMS = (RG_MAX / RG_RUN) * RG_MAX / RG_THREADS;   // such runs per thread at 128 x 128

struct RegShared {
    double red[RG_PMAX][RG_WAVES][8];
    double tot[RG_PMAX * RG_PMAX][RG_NSUM];
    double frac[2][RG_PMAX];                    // f per grid coordinate, axis 0 = y
    float coord[2][RG_PMAX];                    // d per grid coordinate, as the caller sees it
    float tap[2][RG_PMAX][6];
    int whole[2][RG_PMAX];                      // n per grid coordinate
    unsigned table[RG_PMAX * RG_PMAX];          // bit q: the bilinear sample of the 2 x 2 mask pattern q exceeds 0.5
    float score[RG_PMAX * RG_PMAX];
    float best[3];
};

// the sums of the whole workgroup, in a fixed order: every thread gets sum over threads of v[i], i < N (N a power of two <= 8)
template <int N>
__device__ void block_sums(double* v, RegShared& S, int tid) {
    const int lane = tid & 63, wave = tid >> 6;
    WaveSums<N, 0>::run(v, lane);
    const int idx = wave_sums_index<N>(lane);
    __syncthreads();
    if (lane < N) S.red[0][wave][idx] = v[0];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < N; ++i) {
        double s = 0.0;
        for (int w = 0; w < RG_WAVES; ++w) s += S.red[0][w][i];
        v[i] = s;
    }
    __syncthreads();
}

// What a thread keeps for the whole kernel: where its runs lie, and its pixels of the centred reference under the reference's mask.
struct RegThread {
    int x[RG_ITEMS], y0[RG_ITEMS];              // y0 < 0: no such run
    float r[RG_ITEMS][RG_RUN];
    unsigned rbits;                             // bit RG_RUN k + p: pixel p of run k is inside the frame and clear in the reference's mask
};

__device__ void thread_runs(RegThread& t, int H, int W, int tid) {
    const int nitems = W * ((H + RG_RUN - 1) / RG_RUN);
#pragma unroll
    for (int k = 0; k < RG_ITEMS; ++k) {
        const int item = tid + k * RG_THREADS;
        const int run = item / W;
        t.x[k] = item - run * W;
        t.y0[k] = item < nitems ? run * RG_RUN : -1;
    }
}

// The view into LDS: T = view - its mean under its own mask, pat = the 2 x 2 mask patterns.  `A` is scratch here.  Ends with a barrier.
__device__ void stage_view(const float* __restrict__ view, const float* __restrict__ mask, float* T, float* A, unsigned char* pat,
                           RegShared& S, int H, int W, int tid, bool centre) {
    const int hw = H * W;
    unsigned char* mb = reinterpret_cast<unsigned char*>(A);
    double v[2] = {0.0, 0.0};
    for (int i = tid; i < hw; i += RG_THREADS) {
        const float t = view[i];
        const bool m = mask ? mask[i] != 0.f : true;
        T[i] = t;
        mb[i] = m;
        if (m) { v[0] += (double)t; v[1] += 1.0; }
    }
    float mean = 0.f;
    if (centre) {
        block_sums<2>(v, S, tid);
        mean = v[1] > 0.0 ? (float)(v[0] / v[1]) : 0.f;
    } else {
        __syncthreads();
    }
    int y = tid / W, x = tid - y * W;
    const int dy = RG_THREADS / W, dx = RG_THREADS - dy * W;
    for (int i = tid; i < hw; i += RG_THREADS) {
        if (centre) T[i] -= mean;
        const bool right = x + 1 < W, down = y + 1 < H;
        unsigned q = mb[i];
        if (right) q |= mb[i + 1] << 1;
        if (down) q |= mb[i + W] << 2;
        if (right && down) q |= mb[i + W + 1] << 3;
        pat[i] = (unsigned char)q;
        x += dx; y += dy;
        if (x >= W) { x -= W; ++y; }
    }
    __syncthreads();
}

// the pass along rows for one dx: A[y][x] = sum_o tap[o] T[y][x + n + o - 2], columns clamped into the frame (a pixel whose footprint
// leaves the frame is never used)
__device__ void row_pass(const float* T, float* A, const float* tap, int n, int H, int W, int tid) {
    float k[6];
#pragma unroll
    for (int o = 0; o < 6; ++o) k[o] = tap[o];
    const int hw = H * W;
    int y = tid / W, x = tid - y * W;
    const int dy = RG_THREADS / W, dx = RG_THREADS - dy * W;
    for (int i = tid; i < hw; i += RG_THREADS) {
        const float* row = T + y * W;
        float a = k[0] * row[clampi(x + n - 2, 0, W - 1)];
#pragma unroll
        for (int o = 1; o < 6; ++o) a = fmaf(k[o], row[clampi(x + n + o - 2, 0, W - 1)], a);
        A[i] = a;
        x += dx; y += dy;
        if (x >= W) { x -= W; ++y; }
    }
}

// One run of one column for one (dy, dx): the six taps down RG_RUN + 5 rows of A, and which of the run's pixels are valid - footprint
// inside the frame and the bilinear mask sample above 0.5.  t[p] is defined only where bit p of the result is set.
__device__ __forceinline__ unsigned column_run(const float* A, const unsigned char* pat, const float* ky, int ny, int nx, unsigned table,
                                               int x, int y0, int H, int W, float* t) {
    float a[RG_RUN + 5];
#pragma unroll
    for (int m = 0; m < RG_RUN + 5; ++m) a[m] = A[clampi(y0 + ny - 2 + m, 0, H - 1) * W + x];
    column_taps(ky, a, t);
    const bool xin = x + nx - 2 >= 0 && x + nx + 3 <= W - 1;
    const int xp = clampi(x + nx, 0, W - 1);
    unsigned q[RG_RUN];
#pragma unroll
    for (int p = 0; p < RG_RUN; ++p) q[p] = pat[clampi(y0 + p + ny, 0, H - 1) * W + xp];
    return run_valid(xin, y0, ny, H, table, q);
}

// One grid level: S.score[i P + j] = the score at (dy_i, dx_j) of the P x P grid of `width` around (cy, cx).  Ends with a barrier.
__device__ void mncc_level(const float* T, float* A, const unsigned char* pat, RegShared& S, const RegThread& th, int H, int W, int P,
                           float cy, float cx, double width, int tid) {
    if (tid < 2 * P) {
        const int axis = tid / P, i = tid - axis * P;
        const double c = (double)(axis ? cx : cy);
        const float d = grid_coord(c, width, i, P);
        S.coord[axis][i] = d;
        split_and_taps(d, &S.whole[axis][i], &S.frac[axis][i], S.tap[axis][i]);
    }
    __syncthreads();
    if (tid < P * P) S.table[tid] = mask_table(S.frac[0][tid / P], S.frac[1][tid % P]);
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll 1
    for (int j = 0; j < P; ++j) {
        const int nx = S.whole[1][j];
        row_pass(T, A, S.tap[1][j], nx, H, W, tid);
        __syncthreads();
#pragma unroll 1
        for (int i = 0; i < P; ++i) {
            const int ny = S.whole[0][i];
            const unsigned table = S.table[i * P + j];
            float ky[6];
#pragma unroll
            for (int o = 0; o < 6; ++o) ky[o] = S.tap[0][i][o];
            PointSums sum;
#pragma unroll
            for (int k = 0; k < RG_ITEMS; ++k) {
                if (th.y0[k] < 0) continue;
                float t[RG_RUN];
                const unsigned c = column_run(A, pat, ky, ny, nx, table, th.x[k], th.y0[k], H, W, t) & (th.rbits >> (RG_RUN * k));
                sum.add(c, t, th.r[k]);
            }
            sum.to_wave(S.red[i][wave], lane);
        }
        __syncthreads();                         // A and S.red are free again after this
        add_waves<RG_WAVES>(S.red, S.tot, P, j, tid);
    }
    __syncthreads();
    if (tid < P * P) S.score[tid] = mncc_score(S.tot[tid]);
    __syncthreads();
}

// the reference's pixels of this thread's runs, centred on the reference's mean under its own mask and zero where that mask is set
__device__ void stage_reference(const float* __restrict__ ref, const float* __restrict__ ref_mask, RegThread& th, RegShared& S, int H, int W,
                                int tid) {
    double v[2] = {0.0, 0.0};
    th.rbits = 0;
#pragma unroll
    for (int k = 0; k < RG_ITEMS; ++k)
#pragma unroll
        for (int p = 0; p < RG_RUN; ++p) {
            const int y = th.y0[k] + p;
            const bool in = th.y0[k] >= 0 && y < H;
            const int i = in ? y * W + th.x[k] : 0;
            const float r = in ? ref[i] : 0.f;
            const bool m = in && (ref_mask ? ref_mask[i] != 0.f : true);
            th.r[k][p] = r;
            th.rbits |= (unsigned)m << (RG_RUN * k + p);
            if (m) { v[0] += (double)r; v[1] += 1.0; }
        }
    block_sums<2>(v, S, tid);
    const float mean = v[1] > 0.0 ? (float)(v[0] / v[1]) : 0.f;
#pragma unroll
    for (int k = 0; k < RG_ITEMS; ++k)
#pragma unroll
        for (int p = 0; p < RG_RUN; ++p) th.r[k][p] = (th.rbits >> (RG_RUN * k + p)) & 1u ? th.r[k][p] - mean : 0.f;
}

struct RegLds {
    float* T;
    float* A;
    unsigned char* pat;
};
__device__ __forceinline__ RegLds carve(unsigned char* lds, int H, int W) {
    RegLds l;
    l.T = reinterpret_cast<float*>(lds);
    l.A = l.T + H * W;
    l.pat = reinterpret_cast<unsigned char*>(l.A + H * W);
    return l;
}
size_t lds_bytes(int H, int W) { return (size_t)H * W * 9; }

static_assert(RG_ITEMS * RG_RUN <= 32, "RegThread::rbits is one 32-bit word");
static_assert((size_t)RG_MAX * RG_MAX * 9 + sizeof(RegShared) <= 160 * 1024, "LDS budget");

// levels == 0: one grid level around centres[view] of width `width0`, scores (B V, P, P) written.  levels > 0: the search from (0, 0)
// with first width `width0`, shifts (B V, 2) and trace (B V, levels, 3) (may be null) written.  grid (B V), RG_THREADS threads.
__global__ __launch_bounds__(RG_THREADS) void mncc_kernel(const float* __restrict__ ref, const float* __restrict__ ref_mask,
                                                          const float* __restrict__ views, const float* __restrict__ view_masks,
                                                          const float* __restrict__ centres, int V, int H, int W, int P, int levels,
                                                          float width0, double ratio, float* __restrict__ scores,
                                                          float* __restrict__ shifts, float* __restrict__ trace) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    __shared__ RegShared S;
    const int tid = threadIdx.x;
    const size_t view = blockIdx.x, b = view / V, hw = (size_t)H * W;
    const RegLds l = carve(lds, H, W);
    RegThread th;
    thread_runs(th, H, W, tid);
    stage_reference(ref + b * hw, ref_mask ? ref_mask + b * hw : nullptr, th, S, H, W, tid);
    stage_view(views + view * hw, view_masks ? view_masks + view * hw : nullptr, l.T, l.A, l.pat, S, H, W, tid, true);

    if (levels == 0) {
        mncc_level(l.T, l.A, l.pat, S, th, H, W, P, centres[2 * view], centres[2 * view + 1], (double)width0, tid);
        if (tid < P * P) scores[view * P * P + tid] = S.score[tid];
        return;
    }
    float cy = 0.f, cx = 0.f;
    double width = (double)width0;
    for (int k = 0; k < levels; ++k) {
        mncc_level(l.T, l.A, l.pat, S, th, H, W, P, cy, cx, width, tid);
        if (tid == 0) {                          // the first maximum in row-major order; without a finite score the centre stays
            const float best = mncc_first_maximum(S.score, S.coord[0], S.coord[1], P, cy, cx);
            S.best[0] = cy; S.best[1] = cx; S.best[2] = best;
            if (trace) {
                float* tr = trace + (view * levels + k) * 3;
                tr[0] = cy; tr[1] = cx; tr[2] = best;
            }
        }
        __syncthreads();
        cy = S.best[0]; cx = S.best[1];
        width = width * ratio;
    }
    if (tid == 0) { shifts[2 * view] = cy; shifts[2 * view + 1] = cx; }
}

// out = S(view, shift), out_valid = V(mask, shift); grid (B V), RG_THREADS threads
__global__ __launch_bounds__(RG_THREADS) void mncc_apply_kernel(const float* __restrict__ views, const float* __restrict__ view_masks,
                                                                const float* __restrict__ shifts, int H, int W, float* __restrict__ out,
                                                                float* __restrict__ out_valid) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    __shared__ RegShared S;
    const int tid = threadIdx.x;
    const size_t view = blockIdx.x, hw = (size_t)H * W;
    const RegLds l = carve(lds, H, W);
    RegThread th;
    thread_runs(th, H, W, tid);
    stage_view(views + view * hw, view_masks ? view_masks + view * hw : nullptr, l.T, l.A, l.pat, S, H, W, tid, false);
    if (tid < 2) split_and_taps(shifts[2 * view + tid], &S.whole[tid][0], &S.frac[tid][0], S.tap[tid][0]);
    __syncthreads();
    if (tid == 0) S.table[0] = mask_table(S.frac[0][0], S.frac[1][0]);
    const int ny = S.whole[0][0], nx = S.whole[1][0];
    row_pass(l.T, l.A, S.tap[1][0], nx, H, W, tid);
    __syncthreads();
    const unsigned table = S.table[0];
    float ky[6];
#pragma unroll
    for (int o = 0; o < 6; ++o) ky[o] = S.tap[0][0][o];
#pragma unroll
    for (int k = 0; k < RG_ITEMS; ++k) {
        if (th.y0[k] < 0) continue;
        float t[RG_RUN];
        const unsigned c = column_run(l.A, l.pat, ky, ny, nx, table, th.x[k], th.y0[k], H, W, t);
#pragma unroll
        for (int p = 0; p < RG_RUN; ++p) {
            const int y = th.y0[k] + p;
            if (y >= H) break;
            const bool on = (c >> p) & 1u;
            const size_t i = view * hw + (size_t)y * W + th.x[k];
            out[i] = on ? t[p] : 0.f;
            out_valid[i] = on ? 1.f : 0.f;
        }
    }
}

}  // namespace

int hrn_launch_mncc_grid(const float* ref, const float* ref_mask, const float* views, const float* view_masks, const float* centres, int B,
                         int V, int H, int W, int P, float width, float* scores, hipStream_t stream) {
    const int lds = (int)lds_bytes(H, W);
    if (int rc = hrn_allow_lds((const void*)mncc_kernel, (int)lds_bytes(RG_MAX, RG_MAX))) return rc;
    HrnProfScope prof("mncc_grid", level_flops(P) * B * V * H * W, 4.0 * B * V * (2.0 * H * W + P * P), stream);
    hipLaunchKernelGGL(mncc_kernel, dim3((unsigned)(B * V)), dim3(RG_THREADS), lds, stream, ref, ref_mask, views, view_masks, centres, V, H, W, P,
                       0, width, 0.0, scores, (float*)nullptr, (float*)nullptr);
    HRN_LAUNCH_CHECK();
    return 0;
}

int hrn_launch_mncc_search(const float* ref, const float* ref_mask, const float* views, const float* view_masks, int B, int V, int H, int W,
                           int P, int levels, float radius, float* shifts, float* trace, hipStream_t stream) {
    const int lds = (int)lds_bytes(H, W);
    if (int rc = hrn_allow_lds((const void*)mncc_kernel, (int)lds_bytes(RG_MAX, RG_MAX))) return rc;
    HrnProfScope prof("mncc_search", level_flops(P) * levels * B * V * H * W, 4.0 * B * V * (2.0 * H * W + 2 + 3 * levels), stream);
    hipLaunchKernelGGL(mncc_kernel, dim3((unsigned)(B * V)), dim3(RG_THREADS), lds, stream, ref, ref_mask, views, view_masks,
                       (const float*)nullptr, V, H, W, P, levels, 2.f * radius, level_ratio(P), (float*)nullptr, shifts, trace);
    HRN_LAUNCH_CHECK();
    return 0;
}

int hrn_launch_mncc_apply(const float* views, const float* view_masks, const float* shifts, int B, int V, int H, int W, float* out,
                          float* out_valid, hipStream_t stream) {
    const int lds = (int)lds_bytes(H, W);
    if (int rc = hrn_allow_lds((const void*)mncc_apply_kernel, (int)lds_bytes(RG_MAX, RG_MAX))) return rc;
    HrnProfScope prof("mncc_apply", 2.0 * 12.0 * B * V * H * W, 4.0 * B * V * (4.0 * H * W + 2), stream);
    hipLaunchKernelGGL(mncc_apply_kernel, dim3((unsigned)(B * V)), dim3(RG_THREADS), lds, stream, views, view_masks, shifts, H, W, out, out_valid);
    HRN_LAUNCH_CHECK();
    return 0;
}
