// Decoder backward (HRNet.py:147-156,167-169): sr = conv1x1(PReLU(ConvTranspose kS sS (fused))), S in {2, 3, 4}.
// Per LR pixel p and the S^2 positions pos = (ky, kx) of its S x S output patch:
//     up[co][pos] = bd[co] + sum_ci F[p][ci] Wd[ci][co][pos];  y = PReLU(up);  sr[pos] = bf + sum_co wf[co] y[co][pos]
//     dy = wf[co] dsr[pos];  dup = dy PReLU'(up);  dF[p][ci] = sum_{co,pos} Wd[ci][co][pos] dup[co][pos]
//     dWd[ci][co][pos] += F[p][ci] dup[co][pos];  dbd[co] += sum_pos dup;  dad += sum dy min(up, 0);  dwf[co] += sum_pos y dsr;  dbf += sum dsr
// The forward never stores `up` (1.1 GiB at the bench size), so it is recomputed here.  One persistent 256-thread workgroup
// per CU: lane = co, wave = a quarter of the input channels (16 ci), whose 16 NP weights and 16 NP weight-gradient sums stay in
// registers for the whole launch, NP = the positions one launch covers.  S = 2, 3: all S^2 positions in one launch (NP = 4, 9).
// S = 4: 2 x 16 x 16 floats per lane would not fit (weights and sums of all 64 x 64 x 16 taps fill a CU's whole register file),
// so two launches cover rows 0-1 and rows 2-3 (NP = 8); the second adds its part of d_fused and of the slab's small gradients
// to what the first wrote.  Deterministic: per-workgroup partial slabs + a fixed-order finish.
#include "backward.h"

namespace {

constexpr int db_dw(int S) { return 64 * 64 * S * S; }
constexpr int db_slab(int S) { return db_dw(S) + 64 + 64 + 64 + 64; }     // dWd | dbd[64] | dwf[64] | dad per lane[64] | dbf (+ pad)
constexpr int db_npos(int S) { return S == 4 ? 8 : S * S; }               // positions per launch

// positions pos0 .. pos0 + NP - 1 (row-major in the S x S patch); pos0 > 0: a later launch, which accumulates
template <int S, int NP>
__global__ __launch_bounds__(256, 1) void decoder_bwd_kernel(const float* __restrict__ fused, const float* __restrict__ d_sr,
                                                             const float* __restrict__ wd, const float* __restrict__ bd,
                                                             const float* __restrict__ ad, const float* __restrict__ wf,
                                                             float* __restrict__ d_fused, float* __restrict__ partial, int N, int H, int W,
                                                             int pos0_arg) {
    constexpr int SS = S * S, DB_DW = db_dw(S), DB_SLAB = db_slab(S);
    const int pos0 = NP == SS ? 0 : pos0_arg;
    const bool later = pos0 != 0;
    __shared__ float upp[2][4][64][NP];
    __shared__ float part[4][64][17];
    const int tid = threadIdx.x, co = tid & 63, cig = tid >> 6;
    float wreg[16][NP], acc[16][NP];
#pragma unroll
    for (int k = 0; k < 16; ++k)
#pragma unroll
        for (int pos = 0; pos < NP; ++pos) {
            wreg[k][pos] = wd[((size_t)(16 * cig + k) * 64 + co) * SS + pos0 + pos];
            acc[k][pos] = 0.f;
        }
    const float bdc = bd[co], wfc = wf[co], a = ad[0];
    float a_dbd = 0.f, a_dwf = 0.f, a_dad = 0.f, a_dbf = 0.f;
    const long hw = (long)H * W, P = hw * N;
    const int WS = S * W;
    int it = 0;
    for (long p = blockIdx.x; p < P; p += gridDim.x, ++it) {
        const long n = p / hw, rem = p - n * hw;
        const int y = (int)(rem / W), x = (int)(rem - (long)y * W);
        float f[16], ds[NP], up[NP], dup[NP];
#pragma unroll
        for (int k = 0; k < 16; ++k) f[k] = fused[(size_t)p * 64 + 16 * cig + k];
        const float* dp = d_sr + ((size_t)n * S * H + S * y + pos0 / S) * WS + S * x;
#pragma unroll
        for (int pos = 0; pos < NP; ++pos) ds[pos] = dp[(size_t)(pos / S) * WS + pos % S];
#pragma unroll
        for (int pos = 0; pos < NP; ++pos) {
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < 16; ++k) s += f[k] * wreg[k][pos];
            upp[it & 1][cig][co][pos] = s;
        }
        __syncthreads();
#pragma unroll
        for (int pos = 0; pos < NP; ++pos) {
            const float u = bdc + ((upp[it & 1][0][co][pos] + upp[it & 1][1][co][pos]) + (upp[it & 1][2][co][pos] + upp[it & 1][3][co][pos]));
            up[pos] = u;
            const float dy = wfc * ds[pos];
            dup[pos] = u > 0.f ? dy : a * dy;
            if (cig == 0) {
                a_dwf += (u > 0.f ? u : a * u) * ds[pos];
                a_dbd += dup[pos];
                a_dad += u > 0.f ? 0.f : dy * u;
                if (co == 0) a_dbf += ds[pos];
            }
        }
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            float s = 0.f;
#pragma unroll
            for (int pos = 0; pos < NP; ++pos) {
                acc[k][pos] += f[k] * dup[pos];
                s += wreg[k][pos] * dup[pos];
            }
            part[cig][co][k] = s;
        }
        // dF[p][16 cig + k] = sum over co of part[cig][co][k]: lane (sub, k) sums 16 couts, then two cross-lane adds
        __builtin_amdgcn_wave_barrier();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        {
            const int k = co & 15, sub = co >> 4;
            float s = 0.f;
#pragma unroll
            for (int c = 0; c < 16; ++c) s += part[cig][16 * sub + c][k];
            s += __shfl_xor(s, 16);
            s += __shfl_xor(s, 32);
            if (co < 16) {
                float* d = d_fused + (size_t)p * 64 + 16 * cig + k;
                *d = later ? *d + s : s;
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
    float* out = partial + (size_t)blockIdx.x * DB_SLAB;
#pragma unroll
    for (int k = 0; k < 16; ++k)
#pragma unroll
        for (int pos = 0; pos < NP; ++pos) out[((size_t)(16 * cig + k) * 64 + co) * SS + pos0 + pos] = acc[k][pos];
    if (cig == 0) {
        if (later) {
            a_dbd += out[DB_DW + co];
            a_dwf += out[DB_DW + 64 + co];
            a_dad += out[DB_DW + 128 + co];
            a_dbf += out[DB_DW + 192 + co];
        }
        out[DB_DW + co] = a_dbd;
        out[DB_DW + 64 + co] = a_dwf;
        out[DB_DW + 128 + co] = a_dad;
        out[DB_DW + 192 + co] = co == 0 ? a_dbf : 0.f;
    }
}

// blocks 0 .. (DB_DW + 128) / 64 - 1: 64 consecutive elements x 16 slab phases; the last two blocks: the two scalars (slope, final
// bias), whose 64 per-lane terms per slab are summed by 64 x 16 threads as well.  Fixed order throughout.
template <int S>
__global__ __launch_bounds__(1024) void decoder_bwd_finish_kernel(const float* __restrict__ partial, int nblk, float* __restrict__ dwd,
                                                                  float* __restrict__ dbd, float* __restrict__ dad, float* __restrict__ dwf,
                                                                  float* __restrict__ dbf) {
    constexpr int DB_DW = db_dw(S), DB_SLAB = db_slab(S);
    __shared__ double red[16][64];
    const int el = threadIdx.x & 63, ph = threadIdx.x >> 6;
    constexpr int NEB = (DB_DW + 128) / 64;
    const bool scalar = (int)blockIdx.x >= NEB;
    const int idx = scalar ? (blockIdx.x == NEB ? DB_DW + 128 : DB_DW + 192) + el : blockIdx.x * 64 + el;
    double s = 0.0;
#pragma unroll 4
    for (int b = ph; b < nblk; b += 16) s += (double)partial[(size_t)b * DB_SLAB + idx];
    red[ph][el] = s;
    __syncthreads();
    if (ph != 0) return;
    s = 0.0;
#pragma unroll
    for (int k = 0; k < 16; ++k) s += red[k][el];
    // a NULL output: a frozen parameter (hrn_hrnet_backward_sel), whose sum nobody reads
    if (!scalar) {
        if (idx < DB_DW) { if (dwd) dwd[idx] += (float)s; }
        else if (idx < DB_DW + 64) { if (dbd) dbd[idx - DB_DW] += (float)s; }
        else if (dwf) dwf[idx - DB_DW - 64] += (float)s;
        return;
    }
    // the 64 lane terms of a scalar: one wave, fixed order
    red[0][el] = s;                                         // (one wave is left: its LDS accesses are ordered)
    if (el == 0) {
        double t = 0.0;
        for (int l = 0; l < 64; ++l) t += red[0][l];
        if ((int)blockIdx.x == NEB) { if (dad) dad[0] += (float)t; }
        else if (dbf) dbf[0] += (float)t;
    }
}

template <int S>
int launch_decoder_bwd(const float* fused, const float* d_sr, const float* wd, const float* bd, const float* ad, const float* wf, float* d_fused,
                       float* dwd, float* dbd, float* dad, float* dwf, float* dbf, int N, int H, int W, void* scratch, int grid, hipStream_t s) {
    constexpr int NP = db_npos(S), DB_DW = db_dw(S);
    static_assert(S * S % NP == 0 && NP % S == 0, "decoder_bwd: a launch covers whole rows");
    for (int pos0 = 0; pos0 < S * S; pos0 += NP) {
        hipLaunchKernelGGL((decoder_bwd_kernel<S, NP>), dim3(grid), dim3(256), 0, s, fused, d_sr, wd, bd, ad, wf, d_fused, (float*)scratch, N, H,
                           W, pos0);
        hrn_count_launch(HRN_LC_DECODER_BWD);
    }
    static_assert((DB_DW + 128) % 64 == 0, "decoder_bwd_finish: 64 elements per block");
    // every decoder parameter frozen (hrn_hrnet_backward_sel): the partial slabs have no reader
    if (dwd || dbd || dad || dwf || dbf) {
        hipLaunchKernelGGL(decoder_bwd_finish_kernel<S>, dim3((DB_DW + 128) / 64 + 2), dim3(1024), 0, s, (const float*)scratch, grid, dwd, dbd,
                           dad, dwf, dbf);
        hrn_count_launch(HRN_LC_DECODER_BWD_FINISH);
    }
    HRN_LAUNCH_CHECK();
    return 0;
}

}  // namespace

size_t hrn_decoder_bwd_scratch_bytes(int num_cus, int scale) {
    return hrn_scale_ok(scale) ? (size_t)num_cus * db_slab(scale) * 4 : 0;
}

int hrn_launch_decoder_bwd(const float* fused, const float* d_sr, const float* wd, const float* bd, const float* ad, const float* wf,
                           float* d_fused, float* dwd, float* dbd, float* dad, float* dwf, float* dbf, int N, int H, int W,
                           void* scratch, int num_cus, hipStream_t s, int scale) {
    HRN_CHECK(hrn_scale_ok(scale), -2, "decoder_bwd: scale must be 2, 3 or 4 (got %d)", scale);
    const long P = (long)N * H * W;
    int grid = num_cus;
    if (P < grid) grid = (int)P;
    return hrn_by_scale(scale, [&](auto sc) {
        return launch_decoder_bwd<decltype(sc)::value>(fused, d_sr, wd, bd, ad, wf, d_fused, dwd, dbd, dad, dwf, dbf, N, H, W, scratch, grid, s);
    });
}
