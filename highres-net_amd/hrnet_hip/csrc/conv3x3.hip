// conv3x3 (pad 1, stride 1) + bias + PReLU + residual as an implicit GEMM on the gfx950 matrix cores.
//
// Replaces every nn.Conv2d(k=3) of the reference hot path:
//   /root/reference/src/DeepNetworks/HRNet.py:17-22 (ResidualBlock), :51-60 (Encoder), :93-97 (fuse)
//   /root/reference/src/DeepNetworks/ShiftNet.py:19-42 (layers 2..8)
// including the data movement the reference materialises around them (slice / flip / cat of the view
// stack, HRNet.py:114-119; residual add :33; alpha residual :123-128).
//
// GEMM view (per image):  D[cout][pixel] = sum_k  Wt[cout][k] * X[k][pixel],  k = (tap, cin)
//   A operand = weights  (rows = output channels),  B operand = activations (cols = pixels)
//   -> each lane ends up with 4 consecutive output channels of ONE pixel per accumulator quad, which is the
//      NHWC store order (8 B for bf16, 16 B for f32 per store).
//
// Workgroup = 4 waves per 64 output channels (COUT=64: 256 threads, 2 workgroups/CU; COUT=128: 512 threads, 1/CU, so
// both cout halves share ONE staged input tile); output tile 8 rows x 32 cols x COUT; wave (half, w) owns tile rows
// 2w, 2w+1 (two 32-pixel column blocks) x 64 output channels -> 64 accumulator registers, 2 waves per SIMD.
// LDS: input halo tile [10][34] pixels x 128 B of channels (+16 B pad per pixel: conflict-free ds_read_b128),
//      two weight slices [COUT][128 B of K] (+16 B pad per row), double buffered.  67,392 / 85,824 B.
// K is walked in "steps": (channel chunk of 128 B) x (tap); per step a wave issues
//   bf16: 4 k-steps  x 4 MFMA 32x32x16   |  f32: 4 groups x 4 x 4 MFMA 32x32x2 (exact fp32, k-order permuted
//   identically for A and B: lane half hh supplies channel 8q+4hh+j at MFMA j of group q).
//
// Schedule (v2, from the r01 ablation: MFMA time was ~20-45 % of the launch, the rest un-overlapped staging, stores and
// the dispatch of 65k workgroups): PERSISTENT workgroups, 2 per CU, walk the tile list in windows of gridDim.x tiles;
// inside a window the 8 XCDs own contiguous runs of tiles (blocks b and b+8 share an XCD), so the halo rows of
// neighbouring tiles are in flight on the same L2 at the same time.  While a tile is computed, the next tile's (or
// next channel chunk's) halo input is already on its way from HBM into 11 staging registers per lane; it is written
// to the single LDS tile after the last MFMA step's barrier, and the epilogue's stores drain under the next tile.
#include "conv3x3.h"
#include <stdlib.h>


namespace {

constexpr int HALO_H = CONV_TILE_H + 2;
constexpr int HALO_W = CONV_TILE_W + 2;
constexpr int PIX_PITCH = 144;
constexpr int IN_LDS_BYTES = HALO_H * HALO_W * PIX_PITCH;   // 48,960
constexpr int W_ROW_PITCH = 144;
constexpr int N_IN_CHUNKS16 = HALO_H * HALO_W * 8;          // 2,720 16-byte pieces

struct TileCtx {
    int m, y0, x0;
    const unsigned char* src0;      // pair descriptor: view i ...
    const unsigned char* src1;      // ... and its partner in the stack
    const unsigned char* in_plain;  // plain input image
};

template <int DT, int CIN, int COUT>
__global__ __launch_bounds__(256 * (COUT / 64), 2) void conv3x3_kernel(const ConvParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* in_lds = smem;
    unsigned char* w_lds = smem + IN_LDS_BYTES;

    constexpr int ES = ElemOf<DT>::size;
    constexpr int KB = 128 / ES;            // channels per 128-byte chunk
    constexpr int NCHUNK = CIN / KB;
    constexpr int NHALF = COUT / 64;
    constexpr int NT = 256 * NHALF;                         // threads per workgroup
    constexpr int NSTEP = NCHUNK * 9;
    constexpr int W_BUF_BYTES = COUT * W_ROW_PITCH;         // one weight slice: [COUT][128 B of K], padded rows
    constexpr int N_IN_ITERS = (N_IN_CHUNKS16 + NT - 1) / NT;

    if (p.only_if_nonpos && p.only_if_nonpos[0] > 0.f) return;          // uniform: before any barrier
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = (tid >> 6) & 3, half = tid >> 8;    // half: which 64 output channels
    const int r = lane & 31, hh = lane >> 5;
    const int H = p.H, W = p.W;
    const size_t hw = (size_t)H * W;
    const int tiles_x = (W + CONV_TILE_W - 1) / CONV_TILE_W;
    const int tiles_y = (H + CONV_TILE_H - 1) / CONV_TILE_H;
    const int tiles = tiles_x * tiles_y;
    const long total = (long)tiles * p.M;

    // ---- persistent tile walk: window `it` covers tiles [it*G, (it+1)*G); inside it XCD x owns a contiguous run
    const int G = gridDim.x;
    const int bid = blockIdx.x;
    const int slot = (G & 7) == 0 ? (bid & 7) * (G >> 3) + (bid >> 3) : bid;
    long tile = slot;
    if (tile >= total) return;

    const bool in_pair = p.in_pair != 0;
    const int in_pix_bytes = in_pair ? 64 * ES : CIN * ES;

    auto make_tile = [&](long tl) {
        TileCtx c;
        c.m = (int)(tl / tiles);
        const int t = (int)(tl - (long)c.m * tiles);
        const int ty = t / tiles_x;
        c.y0 = ty * CONV_TILE_H;
        c.x0 = (t - ty * tiles_x) * CONV_TILE_W;
        c.src0 = c.src1 = nullptr;
        if (p.pair_h > 0) {
            const int b = c.m / p.pair_h, i = c.m - b * p.pair_h;
            c.src0 = (const unsigned char*)p.stack + ((size_t)b * p.pair_vs + i) * hw * 64 * ES;
            c.src1 = (const unsigned char*)p.stack + ((size_t)b * p.pair_vs + (p.pair_last - i)) * hw * 64 * ES;
        }
        c.in_plain = (const unsigned char*)p.in + (size_t)c.m * hw * CIN * ES;
        return c;
    };

    uint4 inreg[N_IN_ITERS];
    // global -> staging registers (zero fill outside the image == the conv's zero padding)
    auto issue_input = [&](const TileCtx& c, int chunk) {
        const unsigned char* base;
        int choff;
        if (in_pair) {
            const int ch0 = chunk * KB;                 // first channel of this chunk in the virtual 128-ch input
            base = ch0 < 64 ? c.src0 : c.src1;
            choff = (ch0 & 63) * ES;
        } else {
            base = c.in_plain;
            choff = chunk * 128;
        }
#pragma unroll
        for (int it = 0; it < N_IN_ITERS; ++it) {
            const int cc = tid + it * NT;
            const int pix = cc >> 3, part = cc & 7;
            const int py = pix / HALO_W, px = pix - py * HALO_W;
            const int gy = c.y0 + py - 1, gx = c.x0 + px - 1;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (cc < N_IN_CHUNKS16 && (unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W)
                v = *(const uint4*)(base + ((size_t)gy * W + gx) * in_pix_bytes + choff + part * 16);
            inreg[it] = v;
        }
    };
    // staging registers -> LDS tile
    auto commit_input = [&]() {
#pragma unroll
        for (int it = 0; it < N_IN_ITERS; ++it) {
            const int cc = tid + it * NT;
            if (cc < N_IN_CHUNKS16) *(uint4*)(in_lds + (cc >> 3) * PIX_PITCH + (cc & 7) * 16) = inreg[it];
        }
    };

    const uint4* wg = (const uint4*)p.wpk;
    const int w_dst0 = (tid >> 3) * W_ROW_PITCH + (tid & 7) * 16;
    const int w_dst1 = w_dst0 + (NT / 8) * W_ROW_PITCH;
    const unsigned char* a_base = w_lds + (half * 64 + r) * W_ROW_PITCH + hh * 16;                 // + buf, + cb*32 rows
    const unsigned char* b_base = in_lds + ((2 * wave) * HALO_W + r) * PIX_PITCH + hh * 16;        // + tap, + pb row

    const bool has_slope = p.slope != nullptr;
    const float slope = has_slope ? p.slope[0] : 0.f;

    // ---- prologue: first tile's chunk 0 + weight slice 0
    TileCtx cur = make_tile(tile);
    issue_input(cur, 0);
    commit_input();
    {
        const uint4 w0 = wg[tid], w1 = wg[tid + NT];
        *(uint4*)(w_lds + w_dst0) = w0;
        *(uint4*)(w_lds + w_dst1) = w1;
    }
    __syncthreads();

    int gstep = 0;      // running step count: parity selects the weight buffer (NSTEP may be odd)
    for (;;) {
        const long ntile = tile + G;
        const bool has_next_tile = ntile < total;
        const TileCtx nxt = has_next_tile ? make_tile(ntile) : cur;

        f32x16 acc[2][2];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;

#pragma unroll 1
        for (int chunk = 0; chunk < NCHUNK; ++chunk) {
            const bool last_chunk = chunk == NCHUNK - 1;
            const bool has_next = !last_chunk || has_next_tile;
            if (has_next) {     // next halo tile: in flight during this chunk's MFMA steps
                if (last_chunk) issue_input(nxt, 0); else issue_input(cur, chunk + 1);
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const int ky = tap / 3, kx = tap - ky * 3;
                const unsigned char* xb = b_base + (ky * HALO_W + kx) * PIX_PITCH;
                {
                    const int s = chunk * 9 + tap;
                    const bool last_step = s == NSTEP - 1;
                    const bool more = !last_step || has_next_tile;
                    uint4 w0, w1;
                    if (more) {         // prefetch the next weight slice into registers
                        const size_t ns = last_step ? 0 : (size_t)(s + 1);
                        w0 = wg[ns * (2 * NT) + tid];
                        w1 = wg[ns * (2 * NT) + tid + NT];
                        // keep the loads HERE: without the fence hipcc sinks them to their first use (the ds_write at the
                        // end of the step) and every step then pays an L2 round trip in front of its barrier
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    const unsigned char* wb = a_base + (gstep & 1) * W_BUF_BYTES;
                    if constexpr (DT == HRN_BF16) {
                        // all 16 fragment reads of the step go out back to back (one LDS round trip per step instead of
                        // one per k-step: hipcc otherwise waits on each k-step's reads right before its MFMAs), then the
                        // 16 MFMAs drain them under counted lgkmcnt waits
                        // (the 256-thread variants keep 44 staging registers alive, so they batch 2 k-steps at a time)
                        constexpr int KBATCH = NT == 512 ? 4 : 2;
#pragma unroll
                        for (int k0 = 0; k0 < 4; k0 += KBATCH) {
                            bf16x8 a0[KBATCH], a1[KBATCH], b0[KBATCH], b1[KBATCH];
#pragma unroll
                            for (int ks = 0; ks < KBATCH; ++ks) {
                                a0[ks] = *(const bf16x8*)(wb + (k0 + ks) * 32);
                                b0[ks] = *(const bf16x8*)(xb + (k0 + ks) * 32);
                                a1[ks] = *(const bf16x8*)(wb + 32 * W_ROW_PITCH + (k0 + ks) * 32);
                                b1[ks] = *(const bf16x8*)(xb + HALO_W * PIX_PITCH + (k0 + ks) * 32);
                            }
                            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                            for (int ks = 0; ks < KBATCH; ++ks) {
                                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0[ks], b0[ks], acc[0][0], 0, 0, 0);
                                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1[ks], b0[ks], acc[0][1], 0, 0, 0);
                                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0[ks], b1[ks], acc[1][0], 0, 0, 0);
                                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1[ks], b1[ks], acc[1][1], 0, 0, 0);
                            }
                        }
                    } else {
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const f32x4 a0 = *(const f32x4*)(wb + q * 32);
                            const f32x4 a1 = *(const f32x4*)(wb + 32 * W_ROW_PITCH + q * 32);
                            const f32x4 b0 = *(const f32x4*)(xb + q * 32);
                            const f32x4 b1 = *(const f32x4*)(xb + HALO_W * PIX_PITCH + q * 32);
#pragma unroll
                            for (int j = 0; j < 4; ++j) {
                                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[j], b0[j], acc[0][0], 0, 0, 0);
                                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[j], b0[j], acc[0][1], 0, 0, 0);
                                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[j], b1[j], acc[1][0], 0, 0, 0);
                                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[j], b1[j], acc[1][1], 0, 0, 0);
                            }
                        }
                    }
                    if (more) {         // the other buffer was last read in the previous step, which ended with a barrier
                        unsigned char* wd = w_lds + ((gstep + 1) & 1) * W_BUF_BYTES;
                        *(uint4*)(wd + w_dst0) = w0;
                        *(uint4*)(wd + w_dst1) = w1;
                    }
                    __syncthreads();
                    ++gstep;
                }
            }
            // every wave has passed the last step's barrier: nobody reads the LDS tile any more
            if (has_next) commit_input();
            if (!last_chunk) __syncthreads();
        }

        // ---- epilogue: scale/bias, PReLU/ReLU, residual, NHWC store (4 consecutive channels per lane and quad)
        {
            const int m = cur.m;
            size_t out_img;
            float alpha = 1.f;
            const unsigned char* res3 = nullptr;
            if (p.out_h > 0) {
                const int b = m / p.out_h, i = m - b * p.out_h;
                out_img = (size_t)b * p.out_vs + i;
                if (p.res_mode == 3) {
                    if (p.alphas) alpha = p.alphas[(size_t)b * p.alpha_vs + (p.pair_last - i)];
                    res3 = (const unsigned char*)p.res + ((size_t)b * p.res_vs + i) * hw * COUT * ES;
                }
            } else {
                out_img = (size_t)m;
            }
            unsigned char* outp = (unsigned char*)p.out + out_img * hw * COUT * ES;
            const int gx = cur.x0 + r;
#pragma unroll
            for (int pb = 0; pb < 2; ++pb) {
                const int gy = cur.y0 + 2 * wave + pb;
                if (gy >= H || gx >= W) continue;
                const size_t pix = (size_t)gy * W + gx;
                {
#pragma unroll
                    for (int cb = 0; cb < 2; ++cb) {
#pragma unroll
                        for (int g = 0; g < 4; ++g) {
                            const int co = half * 64 + cb * 32 + 8 * g + 4 * hh;
                            f32x4 v;
#pragma unroll
                            for (int j = 0; j < 4; ++j) v[j] = acc[pb][cb][4 * g + j];
                            if (p.scale) {
                                const f32x4 sc = *(const f32x4*)(p.scale + co);
                                v *= sc;
                            }
                            v += *(const f32x4*)(p.bias + co);
                            if (has_slope) {
#pragma unroll
                                for (int j = 0; j < 4; ++j) v[j] = v[j] >= 0.f ? v[j] : slope * v[j];
                            }
                            if (p.relu) {
#pragma unroll
                                for (int j = 0; j < 4; ++j) v[j] = fmaxf(v[j], 0.f);
                            }
                            if (p.res_mode == 1) {
                                v += load4<DT>((const unsigned char*)p.res + (size_t)m * hw * COUT * ES, pix * COUT + co);
                            } else if (p.res_mode == 2) {   // pair gather: channels 0..63 = view i, 64..127 = its partner
                                v += load4<DT>(half == 0 ? cur.src0 : cur.src1, pix * 64 + (co & 63));
                            } else if (p.res_mode == 3) {   // x_i + alpha_partner * f   (HRNet.py:127); may be in place
                                v = load4<DT>(res3, pix * COUT + co) + alpha * v;
                            }
                            store4<DT>(outp, pix * COUT + co, v);
                        }
                    }
                }
            }
        }
        if (!has_next_tile) break;
        __syncthreads();        // next tile's input (committed above) becomes visible to every wave
        tile = ntile;
        cur = nxt;
    }
}


template <int DT, int CIN, int COUT>
int launch(const ConvParams& p, long grid, hipStream_t stream) {
    constexpr int LDS_BYTES = IN_LDS_BYTES + 2 * COUT * W_ROW_PITCH;
    { const int rc_lds = hrn_allow_lds((const void*)conv3x3_kernel<DT, CIN, COUT>, LDS_BYTES); if (rc_lds) return rc_lds; }
    hipLaunchKernelGGL((conv3x3_kernel<DT, CIN, COUT>), dim3((unsigned)grid), dim3(256 * (COUT / 64)), LDS_BYTES, stream, p);
    hrn_count_launch(HRN_LC_CONV_GENERAL);
    HRN_LAUNCH_CHECK();
    return 0;
}

// The general kernel's instances, [dt][cin / 128][cout / 128].  Each takes any res_mode and either input, and files a residual layer under
// the plain name: a row's res_mode / in_pair say nothing.
#define ROW(DT_, TAG_, CI_, CO_) {CI_, CO_, 0, 0, "conv3x3_" TAG_ "_" #CI_ "x" #CO_, launch<DT_, CI_, CO_>}
const ConvInstance GENERAL_ROWS[2][2][2] = {
    {{ROW(HRN_F32, "f32", 64, 64), ROW(HRN_F32, "f32", 64, 128)}, {ROW(HRN_F32, "f32", 128, 64), ROW(HRN_F32, "f32", 128, 128)}},
    {{ROW(HRN_BF16, "bf16", 64, 64), ROW(HRN_BF16, "bf16", 64, 128)}, {ROW(HRN_BF16, "bf16", 128, 64), ROW(HRN_BF16, "bf16", 128, 128)}}};
#undef ROW

// ---- weight packing: OIHW f32 -> [step][64 cout][128 B of K], step = (chunk*9 + tap)*NHALF + half
template <int DT>
__global__ void conv_pack_kernel(const float* __restrict__ w, void* __restrict__ out, int cin, int cout) {
    constexpr int ES = ElemOf<DT>::size;
    constexpr int KB = 128 / ES;
    const int nhalf = cout / 64;
    const size_t total = (size_t)cin * cout * 9;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int kk = (int)(idx % KB);
        const int col = (int)((idx / KB) % 64);
        const int step = (int)(idx / ((size_t)KB * 64));
        const int half = step % nhalf;
        const int ct = step / nhalf;
        const int tap = ct % 9, chunk = ct / 9;
        const int co = half * 64 + col, ci = chunk * KB + kk;
        const float v = w[((size_t)co * cin + ci) * 9 + tap];
        store_elem<DT>(out, idx, v);
    }
}

// bf16x3: the bf16 layout twice - plane 0 holds hi = bf16(w), plane 1 (total elements further on) lo = bf16(w - hi)
__global__ void conv_pack_x3_kernel(const float* __restrict__ w, unsigned short* __restrict__ out, int cin, int cout) {
    constexpr int KB = 64;
    const int nhalf = cout / 64;
    const size_t total = (size_t)cin * cout * 9;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int kk = (int)(idx % KB);
        const int col = (int)((idx / KB) % 64);
        const int step = (int)(idx / ((size_t)KB * 64));
        const int half = step % nhalf;
        const int ct = step / nhalf;
        const int tap = ct % 9, chunk = ct / 9;
        const int co = half * 64 + col, ci = chunk * KB + kk;
        const float v = w[((size_t)co * cin + ci) * 9 + tap];
        const unsigned short h = f32_to_bf16_bits(v);
        out[idx] = h;
        out[total + idx] = f32_to_bf16_bits(v - bf16_bits_to_f32(h));
    }
}

// the descriptor contract of conv3x3.h
int check_descriptor(int dt, int cin, int cout, const ConvParams& p, bool general_only) {
    HRN_CHECK((dt == HRN_F32 || dt == HRN_BF16 || dt == HRN_BF16X3) && (cin == 64 || cin == 128) && (cout == 64 || cout == 128), -2,
              "conv3x3: unsupported dtype/channels dt=%d cin=%d cout=%d", dt, cin, cout);
    HRN_CHECK(p.M > 0 && p.H > 0 && p.W > 0, -2, "conv3x3: empty problem M=%d H=%d W=%d", p.M, p.H, p.W);
    HRN_CHECK(p.wpk && p.bias && p.out, -2, "conv3x3: null %s", !p.wpk ? "wpk" : !p.bias ? "bias" : "out");
    HRN_CHECK(p.in_pair || p.in, -2, "conv3x3: null in without in_pair");
    HRN_CHECK(p.res_mode >= 0 && p.res_mode <= 3, -2, "conv3x3: res_mode %d not in 0..3", p.res_mode);
    HRN_CHECK(!p.in_pair || cin == 128, -2, "conv3x3: in_pair needs cin=128, not %d", cin);
    HRN_CHECK(p.res_mode != 2 || cout == 128, -2, "conv3x3: res_mode 2 needs cout=128, not %d", cout);
    HRN_CHECK(!(p.in_pair || p.res_mode == 2) ||
                  (p.stack && p.pair_h > 0 && p.M % p.pair_h == 0 && p.pair_h - 1 <= p.pair_last && p.pair_last < p.pair_vs), -2,
              "conv3x3: the pair gather needs stack, pair_h > 0 dividing M and pair_h - 1 <= pair_last < pair_vs (stack=%p pair_h=%d M=%d "
              "pair_last=%d pair_vs=%d)", p.stack, p.pair_h, p.M, p.pair_last, p.pair_vs);
    HRN_CHECK(p.res_mode != 1 || p.res, -2, "conv3x3: res_mode 1 needs res");
    HRN_CHECK(p.res_mode != 3 || (p.res && p.out_h > 0 && p.res_vs >= p.out_h), -2,
              "conv3x3: res_mode 3 needs res, slot output and res_vs >= out_h (res=%p out_h=%d res_vs=%d)", p.res, p.out_h, p.res_vs);
    HRN_CHECK(p.res_mode != 3 || !p.alphas || (p.out_h - 1 <= p.pair_last && p.pair_last < p.alpha_vs), -2,
              "conv3x3: alphas need out_h - 1 <= pair_last < alpha_vs (out_h=%d pair_last=%d alpha_vs=%d)", p.out_h, p.pair_last, p.alpha_vs);
    HRN_CHECK(p.out_h <= 0 || (p.M % p.out_h == 0 && p.out_vs >= p.out_h), -2,
              "conv3x3: slot output needs out_h dividing M and out_vs >= out_h (out_h=%d M=%d out_vs=%d)", p.out_h, p.M, p.out_vs);
    if (dt != HRN_BF16X3) return 0;
    HRN_CHECK(!general_only, -2, "conv3x3: bf16x3 has no general kernel");
    HRN_CHECK(!p.scale && !p.relu, -2, "conv3x3 bf16x3: folded scale / relu are not supported");
    HRN_CHECK(p.out_lo != 0 && (p.in_pair ? p.stack_lo : p.in_lo) != 0, -2, "conv3x3 bf16x3: lo-plane offsets missing (out_lo / %s)",
              p.in_pair ? "stack_lo" : "in_lo");
    return 0;
}

long tile_count(const ConvParams& p, int th, int tw) { return (long)((p.W + tw - 1) / tw) * ((p.H + th - 1) / th) * p.M; }    // of the whole launch

// The route of `row` on th x tw tiles.  The grid is persistent: one round of wg_per_cu workgroups per CU, at most one per tile, and a
// multiple of 8 so that the windows split evenly over the 8 XCDs.  The profiler's cost: algorithmic FLOPs, bytes of every plane.
ConvRoute route_of(int family, const ConvInstance& row, int th, int tw, int es, int wg_per_cu, const ConvParams& p) {
    long grid = (long)wg_per_cu * hrn_device_cus();
    if (tile_count(p, th, tw) < grid) grid = tile_count(p, th, tw);
    if (grid >= 8) grid &= ~7L;
    const double px = (double)p.M * p.H * p.W;
    return ConvRoute{family, row.name, th, tw, grid, 2.0 * row.cin * row.cout * 9 * px, px * es * (row.cin + row.cout + (p.res_mode ? row.cout : 0)),
                     row.launch};
}

// A fast family's whole rule: the row of its table that matches the layer, if the image fits its 32-bit arithmetic; else it declines - for
// shape and size only, never a malformed descriptor.  The fast kernels count tiles and in-image bytes in 32 bits: the tile total must stay
// below 2^30, and ONE image of the wider of input and output (2 bytes per channel and pixel; the plain residual is as wide as the output)
// below 2^31 bytes - 16.7 Mpixel at 64 channels, 8.3 Mpixel at 128.  (v6 marks an out-of-image lane with bit 31 of its offset, which
// only a buffer descriptor of fewer than 2^31 bytes drops.)
enum ConvDecline { CONV_NO_INSTANCE = 1, CONV_TOO_LARGE = 2 };
int route_fast(const ConvTable& t, int cin, int cout, const ConvParams& p, ConvRoute& r) {
    for (const ConvInstance* row = t.rows; row < t.rows + t.nrows; ++row) {
        if (row->cin != cin || row->cout != cout || row->res_mode != p.res_mode || row->in_pair != (p.in_pair != 0)) continue;
        if (tile_count(p, t.tile_h, t.tile_w) >= (1L << 30) || (long)p.H * p.W * 2 * (cin > cout ? cin : cout) >= (1L << 31)) return CONV_TOO_LARGE;
        r = route_of(t.family, *row, t.tile_h, t.tile_w, t.es, 1, p);
        return 0;
    }
    return CONV_NO_INSTANCE;
}

}  // namespace

int hrn_conv3x3_route(int dt, int cin, int cout, const ConvParams& p, bool general_only, ConvRoute& route) {
    if (const int rc = check_descriptor(dt, cin, cout, p, general_only)) return rc;
    if (dt == HRN_BF16X3) {                 // the only kernel of this precision mode: nothing behind it
        const int rc = route_fast(conv_table_v6x3(), cin, cout, p, route);
        HRN_CHECK(rc != CONV_NO_INSTANCE, -2, "conv3x3 bf16x3: unsupported layer cin=%d cout=%d res_mode=%d in_pair=%d", cin, cout, p.res_mode, p.in_pair);
        HRN_CHECK(rc != CONV_TOO_LARGE, -2, "conv3x3 bf16x3: image too large for 32-bit in-image offsets (H=%d W=%d)", p.H, p.W);
        return 0;
    }
    if (dt == HRN_BF16 && !p.scale && !p.relu && !general_only) {
        // the HRNet layers in bf16.  HRN_CONV_R64=0 / HRN_CONV_V6=0 force the general kernel (A/B timing, and the test that covers it)
        static const int r64 = [] { const char* e = getenv("HRN_CONV_R64"); return e ? atoi(e) : 1; }();
        static const int v6 = [] { const char* e = getenv("HRN_CONV_V6"); return e ? atoi(e) : 1; }();
        if (r64 && route_fast(conv_table_r64(), cin, cout, p, route) == 0) return 0;
        if (v6 && route_fast(conv_table_v6(), cin, cout, p, route) == 0) return 0;
    }
    HRN_CHECK(tile_count(p, CONV_TILE_H, CONV_TILE_W) < (1L << 40), -2, "conv3x3: bad tile count %ld", tile_count(p, CONV_TILE_H, CONV_TILE_W));
    // one persistent round is 8 waves per CU: 2 workgroups of 256 threads or 1 of 512
    route = route_of(CONV_GENERAL, GENERAL_ROWS[dt][cin / 128][cout / 128], CONV_TILE_H, CONV_TILE_W, hrn_esize(dt), 2 / (cout / 64), p);
    return 0;
}

int hrn_launch_conv3x3(int dt, int cin, int cout, const ConvParams& p, hipStream_t stream, bool general_only) {
    ConvRoute r;
    if (const int rc = hrn_conv3x3_route(dt, cin, cout, p, general_only, r)) return rc;
    HrnProfScope prof(r.name, r.flops, r.bytes, stream);
    return r.launch(p, r.grid, stream);
}

int hrn_launch_conv_pack(int dt, int cin, int cout, const float* w, void* packed, hipStream_t stream) {
    HRN_CHECK((cin == 64 || cin == 128) && (cout == 64 || cout == 128), -2, "conv pack: unsupported channels %d->%d", cin, cout);
    const size_t total = (size_t)cin * cout * 9;
    const int blocks = (int)((total + 255) / 256 < 1024 ? (total + 255) / 256 : 1024);
    if (dt == HRN_BF16X3) hipLaunchKernelGGL(conv_pack_x3_kernel, dim3(blocks), dim3(256), 0, stream, w, (unsigned short*)packed, cin, cout);
    else if (dt == HRN_BF16) hipLaunchKernelGGL(conv_pack_kernel<HRN_BF16>, dim3(blocks), dim3(256), 0, stream, w, packed, cin, cout);
    else hipLaunchKernelGGL(conv_pack_kernel<HRN_F32>, dim3(blocks), dim3(256), 0, stream, w, packed, cin, cout);
    HRN_LAUNCH_CHECK();
    return 0;
}
