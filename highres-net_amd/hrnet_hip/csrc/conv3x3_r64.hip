// conv3x3 64 -> 64, bf16, RESIDENT weights + two ping-pong wave teams: the encoder's five 64->64 layers
// (HRNet.py:17-22, :55-60).
//
// Why a third kernel: 64->64 sits at the MFMA/HBM ridge (288 FLOP/B), and in conv3x3_v3 its time was neither: every
// 256-pixel tile re-staged all 72 KB of weights through the slow ds_write path (a barrier per 3 taps), and the epilogue
// (bias, PReLU, residual, rounding: ~2,000 VALU cycles per tile) ran while the matrix pipe idled.  For CIN = COUT = 64
// the whole weight tensor fits in LDS for the lifetime of a persistent workgroup, next to TWO halo tiles:
//     weights  9 x 64 x 128 B            73,728 B   16-byte chunks XOR-swizzled by row & 7: conflict-free b128 reads (r64_layout.h)
//     input    2 x [10][34] px x 128 B   87,040 B   one halo tile per team, chunks swizzled by pixel & 7
//     bias                                   256 B                                        = 161,024 B
// 512 threads = two teams of four waves, one wave of each team on every SIMD.  The teams alternate:
//     ON  phase: 18 k-steps of 32 (9 taps x 2) on the team's halo tile, 16 v_mfma_f32_16x16x32_bf16 each (4 pixel blocks of 16 x
//                4 cout blocks of 16; a wave's tile is 2 pixel rows x 32 pixels x 64 couts) - one uninterrupted hand-pipelined
//                ds_read/MFMA stream, no weight traffic, no address arithmetic beyond one v_xor per pixel fragment, no barrier
//                inside.  (The chip holds a higher clock under this shape than under 32x32x16: CDNA4 guide, "DVFS give-back"
//                item 7; DESIGN.md 3.3 has the A/B.)  The PIXELS are the MFMA's A operand and row r of cout block cb holds cout
//                4 r + cb (an interleave applied by the one-time weight copy), so the four accumulators a lane has of one pixel
//                are four consecutive channels;
//                the tile's residual is fetched HBM -> VGPR at its start;
//     OFF phase: start the LDS-DMA (global_load_lds_dwordx4) of the team's next halo tile straight into the team's LDS
//                buffer - no staging registers, no ds_write; the bank swizzle is applied to each lane's SOURCE address -
//                then finish the tile just multiplied from the accumulators (bias pre-loaded, PReLU, one exchange between the
//                lanes of a pair so that a lane owns 16 contiguous bytes of one pixel and eight lanes a whole pixel row, residual,
//                one bf16 rounding, whole-line stores),
//                then wait (counted vmcnt: the tile's own stores stay in flight) for the DMAs.
// One workgroup barrier per phase.  While team A's waves occupy the matrix pipe, team B's waves on the same SIMDs do the
// VALU / VMEM work, so neither the epilogue nor the input staging costs MFMA time.  No ordinary global load is issued in
// the OFF phase: beside an LDS-DMA in flight hipcc waits vmcnt(0) for any of them, which would drain the DMAs early.
// Same math / layouts / packed weights / persistent XCD-windowed tile walk as the other conv kernels.
// Measured in-kernel (profiles/r01_final_inkernel_stamps.txt, on the kernel's first form, 36 k-steps of 4 v_mfma_f32_32x32x16_bf16:
// the same matrix-pipe cycles and LDS bytes per tile): ON 5.4 k cycles for 4.6 k of matrix pipe since the fragment
// reads are hand-issued with counted lgkmcnt waits (multiply()); the OFF phase (6.3 k, 8.2 k with the residual) is bound by
// the CU's vector-memory pipe - 44 DMA + 32 store (+ 32 residual load) wave-instructions at ~60-70 cycles each.  Without
// residual, full tiles take their halo from precomputed lane offsets (issue(), fix_borders()).  Outputs leave - and the residual
// arrives - as whole 128-byte lines (8 per instruction), with the non-temporal policy: both are touched once per launch and
// read / written next by another launch from HBM anyway (round 2: the residual variant too; its own time +2 %, the launches
// around it -3 %).
#include <type_traits>
#include "conv3x3.h"
#include "r64_layout.h"

namespace {

constexpr int HALO_H = CONV_TILE_H + 2;
constexpr int HALO_W = CONV_TILE_W + 2;
constexpr int IN_BYTES = HALO_H * HALO_W * 128;              // 43,520 (unpadded, swizzled)
constexpr int W_BYTES = 9 * 64 * 128;                        // 73,728
constexpr int LDS_BYTES = W_BYTES + 2 * IN_BYTES + 256;

__device__ __forceinline__ void lds_done_then_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// v_max_f32 without the canonicalising v_max(x, x) the compiler puts in front of fmaxf (both operands NaN -> NaN, so
// PReLU still propagates NaNs)
__device__ __forceinline__ float raw_max(float a, float b) {
    float y;
    asm("v_max_f32 %0, %1, %2" : "=v"(y) : "v"(a), "v"(b));
    return y;
}

// One exchange between the lanes of a pair (2k, 2k + 1).  Both hold a value for pixel e0 and one for pixel e1, each for its own
// channels (the even lane's are the lower ones).  Afterwards the even lane owns pixel e0 and the odd lane pixel e1: lo = the value
// of the lower channels of the lane's pixel, hi = of the upper ones.  One v_mov_dpp quad_perm [1,0,3,2] + three v_cndmask.
__device__ __forceinline__ void pair_exchange(unsigned a_e0, unsigned a_e1, bool odd, unsigned& lo, unsigned& hi) {
    const unsigned send = odd ? a_e0 : a_e1;
    const unsigned recv = (unsigned)__builtin_amdgcn_update_dpp(0, (int)send, 0xB1, 0xF, 0xF, true);
    lo = odd ? recv : a_e0;
    hi = odd ? a_e1 : recv;
}

__device__ __attribute__((aligned(16))) unsigned hrn_r64_zero16[4];

template <bool RES>
__global__ __launch_bounds__(512, 2) void conv3x3_r64_kernel(const ConvParams p) {
    if (p.only_if_nonpos && p.only_if_nonpos[0] > 0.f) return;      // uniform, before any barrier (ConvParams::only_if_nonpos)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* w_lds = smem;
    float* bias_lds = (float*)(smem + W_BYTES + 2 * IN_BYTES);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int team = wave >> 2, tw = wave & 3;
    unsigned char* in_lds = smem + W_BYTES + team * IN_BYTES;
    const int c15 = lane & 15, q = lane >> 4;             // MFMA fragment row (pixel / cout row of a block of 16) and k group
    const int H = p.H, W = p.W;
    const size_t hw = (size_t)H * W;
    const unsigned tiles_x = (W + CONV_TILE_W - 1) / CONV_TILE_W;
    const unsigned tiles_y = (H + CONV_TILE_H - 1) / CONV_TILE_H;
    const unsigned tiles = tiles_x * tiles_y;
    const unsigned total = tiles * (unsigned)p.M;           // < 2^31 (checked by the launcher)
    const unsigned G = gridDim.x;
    const unsigned bid = blockIdx.x;
    const unsigned slot = (G & 7) == 0 ? (bid & 7) * (G >> 3) + (bid >> 3) : bid;
    if (slot >= total) return;
    const int ntl = (int)((total - slot + G - 1) / G);      // tiles of this workgroup; team T takes local tiles T, T+2, ...
    const int nmine = (ntl + 1 - team) >> 1;

    // this team's tile cursor (image, tile in image): tiles slot + (2k + team) * G, advanced without divisions
    unsigned cur_m = (slot + team * G) / tiles, cur_t = (slot + team * G) - cur_m * tiles;
    const unsigned step_m = (2 * G) / tiles, step_t = 2 * G - step_m * tiles;

    // ---- one-time: all nine weight slices -> LDS (cout rows interleaved, chunks swizzled: r64_layout.h), bias
    {
        const u32x4* wg = (const u32x4*)p.wpk;                  // [tap][64 rows][8 chunks]
#pragma unroll
        for (int j = 0; j < W_BYTES / 16 / 512; ++j) {
            const int idx = tid + j * 512;
            const int row = idx >> 3, c = idx & 7;              // row = tap*64 + cout
            *(u32x4*)(w_lds + r64_chunk_off(r64_w_row(row >> 6, row & 63), c)) = wg[idx];
        }
        if (tid < 64) bias_lds[tid] = p.bias[tid];
    }

    // ---- halo tile of (m, t): HBM -> this team's LDS buffer by LDS-DMA.  Wave tw of the team issues pieces j = tw, tw+4,
    // ... < 43; piece j, lane i -> LDS bytes j*1024 + i*16 = halo pixel j*8 + (i >> 3), physical 16-B chunk i & 7, which
    // holds logical chunk (i & 7) ^ (pixel & 7) (r64_dma_chunk).  Out-of-image pixels are read from a zero line; the half-empty
    // last piece is EXEC-masked.  The geometry is recomputed from an opaque copy of the lane id so that it does not sit
    // in registers through the MFMA phase.
    // Residual-free variant: FULL tiles whose halo addresses all lie inside the tensor take a fast form - per-lane byte
    // offsets from the halo origin precomputed once (11 registers), no bounds tests, no zero-line select; pixels outside the
    // image are then zeroed in LDS (fix_borders) by the wave that fetched them, after its DMAs have landed.  The residual
    // variant has no registers to spare for the offsets (measured slower) and keeps the general form.
    unsigned voff[11], cm_lo = 0, cm_hi = 0;                // cm: 4 bits per piece: pixel in top row | bottom row | left | right column
    if (!RES) {
#pragma unroll
        for (int jj = 0; jj < 11; ++jj) {
            const int j = tw + 4 * jj;
            const int pix = j * 8 + (lane >> 3);
            const int py = pix / HALO_W, px = pix - py * HALO_W;
            voff[jj] = (unsigned)((py * W + px) * 128 + (r64_dma_chunk(j, lane) << 4));
            unsigned cls = (py == 0 ? 1u : 0u) | (py == HALO_H - 1 ? 2u : 0u) | (px == 0 ? 4u : 0u) | (px == HALO_W - 1 ? 8u : 0u);
            if (pix >= HALO_H * HALO_W) cls = 0;
            if (jj < 8) cm_lo |= cls << (4 * jj); else cm_hi |= cls << (4 * (jj - 8));
        }
    }
    unsigned pend_F = 0;                                    // border flags of the tile whose halo is in flight (fast form only)
    auto issue = [&](unsigned m, unsigned t) __attribute__((always_inline)) {
        const int ty = t / tiles_x;
        const int y0 = ty * CONV_TILE_H, x0 = (t - ty * tiles_x) * CONV_TILE_W;
        const unsigned char* base = (const unsigned char*)p.in + (size_t)m * hw * 128;     // uniform: image base
        const bool fast = !RES && y0 + CONV_TILE_H <= H && x0 + CONV_TILE_W <= W && (m > 0 || y0 > 0) &&
                          ((int)m + 1 < p.M || (size_t)(y0 + CONV_TILE_H) * W + x0 + CONV_TILE_W < hw);
        pend_F = 0;
        if (fast) {
            const unsigned char* hb = base + ((long)(y0 - 1) * W + (x0 - 1)) * 128;
#pragma unroll
            for (int jj = 0; jj < 11; ++jj) {
                const int j = tw + 4 * jj;
                if (j < 43) {
                    if (jj < 10 || j * 8 + (lane >> 3) < HALO_H * HALO_W)
                        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(hb + voff[jj]),
                                                         (__attribute__((address_space(3))) void*)(in_lds + j * 1024), 16, 0, 0);
                }
            }
            pend_F = (y0 == 0 ? 1u : 0u) | (y0 + CONV_TILE_H == H ? 2u : 0u) | (x0 == 0 ? 4u : 0u) | (x0 + CONV_TILE_W == W ? 8u : 0u);
            __builtin_amdgcn_sched_barrier(0);
            return;
        }
        int lq = lane;
        asm volatile("" : "+v"(lq));
#pragma unroll
        for (int jj = 0; jj < 11; ++jj) {
            const int j = tw + 4 * jj;
            if (j < 43) {
                const int pix = j * 8 + (lq >> 3);
                const int lc = r64_dma_chunk(j, lq);
                const int py = pix / HALO_W, px = pix - py * HALO_W;
                const int gy = y0 - 1 + py, gx = x0 - 1 + px;
                const bool ok = (unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W;
                const unsigned char* src = ok ? base + (unsigned)((gy * W + gx) * 128 + lc * 16) : (const unsigned char*)hrn_r64_zero16;
                if (pix < HALO_H * HALO_W)
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                                     (__attribute__((address_space(3))) void*)(in_lds + j * 1024), 16, 0, 0);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    };
    auto fix_borders = [&]() __attribute__((always_inline)) {
        if (!RES && pend_F) {
            const unsigned fm = pend_F * 0x11111111u;
            const unsigned hit_lo = cm_lo & fm, hit_hi = cm_hi & fm;
            const u32x4 z = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int jj = 0; jj < 11; ++jj) {
                const int j = tw + 4 * jj;
                if (j < 43) {
                    const unsigned h = jj < 8 ? (hit_lo >> (4 * jj)) & 15u : (hit_hi >> (4 * (jj - 8))) & 15u;
                    if (h) *(u32x4*)(in_lds + j * 1024 + lane * 16) = z;
                }
            }
        }
    };

    const bool has_slope = p.slope != nullptr;
    const float slope = has_slope ? p.slope[0] : 0.f;
    const bool slope01 = slope >= 0.f && slope <= 1.f;
    // fragment addresses (r64_layout.h).  Weights: row c15 of cout block cb, k-half kh -> a_off[kh] + cb*2048 + tap*8192.
    // Input: pixel block pxb = (row pxb >> 1, column half pxb & 1) of the wave, tap (ky, kx): halo pixel (2*tw + (pxb >> 1) + ky,
    // 16*(pxb & 1) + c15 + kx), k-half kh -> (b_off[(pxb >> 1) + ky][kx] ^ (kh << 6)) + (pxb & 1)*2048   (12 registers; the swizzle
    // has period 8 pixels, so the second column half is an instruction offset; kh is bit 2 of the chunk = bit 6 of the address, and
    // the buffer base has zero low bits, so it is folded in before the xor)
    // All of them are absolute LDS byte addresses (the fragment reads are hand-written ds_read_b128, see multiply()); the
    // 16-bit instruction offset reaches taps 0-3 from a_off and taps 4-8 from a_off_hi.
    const unsigned lds0 = (unsigned)(__UINTPTR_TYPE__)(__attribute__((address_space(3))) unsigned char*)smem;
    unsigned a_off[2], a_off_hi[2], b_off[4][3];
#pragma unroll
    for (int kh = 0; kh < 2; ++kh) {
        a_off[kh] = lds0 + (unsigned)r64_frag_off(0, c15, q, kh);
        a_off_hi[kh] = a_off[kh] + 4 * 8192;
    }
#pragma unroll
    for (int row = 0; row < 4; ++row)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx)
            b_off[row][kx] = lds0 + (unsigned)(W_BYTES + team * IN_BYTES) + (unsigned)r64_frag_off((2 * tw + row) * HALO_W + kx, c15, q, 0);

    // [cout block][pixel block]: element e of lane (q, c15) = pixel 4q + e of the pixel block, channel 4*c15 + cb.  Lives from the ON
    // phase into the OFF phase
    f32x4 acc[4][4];

    // ---- ON phase: the 18 k-steps of one tile
    auto multiply = [&]() __attribute__((always_inline)) {
        // the accumulators start at the bias
        {
            const f32x4 b = *(const f32x4*)(bias_lds + r64_acc_channel(c15, 0));
#pragma unroll
            for (int cb = 0; cb < 4; ++cb)
#pragma unroll
                for (int pxb = 0; pxb < 4; ++pxb) acc[cb][pxb] = f32x4{b[cb], b[cb], b[cb], b[cb]};
        }
        // Hand-issued fragment stream.  In a kernel that also issues LDS-DMA hipcc does not count LDS waits: it answers
        // every fragment use with s_waitcnt lgkmcnt(0), which waits for the reads issued a moment ago as well and exposed
        // the whole LDS latency every third k-step (in-kernel stamps: 6,800 cycles per tile for 4,608 cycles of MFMA).  So
        // the ds_read_b128 are inline asm - invisible to the compiler's wait insertion - and are waited for with counted
        // lgkmcnt here; and they are spread over the MFMA gaps instead of eight in a burst in front of the sixteen MFMAs (all
        // four waves of the team burst together, and an MFMA cannot issue before the reads in front of it have).
        // A step's eight reads, in program order: B0 B1 B2 B3 (pixel blocks) A0 A1 A2 A3 (cout blocks).  Step i issues the reads
        // of step i+2, one behind every second MFMA.  MFMA order: cout block g = 0..3, within it pixel block 0..3.  LDS reads
        // return in order, so before group g of step i the reads B0-3(i), A0..Ag(i) are back once at most the younger ones are
        // outstanding: A(g+1)..A3(i), the eight of step i+1, and the 2g of step i+2 issued so far.  Before group 3 that would be
        // lgkmcnt(14); it waits for one read more (13), so that never more than 15 reads are in flight: the counter has four
        // bits.  The last two steps issue nothing and count down.  The asm statements are volatile: they keep their order, and
        // each wait names the fragments it guards as in/out operands, so no MFMA can move in front of its wait.  The read of a
        // gap may be scheduled in front of that gap's MFMA but never across the sched_barrier to another gap's wait.
        constexpr int NK = 18;
        bf16x8 fa[3][4], fb[3][4];
        auto rd = [&](bf16x8& dst, unsigned addr, int imm) __attribute__((always_inline)) {
            asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(imm));
        };
        auto load_part = [&](int i, int part) __attribute__((always_inline)) {
            const int s_ = i % 3, tap = i >> 1, kh = i & 1;
            const int ky = tap / 3, kx = tap - ky * 3;
            if (part < 4) {
                unsigned kbits = 0;
                if (kh) asm volatile("s_mov_b32 %0, %1" : "=s"(kbits) : "n"(64));          // opaque: keeps the compiler from
                rd(fb[s_][part], b_off[(part >> 1) + ky][kx] ^ kbits, (part & 1) * 2048);   // materialising all 72 addresses
            } else {
                rd(fa[s_][part - 4], tap < 4 ? a_off[kh] : a_off_hi[kh], (tap < 4 ? tap : tap - 4) * 8192 + (part - 4) * 2048);
            }
        };
        auto wait_lgkm = [&](int n, bf16x8& f) __attribute__((always_inline)) {
            asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(f) : "n"(n));
        };
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");          // nothing of the compiler's own left in the LGKM queue
        __builtin_amdgcn_s_setprio(3);                              // the matrix-pipe stream wins issue ties against the OFF team
#pragma unroll
        for (int part = 0; part < 8; ++part) load_part(0, part);
#pragma unroll
        for (int part = 0; part < 4; ++part) load_part(1, part);
        asm volatile("s_waitcnt lgkmcnt(11)" ::: "memory");         // (at most 15 in flight)
#pragma unroll
        for (int part = 4; part < 8; ++part) load_part(1, part);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < NK; ++i) {
            const int s_ = i % 3;
            const bool more = i + 2 < NK;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int younger = (3 - g) + (i + 1 < NK ? 8 : 0) + (more ? 2 * g : 0);
                if (g == 0) asm volatile("" : "+v"(fb[s_][0]), "+v"(fb[s_][1]), "+v"(fb[s_][2]), "+v"(fb[s_][3]));   // older than A0(i)
                wait_lgkm(younger < 13 ? younger : 13, fa[s_][g]);
#pragma unroll
                for (int pxb = 0; pxb < 4; ++pxb) {
                    acc[g][pxb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[s_][pxb], fa[s_][g], acc[g][pxb], 0, 0, 0);
                    if (more && (pxb & 1) == 0) load_part(i + 2, 2 * g + (pxb >> 1));
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
        __builtin_amdgcn_s_setprio(0);
    };

    // ---- epilogue geometry.  After the pair exchange the even lane of a pair owns pixel 4q + 2h and the odd lane pixel 4q + 2h + 1
    // of a pixel block (h = 0, 1: two store instructions per block), 16 bytes = channels 8*(c15 >> 1) .. + 7: the eight lanes
    // with one (q, parity) are one whole pixel row, an instruction covers 8 whole 128-byte lines.  The residual is fetched the same way.
    // Byte offset from the tile origin of pixel block pxb, half h: ((2*tw + (pxb >> 1)) * W + 16*(pxb & 1) + 2*h) * 128 + lane_off.
    // ---- residual of the tile at the cursor: the 16 bytes this lane will own after the exchange, per pixel block and half.  Fetched
    // at the START of the ON phase, consumed in the OFF phase - a whole K loop of latency cover.
    u32x4 resv[4][2];
    float res_alpha = 1.f;
    auto fetch_residual = [&]() __attribute__((always_inline)) {
        const int m = (int)cur_m;
        const int ty = cur_t / tiles_x;
        const int y0 = ty * CONV_TILE_H, x0 = (cur_t - ty * tiles_x) * CONV_TILE_W;
        const unsigned char* rbase = (const unsigned char*)p.res + (size_t)m * hw * 128;               // res_mode 1 (image base)
        if (p.res_mode == 3) {
            const int ob = m / p.out_h, oi = m - ob * p.out_h;
            rbase = (const unsigned char*)p.res + ((size_t)ob * p.res_vs + oi) * hw * 128;
            res_alpha = p.alphas ? p.alphas[(size_t)ob * p.alpha_vs + (p.pair_last - oi)] : 1.f;
        }
#pragma unroll
        for (int pxb = 0; pxb < 4; ++pxb) {
            const int gy = y0 + 2 * tw + (pxb >> 1), gyc = gy < H ? gy : H - 1;
            // whole 128-byte lines per instruction; read once: non-temporal (with 16-byte pieces per instruction that costs +16 %:
            // nothing merges them)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int gx = x0 + 16 * (pxb & 1) + 4 * q + 2 * h + (lane & 1), gxc = gx < W ? gx : W - 1;
                resv[pxb][h] = __builtin_nontemporal_load((const u32x4*)(rbase + (unsigned)((gyc * W + gxc) * 128 + (c15 >> 1) * 16)));
            }
        }
    };

    // ---- OFF phase: finish the tile at the cursor from the accumulators, refill the team's halo buffer with the next one
    auto finish = [&](bool more) __attribute__((always_inline)) {
        const int m = (int)cur_m;
        const int ty = cur_t / tiles_x;
        const int y0 = ty * CONV_TILE_H, x0 = (cur_t - ty * tiles_x) * CONV_TILE_W;
        cur_t += step_t; cur_m += step_m;
        if (cur_t >= tiles) { cur_t -= tiles; ++cur_m; }
        size_t oimg = (size_t)m;
        int ob = 0, oi = 0;
        if (p.out_h > 0) { ob = m / p.out_h; oi = m - ob * p.out_h; oimg = (size_t)ob * p.out_vs + oi; }
        // uniform base at the tile origin; the per-lane byte offset is tile-independent
        unsigned char* outp = (unsigned char*)p.out + (oimg * hw + (size_t)y0 * W + x0) * 128;
        if (RES) {                                          // make the residual's wait happen BEFORE the DMAs are issued
#pragma unroll
            for (int pxb = 0; pxb < 4; ++pxb)
#pragma unroll
                for (int h = 0; h < 2; ++h) asm volatile("" :: "v"(resv[pxb][h]));
            asm volatile("" :: "v"(res_alpha));
        }
        if (more) issue(cur_m, cur_t);                      // in flight while the epilogue runs
        const bool odd = (lane & 1) != 0;
        const int lane_px = 4 * q + (lane & 1);             // the lane's pixel in its pixel block, for h = 0
        const unsigned lane_off = (unsigned)(lane_px * 128 + (c15 >> 1) * 16);
        // ACT 0: no activation | 1: PReLU with 0 <= slope <= 1 as max(x, slope*x) (2 VALU) | 2: general PReLU (3 VALU)
        auto epilogue = [&](auto act_c) __attribute__((always_inline)) {
        constexpr int ACT = decltype(act_c)::value;
#pragma unroll
        for (int pxb = 0; pxb < 4; ++pxb) {
            const int gy = y0 + 2 * tw + (pxb >> 1);
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                float xe[4], xo[4];                         // channels 4*c15 + cb of pixels 4q + 2h (the even lane's) and 4q + 2h + 1
#pragma unroll
                for (int cb = 0; cb < 4; ++cb) { xe[cb] = acc[cb][pxb][2 * h]; xo[cb] = acc[cb][pxb][2 * h + 1]; }
                if (ACT == 1) {
#pragma unroll
                    for (int cb = 0; cb < 4; ++cb) { xe[cb] = raw_max(xe[cb], slope * xe[cb]); xo[cb] = raw_max(xo[cb], slope * xo[cb]); }
                } else if (ACT == 2) {
#pragma unroll
                    for (int cb = 0; cb < 4; ++cb) { xe[cb] = xe[cb] >= 0.f ? xe[cb] : slope * xe[cb]; xo[cb] = xo[cb] >= 0.f ? xo[cb] : slope * xo[cb]; }
                }
                // pair_exchange: afterwards a lane holds, for its pixel, channels 8*(c15 >> 1) + (0..3, 4..7): 16 contiguous bytes once
                // rounded to bf16
                u32x4 u;
                if (RES) {
                    float v[8];
#pragma unroll
                    for (int cb = 0; cb < 4; ++cb) {
                        unsigned lo, hi;
                        pair_exchange(__float_as_uint(xe[cb]), __float_as_uint(xo[cb]), odd, lo, hi);
                        v[cb] = __uint_as_float(lo);
                        v[4 + cb] = __uint_as_float(hi);
                    }
                    const u32x4 rq = resv[pxb][h];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float r0 = __uint_as_float(rq[j] << 16), r1 = __uint_as_float(rq[j] & 0xffff0000u);
                        if (p.res_mode == 3) { v[2 * j] = r0 + res_alpha * v[2 * j]; v[2 * j + 1] = r1 + res_alpha * v[2 * j + 1]; }
                        else { v[2 * j] += r0; v[2 * j + 1] += r1; }
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j) u[j] = pack2_bf16(v[2 * j], v[2 * j + 1]);
                } else {                                    // no residual: round first, exchange packed pairs (half the exchanges)
                    unsigned lo0, hi0, lo1, hi1;
                    pair_exchange(pack2_bf16(xe[0], xe[1]), pack2_bf16(xo[0], xo[1]), odd, lo0, hi0);
                    pair_exchange(pack2_bf16(xe[2], xe[3]), pack2_bf16(xo[2], xo[3]), odd, lo1, hi1);
                    u[0] = lo0; u[1] = lo1; u[2] = hi0; u[3] = hi1;
                }
                // whole-line store.  Read next by another launch, from HBM anyway: non-temporal.  A/B on one box, both variants with
                // whole-line nt accesses against plain stores / 16-byte residual pieces: 64->64 1.015 -> 0.986 ms, + residual 1.328 ->
                // 1.356, the encoder -0.03 ms and the launches after it a little faster (less of the L2 turned over)
                unsigned char* oq = outp + ((unsigned)(((2 * tw + (pxb >> 1)) * W + 16 * (pxb & 1) + 2 * h) * 128) + lane_off);
                if (gy < H && x0 + 16 * (pxb & 1) + 2 * h + lane_px < W) __builtin_nontemporal_store(u, (u32x4*)oq);
            }
        }
        };
        if (!has_slope) epilogue(std::integral_constant<int, 0>{});
        else if (slope01) epilogue(std::integral_constant<int, 1>{});
        else epilogue(std::integral_constant<int, 2>{});
        {   // the halo DMAs were issued before this tile's stores: wait until only those stores are outstanding.  Four store
            // instructions per pixel row inside the image; where the tile reaches past the image's right edge an instruction may have
            // no active lane and may be skipped, so there nothing is left in flight
            const int nst = x0 + CONV_TILE_W <= W ? 4 * ((y0 + 2 * tw < H) + (y0 + 2 * tw + 1 < H)) : 0;
            if (nst == 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
            else if (nst == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        fix_borders();
    };

    if (nmine > 0) issue(cur_m, cur_t);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    fix_borders();
    lds_done_then_barrier();                                // weights, bias, both teams' first halo tiles

    // phase ph: team 0 is at step s = ph, team 1 at s = ph - 1; even s = ON (tile s/2), odd s = OFF (tile (s-1)/2)
    for (int ph = 0; ph <= ntl; ++ph) {
        const int s = ph - team;
        if (s >= 0) {
            const int k = s >> 1;
            if (k < nmine) {
                if ((s & 1) == 0) { if (RES) fetch_residual(); multiply(); }
                else finish(k + 1 < nmine);
            }
        }
        if (ph < ntl) lds_done_then_barrier();
    }
}


template <bool RES>
int launch_r64(const ConvParams& p, long grid, hipStream_t stream) {
    { const int rc_lds = hrn_allow_lds((const void*)conv3x3_r64_kernel<RES>, LDS_BYTES); if (rc_lds) return rc_lds; }
    hipLaunchKernelGGL(conv3x3_r64_kernel<RES>, dim3((unsigned)grid), dim3(512), LDS_BYTES, stream, p);
    HRN_LAUNCH_CHECK();
    return 0;
}

// The instances: <RES> is any residual read at the stored pixel, the plain tensor (1) or the view-stack slot with its alpha (3); a plain
// input tensor only.
const ConvInstance R64_ROWS[] = {{64, 64, 0, 0, "conv3x3_bf16_64x64", launch_r64<false>},
                                 {64, 64, 1, 0, "conv3x3_bf16_64x64+res", launch_r64<true>},
                                 {64, 64, 3, 0, "conv3x3_bf16_64x64+res", launch_r64<true>}};
static_assert(LDS_BYTES <= 160 * 1024, "LDS budget");

}  // namespace

const ConvTable& conv_table_r64() {
    static const ConvTable t = {CONV_R64, CONV_TILE_H, CONV_TILE_W, 2, R64_ROWS, sizeof R64_ROWS / sizeof *R64_ROWS};
    return t;
}
