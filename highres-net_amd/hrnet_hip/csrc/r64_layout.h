// Index arithmetic of conv3x3_r64's two LDS images (weights, halo tile) and of its v_mfma_f32_16x16x32_bf16 fragments.  Plain
// integer functions, included by the kernel and compiled on the host by tests/test_r64_swizzle_host.py, which enumerates every
// fragment read for bank conflicts and checks that the write side (weight copy, halo DMA) is the inverse of the read side.
//
// Both images have 128-byte rows (one halo pixel or one cout row of a tap: 64 bf16 = 8 chunks of 16 bytes).  A fragment read is
// one ds_read_b128 per lane: lane l = (q = l >> 4, c15 = l & 15) takes row base + c15, logical chunk 4 kh + q (kh = which 32 of
// the 64 input channels the k-step covers).  The LDS serves a ds_read_b128 in four groups of 16 lanes, {0-3, 12-15, 20-27},
// {4-11, 16-19, 28-31} and the same + 32: a group mixes eight rows at one q with the other eight rows at q ^ 1.  Storing logical
// chunk c of row `row` at physical chunk c ^ (row & 7) makes every group hit the sixteen 16-byte slots of the 256-byte bank row
// once, for every base row (the halo image is read at every alignment).  The 32x32x16 kernel's swizzle, (row >> 1) & 7, is
// 2-way on this fragment for three base alignments in four.
#pragma once

#if defined(__HIPCC__)
#define R64_FN __host__ __device__ inline constexpr
#else
#define R64_FN inline constexpr
#endif

R64_FN int r64_swz(int row) { return row & 7; }
// byte offset, inside an image, of logical 16-byte chunk `chunk` (0..7) of row `row`
R64_FN int r64_chunk_off(int row, int chunk) { return row * 128 + ((chunk ^ r64_swz(row)) << 4); }
// the logical chunk lane group q reads in k-half kh: both operands take their 32 k-values in this order
R64_FN int r64_frag_chunk(int q, int kh) { return kh * 4 + q; }
// byte offset of the fragment piece lane (q, c15) reads: row base_row + c15
R64_FN int r64_frag_off(int base_row, int c15, int q, int kh) { return r64_chunk_off(base_row + c15, r64_frag_chunk(q, kh)); }
// halo DMA: lane i of 1 KB piece j writes LDS bytes j * 1024 + i * 16 = pixel j * 8 + (i >> 3), physical chunk i & 7; the logical
// chunk it has to fetch there
R64_FN int r64_dma_pixel(int piece, int lane) { return piece * 8 + (lane >> 3); }
R64_FN int r64_dma_chunk(int piece, int lane) { return (lane & 7) ^ r64_swz(r64_dma_pixel(piece, lane)); }
// weights: row `r` of cout block cb of a tap holds cout 4 r + cb, so that the four accumulators a lane has of one pixel (one per cout
// block) are four consecutive channels.  LDS row of (tap, cout):
R64_FN int r64_w_row(int tap, int cout) { return tap * 64 + (cout & 3) * 16 + (cout >> 2); }
R64_FN int r64_acc_channel(int c15, int cb) { return 4 * c15 + cb; }
