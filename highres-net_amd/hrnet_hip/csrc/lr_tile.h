// What the operators on the HR grid share (upsample.hip, shift_add.hip, observe.hip): the walk over tiles of LR pixels, the test whether
// a view counts, the list of a chunk's counting views, and what every entry point refuses of a frame's sides and of the scale.  A file
// keeps its own kernels, weights, LDS layout and predicate.
//
// The walk: a workgroup of kThreads = 256 threads owns kTH x kTW = 8 x 32 LR pixels (one thread per pixel in a kernel's last pass) of one
// plane.  Tiles are numbered plane-major, tile = (plane * tiles_y + row) * tiles_x + column, as a size_t: their number may pass 2^32.  A
// launch has at most kMaxBlocks workgroups, and a workgroup takes the tiles blockIdx.x, blockIdx.x + gridDim.x, ...
#pragma once
#include "../../../include/hrnet_hip.h"
#include "kernels.h"

namespace {

constexpr int kTH = 8, kTW = 32, kThreads = 256;
constexpr unsigned kMaxBlocks = 1u << 16;                // tiles are grid-strided beyond this
constexpr int kMaxSide = 16384;
static_assert(kThreads == kTH * kTW, "one thread per LR pixel of the tile");
static_assert(HRN_UPSAMPLE_TILE_H == kTH && HRN_UPSAMPLE_TILE_W == kTW && HRN_SHIFT_ADD_TILE_H == kTH && HRN_SHIFT_ADD_TILE_W == kTW &&
                  HRN_OBSERVE_TILE_H == kTH && HRN_OBSERVE_TILE_W == kTW,
              "the three public tiles are this one: an operator's output goes straight into the next");

struct TilePos { size_t n; int y0, x0; };                // the plane and the tile's first LR row and column

__device__ __forceinline__ TilePos tile_pos(size_t tile, unsigned tiles_x, unsigned tiles_y) {
    const size_t per = (size_t)tiles_x * tiles_y;
    TilePos t;
    t.n = tile / per;
    const unsigned r = (unsigned)(tile - t.n * per);
    t.y0 = (int)(r / tiles_x) * kTH;
    t.x0 = (int)(r % tiles_x) * kTW;
    return t;
}

// the tiles of one H x W plane, H, W in 1..kMaxSide -> their number; tiles_x / tiles_y (may be null): along each axis
inline size_t plane_tiles(int H, int W, unsigned* tiles_x = nullptr, unsigned* tiles_y = nullptr) {
    const unsigned ny = (unsigned)((H + kTH - 1) / kTH), nx = (unsigned)((W + kTW - 1) / kTW);
    if (tiles_x) *tiles_x = nx;
    if (tiles_y) *tiles_y = ny;
    return (size_t)nx * ny;
}

inline unsigned blocks_for(size_t tiles) { return (unsigned)(tiles < kMaxBlocks ? tiles : kMaxBlocks); }

// view bv = b V + v counts: alpha non-zero (a flag; null: every view) and both shift components finite
__device__ __forceinline__ bool view_counts(const float* alphas, const float* shifts, size_t bv) {
    const float dy = shifts[2 * bv], dx = shifts[2 * bv + 1];
    return (!alphas || alphas[bv] != 0.f) && isfinite(dy) && isfinite(dx);
}

// Called by all 64 lanes of the workgroup's first wave, lane i with the verdict on view i of a chunk of at most 64 (false beyond its
// end): list[] <- the indices with a true verdict in ascending order, n_list <- their number.  The caller's barrier publishes both.
__device__ __forceinline__ void compact_chunk(bool ok, int* list, int* n_list) {
    const int tid = threadIdx.x;
    const unsigned long long votes = __ballot(ok);
    if (ok) list[__popcll(votes & ((1ull << tid) - 1ull))] = tid;
    if (tid == 0) *n_list = __popcll(votes);
}

// [a, a + na) and [b, b + nb), in bytes, share a byte
inline bool overlaps(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t a0 = (uintptr_t)a, a1 = a0 + na, b0 = (uintptr_t)b, b1 = b0 + nb;
    return a0 < b1 && b0 < a1;
}

// What every entry point refuses of positive H, W and of the scale; noun: "planes" or "frames".  -> true, or false with the error set.
inline bool check_side_scale(const char* fn, const char* noun, int H, int W, int scale) {
    if (H > kMaxSide || W > kMaxSide) { hrn_set_error("%s: %s of 1..%d a side; got H=%d W=%d", fn, noun, kMaxSide, H, W); return false; }
    if (!hrn_scale_ok(scale)) { hrn_set_error("%s: scale must be 2, 3 or 4 (got %d)", fn, scale); return false; }
    return true;
}

}  // namespace
