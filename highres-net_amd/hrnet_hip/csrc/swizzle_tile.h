// The 32 x 32 f32 LDS tile that collate.hip and dihedral.hip transpose through: pitch kTile = 32 dwords (no padding - a
// ds_read_b128 needs 16-byte rows), the 16-byte slot of element (R, C) XOR-swizzled with the row block.  collate.hip's header
// derives the bank-conflict counts (0 for the column writes, 0 for the row reads); dihedral.hip accesses it the same way.
#pragma once

constexpr int kTile = 32;                                // side of a transposed sub-tile: 256 lanes x 4 samples = one tile

// dword index of element (R, C) of a kTile x kTile f32 tile: R * 32 + 4 * ((C / 4) ^ (R / 4)) + C % 4
static __device__ __forceinline__ int tile_at(int R, int C) { return R * kTile + ((((C >> 2) ^ (R >> 2)) & 7) << 2) + (C & 3); }
