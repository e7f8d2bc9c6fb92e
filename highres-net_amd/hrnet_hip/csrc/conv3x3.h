// 3x3 / pad 1 / stride 1 convolution as an LDS-staged implicit GEMM on MFMA (gfx950).
#pragma once
#include <string.h>
#include "common.h"

// Tile geometry shared by the kernel, the weight packer and the host launcher.
#define CONV_TILE_H 8
#define CONV_TILE_W 32
#define CONV_STEP_BYTES 8192   // one weight slice: 64 output channels x 128 bytes of K

struct ConvParams {
    const void* in;        // in_pair == 0: [M][H][W][CIN];  in_pair == 1: unused (input gathered from `stack`)
    const void* stack;     // view stack [B][pair_vs][H][W][64] for the pair descriptor (pair_h > 0)
    int in_pair;           // 1: the conv input is cat(view i, view pair_last - i) on channels, never materialised
    void* out;             // plain: [M][H][W][COUT]; slot: view stack, image b*out_vs + i
    const void* res;       // res_mode 1: [M][H][W][COUT]; res_mode 3: view stack, image b*res_vs + i
    const float* alphas;   // res_mode 3: [B][alpha_vs] (null -> scale 1)
    const void* wpk;       // packed weights, see conv_pack_index()
    const float* bias;     // [COUT] f32
    const float* slope;    // PReLU slope (1 float, device) or null = no activation
    int M, H, W;
    int pair_h, pair_last, pair_vs;   // pair_h > 0: image m -> (b = m / pair_h, i = m % pair_h); channels 0..63 = view i, 64..127 = view pair_last - i
    int out_h, out_vs;                // out_h > 0: output image m -> slot b*out_vs + i
    int res_mode;                     // 0 none | 1 tensor `res` | 2 pair gather of `in` | 3 x_i (slot of `res`) + alpha_partner * y
    int alpha_vs, res_vs;
    int relu;                         // 1: y = max(y, 0) after bias (ShiftNet eval with folded BN uses scale/shift below)
    const float* scale;               // optional per-channel scale applied before bias (folded BatchNorm), null = 1
    // HRN_BF16X3 only: every activation tensor is a PAIR of bf16 planes (hi, lo) in the bf16 layout; byte offset of the lo plane from
    // the hi plane of `in` / `stack` / `out` / `res` (0 otherwise)
    size_t in_lo, stack_lo, out_lo, res_lo;
    const float* only_if_nonpos;      // when set, the launch does nothing unless only_if_nonpos[0] <= 0 (the training backward's
                                      // recomputation of a pre-activation, needed only behind a PReLU whose slope is not positive)
};

// A well-formed descriptor - what keeps every index the kernels form inside the tensors as described above.  hrn_conv3x3_route checks it
// first, for every dtype, before any route is considered; a violation is error -2 with a message that names the field.
//   always                  M, H, W > 0;  wpk, bias, out non-null;  in non-null unless in_pair;  res_mode in 0..3
//   in_pair                 cin == 128
//   in_pair or res_mode 2   stack non-null, pair_h > 0, M % pair_h == 0, pair_h - 1 <= pair_last < pair_vs (both views of every pair lie
//                           in the sample's pair_vs slots);  res_mode 2: cout == 128
//   res_mode 1              res non-null
//   res_mode 3              res non-null, out_h > 0, res_vs >= out_h; with alphas: out_h - 1 <= pair_last < alpha_vs
//   out_h > 0               M % out_h == 0, out_vs >= out_h
//   bf16x3                  out_lo and in_lo (in_pair: stack_lo) != 0; no scale / relu; no general kernel
static inline ConvParams conv_base(int M, int H, int W) {
    ConvParams p;
    memset(&p, 0, sizeof p);
    p.M = M; p.H = H; p.W = W;
    return p;
}

// Number of packed weight elements of one conv layer (== cin*cout*9).
static inline size_t conv_packed_elems(int cin, int cout) { return (size_t)cin * cout * 9; }

// ---- Which kernel runs a launch.  Four families: the general kernel (conv3x3.hip), r64 (conv3x3_r64.hip: bf16 64 -> 64, LDS-resident
// weights), v6 (conv3x3_v6.hip: bf16 with 128 channels on a side - the three layers of a fusion level, and the data gradients 64 -> 128 and
// 128 -> 128 + plain residual) and v6x3 (conv3x3_v6x3.hip: bf16x3 on the v6 skeleton, the only kernel of that dtype).  A fast family
// states its instantiated kernels as a table of rows, in the translation unit of its kernels: a layer is applicable to the family exactly
// when a row matches its (cin, cout, res_mode, in_pair), and that row's pointer is the dispatch.
enum ConvFamily { CONV_GENERAL, CONV_R64, CONV_V6, CONV_V6X3 };
typedef int (*ConvLaunchFn)(const ConvParams& p, long grid, hipStream_t stream);
struct ConvInstance { int cin, cout, res_mode, in_pair; const char* name; ConvLaunchFn launch; };      // name: the profiler's family name
struct ConvTable { int family, tile_h, tile_w, es; const ConvInstance* rows; int nrows; };            // es: bytes per element, all planes
const ConvTable &conv_table_r64(), &conv_table_v6(), &conv_table_v6x3();
// a chosen route: family, profiler name and cost, tile shape, persistent grid, and the launcher of the template instance
struct ConvRoute { int family; const char* name; int tile_h, tile_w; long grid; double flops, bytes; ConvLaunchFn launch; };

// The pure step: checks the contract above, then chooses.  Launches nothing, allocates nothing.  dt: HRN_F32 / HRN_BF16 / HRN_BF16X3;
// (cin, cout) in {64,128}^2.  bf16x3 -> v6x3 only (no row, or an image beyond its 32-bit offsets: an error).  bf16 without scale / relu /
// general_only -> r64, then v6, where a row matches and the image fits (HRN_CONV_R64=0 / HRN_CONV_V6=0, read once per process, switch
// them off), else general.  Everything else -> general.  Returns 0 or a negative error.
int hrn_conv3x3_route(int dt, int cin, int cout, const ConvParams& p, bool general_only, ConvRoute& route);

// Route, then launch on `stream`: the one entry the rest of the library calls.  general_only: conv3x3.hip's general kernel even where
// r64 / v6 apply (the route HRN_CONV_R64=0 HRN_CONV_V6=0 selects; kernel_test.hip's route 1).  Returns 0 or a negative error.
int hrn_launch_conv3x3(int dt, int cin, int cout, const ConvParams& p, hipStream_t stream, bool general_only);

// Pack OIHW f32 weights [cout][cin][3][3] into the kernel's step-major layout (device to device).
int hrn_launch_conv_pack(int dt, int cin, int cout, const float* w_oihw, void* packed, hipStream_t stream);
