// conv3x3 in split-bf16 ("bf16x3"): the precision mode that meets the reference's fp32 arithmetic (train.py:168-171, predict.py:36-37)
// to ~1e-5 at matrix-core speed.  Every fp32 value v travels as two bf16 planes, hi = bf16(v) and lo = bf16(v - hi) (~16 significant
// bits), weights likewise (packed as two planes), and a product is hi*hi + hi*lo + lo*hi on v_mfma_f32_16x16x32_bf16 with fp32
// accumulation (the dropped lo*lo term is ~2^-16 of the product).  The kernel is conv3x3_v6's (conv3x3_v6_impl.h) with the K loop run
// three passes per chunk and an epilogue that splits the fp32 result again; here are its instantiations and their route table:
//   64 -> 64   (+ plain residual)                 the encoder's five layers                       HRNet.py:17-22, :55-60
//   128 -> 128 (pair gather in / residual)        the fusion ResidualBlock                        HRNet.py:90-94, :113-119
//   128 -> 64  (+ alpha residual into the stack)  the fusion output conv                          HRNet.py:95-97, :123-131
//   64 -> 128, 128 -> 128 + plain residual        data gradients of the training path (a cout -> cin convolution on transposed weights)
#include "conv3x3_v6_impl.h"

// this file's instances: the family's common rows in bf16x3, and the encoder's two
#define X3_ROW(CI_, CO_, RESM_, PAIR_, NAME_) {CI_, CO_, RESM_, PAIR_, "conv3x3_bf16x3_" NAME_, launch_v6<CI_, CO_, RESM_, PAIR_, true>},
static const ConvInstance V6X3_ROWS[] = {V6_COMMON_ROWS(X3_ROW) X3_ROW(64, 64, 0, false, "64x64") X3_ROW(64, 64, 1, false, "64x64+res")};
#undef X3_ROW

// es = 4: the profiler's cost is the layer's algorithmic FLOPs (not x 3) and the bytes of both planes
const ConvTable& conv_table_v6x3() {
    static const ConvTable t = {CONV_V6X3, T6_H, T6_W, 4, V6X3_ROWS, sizeof V6X3_ROWS / sizeof *V6X3_ROWS};
    return t;
}
