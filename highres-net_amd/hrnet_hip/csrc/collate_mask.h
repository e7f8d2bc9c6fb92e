// The launcher of the collate kernel with LR quality masks (collate_mask.hip), called by hrn_collate_device_m (collate.hip).
#pragma once
#include "common.h"

// Arguments as checked by hrn_collate_device_m: every pointer but hrs / hr_arena / codes non-null, the QM arena of lr_elems bytes.
int hrn_launch_collate_masks(bool vec, const uint16_t* lr_arena, int64_t lr_elems, const uint16_t* hr_arena, int64_t hr_elems,
                             const uint8_t* sm_arena, int64_t sm_elems, const uint8_t* qm_arena, const int64_t* plan, const int32_t* codes,
                             int B, int min_L, int S, int scale, float* lrs, float* alphas, float* hrs, float* maps, float* lr_masks,
                             hipStream_t stream);
