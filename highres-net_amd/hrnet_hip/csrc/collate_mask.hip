// The collate kernel with LR quality masks (hrn_collate_device_m in collate.hip, which has the design, the argument checks and the
// instances without masks): collate_kernel.h once more with COLLATE_MASK 1, in a translation unit of its own so that the instances
// that existed keep their code (collate_kernel.h says why).  min_L mask units follow the LR, SM and HR units of the grid.
// Resources (gfx950, -Rpass-analysis=kernel-resource-usage): with codes, collate_mask_kernel<true, true> 34 VGPRs, 8 KiB LDS (two
// tiles), <false, true> 22 VGPRs, no LDS; without codes <true, false> / <false, false> 30 / 22 VGPRs, no LDS.  No instance uses scratch.
#include "../../../include/hrnet_hip.h"
#include "collate_mask.h"
#define COLLATE_MASK 1
#include "collate_kernel.h"                              // collate_mask_kernel<VEC, AUG>

int hrn_launch_collate_masks(bool vec, const uint16_t* lr_arena, int64_t lr_elems, const uint16_t* hr_arena, int64_t hr_elems,
                             const uint8_t* sm_arena, int64_t sm_elems, const uint8_t* qm_arena, const int64_t* plan, const int32_t* codes,
                             int B, int min_L, int S, int scale, float* lrs, float* alphas, float* hrs, float* maps, float* lr_masks,
                             hipStream_t stream) {
    const int pieces = scale * scale;
    const dim3 grid((unsigned)(min_L + pieces + (hrs ? pieces : 0) + min_L), (unsigned)B);
    auto kernel = vec ? (codes ? collate_mask_kernel<true, true> : collate_mask_kernel<true, false>)
                      : (codes ? collate_mask_kernel<false, true> : collate_mask_kernel<false, false>);
    hipLaunchKernelGGL(kernel, grid, dim3(kThreads), 0, stream, lr_arena, (long long)lr_elems, hr_arena, (long long)hr_elems, sm_arena,
                       (long long)sm_elems, qm_arena, (const long long*)plan, (const int*)codes, min_L, S, scale, lrs, alphas, hrs, maps, lr_masks);
    HRN_LAUNCH_CHECK();
    return 0;
}
