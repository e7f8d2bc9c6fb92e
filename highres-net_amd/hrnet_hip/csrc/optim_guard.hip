// The guarded optimiser step: global-norm gradient clipping, a skip when any gradient element is not finite, decoupled weight decay
// (AdamW) and an exponential moving average of the weights, all on the flat fp32 buffers hrnet_hip/optim.py owns, with no host
// round trip.  Three stages per step, all enqueued on one stream:
//   1. grad_sumsq_kernel + grad_sumsq_finish_kernel (per parameter group): sum of g^2 over the finite elements and the number of
//      non-finite ones, in fp64.  (double)g * (double)g is exact, so the only rounding is the additions; the order is fixed (the
//      grid is a function of n alone, no atomics), so the result is bit-reproducible and does not depend on what else runs.
//      fp32 sums, as torch.nn.utils.clip_grad_norm_ takes them, overflow at |g| ~ 2e19 and hand back a coefficient of 0.
//   2. optim_prepare_kernel (one wave, per group): the groups' sums -> the step-control block hrn_optim_ctl of one group: the
//      global norm, the clip coefficient min(1, max_norm / (norm + 1e-6)), skip, and - only when the step is applied - the applied
//      count and the bias corrections that follow from it.  The count lives on the device because the host cannot know about a
//      skip without a sync, and a skipped step must not advance the bias correction (a skipped optimizer.step() does not count).
//   3. adam_ex_kernel: adam.hip's update with g' = coef g formed in registers (the gradient buffer is never written - unlike
//      clip_grad_norm_, which rescales .grad in place), coupled or decoupled decay, and the EMA of the new weights.  It reads the
//      control block with uniform loads and returns without writing when skip is set.
// HBM traffic of the step: 16 B read + 12 B written per parameter as adam_kernel, + 4 B read + 4 B written with the EMA; the
// sum of squares reads the gradient once more (4 B).
#include "../../../include/hrnet_hip.h"
#include "common.h"
#include "wave_sums.h"
#include <math.h>
#include <stdint.h>

namespace {

constexpr int SUMSQ_THREADS = 256;
constexpr size_t SUMSQ_MAX_BLOCKS = 1024;

// the grid of the sum of squares: a function of n alone, so that the order of the additions is fixed
size_t sumsq_blocks(size_t n) {
    size_t b = (n / 4 + SUMSQ_THREADS - 1) / SUMSQ_THREADS;
    return b < 1 ? 1 : b > SUMSQ_MAX_BLOCKS ? SUMSQ_MAX_BLOCKS : b;
}

__device__ __forceinline__ void sumsq_add(float x, double& sum, double& bad) {
    const bool finite = (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u;
    const double d = finite ? (double)x : 0.0;
    sum += d * d;                                                // the product of two floats is exact in a double
    bad += finite ? 0.0 : 1.0;
}

// (sum, count) of the block's four waves -> lane 0 of wave 0, waves added in index order
__device__ __forceinline__ void block_sums(double* a, double (*lds)[2], int tid) {
    const int lane = tid & 63, wave = tid >> 6;
    WaveSums<2, 0>::run(a, lane);                                // lane 0: the wave's sum, lane 1: the wave's count
    if (lane < 2) lds[wave][lane] = a[0];
    __syncthreads();
    if (tid < 2) a[0] = ((lds[0][tid] + lds[1][tid]) + lds[2][tid]) + lds[3][tid];
}

__global__ __launch_bounds__(SUMSQ_THREADS) void grad_sumsq_kernel(const float* __restrict__ g, size_t n, double* __restrict__ partial) {
    __shared__ double lds[SUMSQ_THREADS / 64][2];
    const size_t n4 = n / 4;
    double s[4] = {0.0, 0.0, 0.0, 0.0}, bad = 0.0;
    for (size_t i = (size_t)blockIdx.x * SUMSQ_THREADS + threadIdx.x; i < n4; i += (size_t)gridDim.x * SUMSQ_THREADS) {
        const f32x4 gv = ((const f32x4*)g)[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) sumsq_add(gv[j], s[j], bad);
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) sumsq_add(g[n4 * 4 + threadIdx.x], s[0], bad);      // scalar tail
    double a[2] = {(s[0] + s[1]) + (s[2] + s[3]), bad};
    block_sums(a, lds, threadIdx.x);
    if (threadIdx.x < 2) partial[2 * (size_t)blockIdx.x + threadIdx.x] = a[0];
}

// one block: thread t adds partials t, t + 256, ... in index order, then the block's fixed tree.  n_parts == 0 writes {0, 0}.
__global__ __launch_bounds__(SUMSQ_THREADS) void grad_sumsq_finish_kernel(const double* __restrict__ partial, int n_parts,
                                                                          double* __restrict__ out) {
    __shared__ double lds[SUMSQ_THREADS / 64][2];
    double a[2] = {0.0, 0.0};
    for (int i = threadIdx.x; i < n_parts; i += SUMSQ_THREADS) {
        a[0] += partial[2 * i];
        a[1] += partial[2 * i + 1];
    }
    block_sums(a, lds, threadIdx.x);
    if (threadIdx.x < 2) out[threadIdx.x] = a[0];
}

__global__ __launch_bounds__(64) void optim_prepare_kernel(const double* __restrict__ sums, int n_groups, double max_norm, float lr,
                                                           double b1, double b2, hrn_optim_ctl* __restrict__ ctl) {
    if (threadIdx.x != 0) return;
    double total = 0.0, bad = 0.0;
    for (int k = 0; k < n_groups; ++k) {                         // index order
        total += sums[2 * k];
        bad += sums[2 * k + 1];
    }
    const double norm = sqrt(total);
    ctl->norm = norm;
    if (bad != 0.0) {                                            // counters and corrections stay where the last applied step left them
        ctl->skipped += 1;
        ctl->skip = 1;
        return;
    }
    const int64_t applied = ctl->applied + 1;
    double coef = 1.0;
    if (max_norm > 0.0) coef = fmin(1.0, max_norm / (norm + 1e-6));
    ctl->applied = applied;
    ctl->coef = (float)coef;
    ctl->step_size = (float)((double)lr / (1.0 - pow(b1, (double)applied)));
    ctl->inv_bc2_sqrt = (float)(1.0 / sqrt(1.0 - pow(b2, (double)applied)));
    ctl->lr = lr;
    ctl->skip = 0;
}

template <bool EMA>
__global__ __launch_bounds__(256) void adam_ex_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                      float* __restrict__ v, float* __restrict__ ema, size_t n, float b1, float b2, float eps,
                                                      float wd, int decoupled, float ema_decay, const hrn_optim_ctl* __restrict__ ctl) {
    if (ctl->skip) return;                                       // uniform: the whole grid leaves p, m, v and ema as they are
    const float coef = ctl->coef, step_size = ctl->step_size, inv_bc2_sqrt = ctl->inv_bc2_sqrt;
    const float wd_g = decoupled ? 0.f : wd;                     // coupled: L2 in the gradient
    // decoupled: p (1 - lr wd) - update = p - (lr wd p + update): the two small terms are added first, so p' is rounded once
    const float lr_wd = decoupled ? (float)((double)ctl->lr * (double)wd) : 0.f;
    const double d = (double)ema_decay;
    auto one = [&](float& pj, float gj, float& mj, float& vj, float& ej) {
        gj = fmaf(wd_g, pj, coef * gj);
        mj = b1 * mj + (1.f - b1) * gj;
        vj = b2 * vj + (1.f - b2) * gj * gj;
        pj -= fmaf(lr_wd, pj, step_size * mj / (sqrtf(vj) * inv_bc2_sqrt + eps));
        if (EMA) ej = (float)(d * (double)ej + (1.0 - d) * (double)pj);       // in fp64, rounded once
    };
    const size_t n4 = n / 4;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        f32x4 pv = ((f32x4*)p)[i], gv = ((const f32x4*)g)[i], mv = ((f32x4*)m)[i], vv = ((f32x4*)v)[i], ev = {0.f, 0.f, 0.f, 0.f};
        if (EMA) ev = ((f32x4*)ema)[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float pj = pv[j], mj = mv[j], vj = vv[j], ej = ev[j];
            one(pj, gv[j], mj, vj, ej);
            pv[j] = pj; mv[j] = mj; vv[j] = vj; ev[j] = ej;
        }
        ((f32x4*)p)[i] = pv; ((f32x4*)m)[i] = mv; ((f32x4*)v)[i] = vv;
        if (EMA) ((f32x4*)ema)[i] = ev;
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {              // scalar tail
        const size_t i = n4 * 4 + threadIdx.x;
        float pj = p[i], mj = m[i], vj = v[i], ej = EMA ? ema[i] : 0.f;
        one(pj, g[i], mj, vj, ej);
        p[i] = pj; m[i] = mj; v[i] = vj;
        if (EMA) ema[i] = ej;
    }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
bool beta_ok(float b) { return b >= 0.f && b < 1.f; }

}  // namespace

extern "C" size_t hrn_grad_sumsq_workspace_bytes(size_t n) { return sumsq_blocks(n) * 2 * sizeof(double); }

extern "C" int hrn_grad_sumsq(const float* grads, size_t n, double* out, void* ws, size_t ws_bytes, void* stream) {
    HRN_CHECK(grads || n == 0, -2, "hrn_grad_sumsq: grads is null");
    HRN_CHECK(out, -2, "hrn_grad_sumsq: out is null");
    HRN_CHECK(ws, -2, "hrn_grad_sumsq: ws is null");
    HRN_CHECK(aligned16(grads) && aligned16(ws) && aligned16(out), -2, "hrn_grad_sumsq: grads, out and ws must be 16-byte aligned");
    HRN_CHECK(ws_bytes >= hrn_grad_sumsq_workspace_bytes(n), -2, "hrn_grad_sumsq: ws_bytes too small (%zu < %zu)", ws_bytes,
              hrn_grad_sumsq_workspace_bytes(n));
    const size_t blocks = n ? sumsq_blocks(n) : 0;
    if (blocks) {
        hipLaunchKernelGGL(grad_sumsq_kernel, dim3((unsigned)blocks), dim3(SUMSQ_THREADS), 0, (hipStream_t)stream, grads, n, (double*)ws);
        HRN_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(grad_sumsq_finish_kernel, dim3(1), dim3(SUMSQ_THREADS), 0, (hipStream_t)stream, (const double*)ws, (int)blocks, out);
    HRN_LAUNCH_CHECK();
    return 0;
}

extern "C" int hrn_optim_prepare(const double* sums, int n_groups, int group, float max_norm, float lr, float beta1, float beta2,
                                 hrn_optim_ctl* ctl, void* stream) {
    HRN_CHECK(sums, -2, "hrn_optim_prepare: sums is null");
    HRN_CHECK(ctl, -2, "hrn_optim_prepare: ctl is null");
    HRN_CHECK(n_groups >= 1 && n_groups <= HRN_OPTIM_MAX_GROUPS, -2, "hrn_optim_prepare: n_groups must be in 1..%d (got %d)",
              HRN_OPTIM_MAX_GROUPS, n_groups);
    HRN_CHECK(group >= 0 && group < n_groups, -2, "hrn_optim_prepare: group must be in 0..%d (got %d)", n_groups - 1, group);
    HRN_CHECK(beta_ok(beta1), -2, "hrn_optim_prepare: beta1 must be in [0, 1) (got %g)", (double)beta1);
    HRN_CHECK(beta_ok(beta2), -2, "hrn_optim_prepare: beta2 must be in [0, 1) (got %g)", (double)beta2);
    HRN_CHECK(max_norm == max_norm, -2, "hrn_optim_prepare: max_norm is NaN");
    hipLaunchKernelGGL(optim_prepare_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, sums, n_groups, (double)max_norm, lr, (double)beta1,
                       (double)beta2, ctl + group);
    HRN_LAUNCH_CHECK();
    return 0;
}

extern "C" int hrn_adam_step_ex(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* ema_or_null, size_t n,
                                float beta1, float beta2, float eps, float weight_decay, int decoupled, float ema_decay,
                                const hrn_optim_ctl* ctl, void* stream) {
    HRN_CHECK(params, -2, "hrn_adam_step_ex: params is null");
    HRN_CHECK(grads, -2, "hrn_adam_step_ex: grads is null");
    HRN_CHECK(exp_avg, -2, "hrn_adam_step_ex: exp_avg is null");
    HRN_CHECK(exp_avg_sq, -2, "hrn_adam_step_ex: exp_avg_sq is null");
    HRN_CHECK(ctl, -2, "hrn_adam_step_ex: ctl is null");
    HRN_CHECK(beta_ok(beta1), -2, "hrn_adam_step_ex: beta1 must be in [0, 1) (got %g)", (double)beta1);
    HRN_CHECK(beta_ok(beta2), -2, "hrn_adam_step_ex: beta2 must be in [0, 1) (got %g)", (double)beta2);
    HRN_CHECK(!ema_or_null || beta_ok(ema_decay), -2, "hrn_adam_step_ex: ema_decay must be in [0, 1) (got %g)", (double)ema_decay);
    HRN_CHECK(aligned16(params) && aligned16(grads) && aligned16(exp_avg) && aligned16(exp_avg_sq) && aligned16(ema_or_null), -2,
              "hrn_adam_step_ex: the buffers must be 16-byte aligned");
    if (n == 0) return 0;
    size_t grid = (n / 4 + 255) / 256;
    if (grid < 1) grid = 1;
    if (grid > 4096) grid = 4096;
    if (ema_or_null)
        hipLaunchKernelGGL(adam_ex_kernel<true>, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, params, grads, exp_avg, exp_avg_sq,
                           ema_or_null, n, beta1, beta2, eps, weight_decay, decoupled, ema_decay, ctl);
    else
        hipLaunchKernelGGL(adam_ex_kernel<false>, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, params, grads, exp_avg, exp_avg_sq,
                           (float*)nullptr, n, beta1, beta2, eps, weight_decay, decoupled, ema_decay, ctl);
    HRN_LAUNCH_CHECK();
    return 0;
}
