// The coarse-to-fine masked-NCC search for shifts beyond one search's reach (the definitions are in
// include/hrnet_hip.h): a masked image pyramid by reduce2, and the scene search of registration_scene.hip per octave, the coarsest from
// (0, 0) and every finer one from twice the shift of the octave above.  New device code here is only the reduction and the doubling; the
// level and finish kernels are registration_scene.hip's, through its launcher, untouched.
//
// reduce2.  A workgroup of 256 threads owns R2_TY x R2_TX = 16 x 64 pixels of one coarse plane.  It stages their fine window - rows
// 2 Y0 - 1 .. 2 Y0 + 2 R2_TY, columns 2 X0 - 1 .. 2 X0 + 2 R2_TX, that is 34 x 130 - in LDS: the values as they are (0 outside the frame)
// and one byte per pixel for "inside the frame and clear".  The path of a window row is chosen PER ROW AND PER PLANE POINTER from the
// address of its first element, as tile.hip's copy_row does: the h = (4 - address / 4 mod 4) mod 4 elements in front of the first 16-byte
// boundary one by one, then 16-byte loads where the four elements lie inside the frame and the window, 4-byte loads where they do not
// (the frame's borders, the window's end).  Image and mask are staged by the same routine, each by its own alignment.  The kernel is
// bound by bytes - 8 H W read with a mask, 4 H W without, 2 H W written - and every fine pixel is read by one workgroup only, except the
// one-pixel apron around a tile (130 x 34 / (128 x 32) = 1.08 of the floor, from L2 for the most part).
//
// A thread then forms four coarse pixels (rows ty + 4 k, column tx) out of LDS, each from its 4 x 4 taps as two 8-byte reads per row,
// which consecutive lanes take from consecutive banks.  The arithmetic of a pixel, in this order and with contraction off:
//     den = 0, num = 0;  for a = 0..3 (rows), for b = 0..3 (columns):  w = w_a w_b (exact),  den = den + w m,  num = fmaf(w, m ? x : 0, num)
//     clear = den > 0.5;  value = clear ? num / den : 0
// den adds multiples of 1/64 up to 1 and is exact; a masked x never enters num (a NaN under the mask stays there).  Stores are 4 bytes a
// lane, 256 bytes a wave and row.  No atomics, nothing depends on the launch: two runs agree bit for bit.
//
// Resources (gfx950, -Rpass-analysis=kernel-resource-usage): see DESIGN.md section 7j.
#include "kernels.h"
#include "mncc_common.h"            // for turning fp contraction off; none of its functions is used here

namespace {

constexpr int R2_TY = 16, R2_TX = 64, R2_THREADS = 256;
constexpr int R2_ROWS = 2 * R2_TY + 2, R2_COLS = 2 * R2_TX + 2;        // the fine window: 34 x 130
constexpr int R2_PITCH = R2_COLS + 2;                                  // 132: rows stay 8-byte aligned in LDS
constexpr int R2_SLOTS = (R2_COLS + 3) / 4 + 1;                        // 16-byte slots of a window row after any head h <= 3; the last slot is the head's
constexpr int R2_PER_THREAD = R2_TY * R2_TX / R2_THREADS;              // 4 coarse pixels a thread
static_assert(R2_TX == 64 && R2_THREADS / 64 * R2_PER_THREAD == R2_TY, "a lane per coarse column, the waves interleaved over the rows");
static_assert(R2_PITCH % 2 == 0, "ds_read_b64 of a column pair");

struct Reduce2Shared {
    float x[R2_ROWS * R2_PITCH];
    unsigned char m[R2_ROWS * R2_PITCH];
};

// One 16-byte slot (or the head) of one window row of one plane into LDS.  `row` points at the frame's row (nullptr: the row lies outside
// the frame), fx0 is the frame column of window column 0.  MASK: dst is the byte array and gets (value != 0); a null plane with MASK
// means all clear.  Out of the frame: 0.
template <bool MASK>
__device__ __forceinline__ void stage_slot(const float* __restrict__ plane, bool have_plane, size_t row_off, bool row_in, int fx0, int W,
                                           int slot, float* __restrict__ dx, unsigned char* __restrict__ dm) {
    // the address of window column 0 in units of 4 bytes, mod 4; taken on integers: column fx0 may be -1
    const long long a0 = (long long)((uintptr_t)plane >> 2) + (long long)row_off + (long long)fx0;
    const int h = have_plane ? (int)((4u - (unsigned)(a0 & 3)) & 3u) : 0;
    int e0, e1;
    if (slot == R2_SLOTS - 1) { e0 = 0; e1 = h; }                      // the head, one by one
    else { e0 = h + 4 * slot; e1 = e0 + 4 < R2_COLS ? e0 + 4 : R2_COLS; }
    if (e0 >= e1) return;
    const bool whole = row_in && have_plane && e1 - e0 == 4 && fx0 + e0 >= 0 && fx0 + e0 + 3 < W;
    if (whole) {
        const f32x4 v = *(const f32x4*)(plane + row_off + (size_t)(fx0 + e0));
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (MASK) dm[e0 + e] = v[e] != 0.f;
            else dx[e0 + e] = v[e];
        }
        return;
    }
    for (int e = e0; e < e1; ++e) {
        const int x = fx0 + e;
        const bool in = row_in && x >= 0 && x < W;
        if (MASK) dm[e] = in && (have_plane ? plane[row_off + (size_t)x] != 0.f : true);
        else dx[e] = in ? plane[row_off + (size_t)x] : 0.f;
    }
}

// Planes 0 .. na - 1 are a's (the views), na .. na + nb - 1 are b's (the references); a mask pointer may be null (all clear).
// out / out_mask: (H / 2, W / 2) per plane.  grid (planes * tiles), tiles = tiles_x * tiles_y
__global__ __launch_bounds__(R2_THREADS) void reduce2_kernel(const float* __restrict__ a, const float* __restrict__ a_mask, unsigned na,
                                                             const float* __restrict__ b, const float* __restrict__ b_mask, int H, int W,
                                                             unsigned tiles_x, unsigned tiles, float* __restrict__ a_out,
                                                             float* __restrict__ a_out_mask, float* __restrict__ b_out,
                                                             float* __restrict__ b_out_mask) {
    __shared__ Reduce2Shared S;
    const int tid = threadIdx.x;
    const unsigned plane = blockIdx.x / tiles, tile = blockIdx.x - plane * tiles;
    const bool second = plane >= na;
    const size_t p = second ? plane - na : plane, hw = (size_t)H * W;
    const int Ho = H / 2, Wo = W / 2;
    const size_t hwo = (size_t)Ho * Wo;
    const float* img = (second ? b : a) + p * hw;
    const float* msk = second ? b_mask : a_mask;
    const bool have_mask = msk != nullptr;
    if (have_mask) msk += p * hw;
    float* out = (second ? b_out : a_out) + p * hwo;
    float* out_mask = (second ? b_out_mask : a_out_mask) + p * hwo;
    const int Y0 = (int)(tile / tiles_x) * R2_TY, X0 = (int)(tile % tiles_x) * R2_TX;
    const int fy0 = 2 * Y0 - 1, fx0 = 2 * X0 - 1;

    for (int i = tid; i < R2_ROWS * R2_SLOTS; i += R2_THREADS) {
        const int wy = i / R2_SLOTS, slot = i - wy * R2_SLOTS;
        const int y = fy0 + wy;
        const bool row_in = y >= 0 && y < H;
        const size_t row_off = row_in ? (size_t)y * W : 0;
        stage_slot<false>(img, true, row_off, row_in, fx0, W, slot, S.x + wy * R2_PITCH, nullptr);
        stage_slot<true>(msk, have_mask, row_off, row_in, fx0, W, slot, nullptr, S.m + wy * R2_PITCH);
    }
    __syncthreads();

    const int tx = tid & 63, ty = tid >> 6, X = X0 + tx;
    if (X >= Wo) return;
    const float wt[4] = {0.125f, 0.375f, 0.375f, 0.125f};
#pragma unroll
    for (int k = 0; k < R2_PER_THREAD; ++k) {
        const int yl = ty + (R2_THREADS / 64) * k, Y = Y0 + yl;
        if (Y >= Ho) break;
        float den = 0.f, num = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int at = (2 * yl + r) * R2_PITCH + 2 * tx;
            const float2 x01 = *(const float2*)(S.x + at), x23 = *(const float2*)(S.x + at + 2);
            const uchar2 m01 = *(const uchar2*)(S.m + at), m23 = *(const uchar2*)(S.m + at + 2);
            const float xs[4] = {x01.x, x01.y, x23.x, x23.y};
            const bool ms[4] = {m01.x != 0, m01.y != 0, m23.x != 0, m23.y != 0};
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float w = wt[r] * wt[c];
                den = den + w * (ms[c] ? 1.f : 0.f);
                num = fmaf(w, ms[c] ? xs[c] : 0.f, num);
            }
        }
        const bool clear = den > 0.5f;
        const size_t o = (size_t)Y * Wo + X;
        out[o] = clear ? num / den : 0.f;
        out_mask[o] = clear ? 1.f : 0.f;
    }
}

// out[i] = 2 in[i]: the shift of an octave in the pixels of the octave below.  Exact in fp32.  n = 2 B V
__global__ __launch_bounds__(256) void double_kernel(const float* __restrict__ in, float* __restrict__ out, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) out[i] = 2.f * in[i];
}

struct Reduce2Plan { unsigned tiles_x, tiles; };

Reduce2Plan reduce2_plan(int H, int W) {
    Reduce2Plan p;
    p.tiles_x = (unsigned)((W / 2 + R2_TX - 1) / R2_TX);
    p.tiles = p.tiles_x * (unsigned)((H / 2 + R2_TY - 1) / R2_TY);
    return p;
}

size_t align16(size_t x) { return (x + 15) / 16 * 16; }

// the four reduced tensors of octave k (1..K) of a pyramid over (B, V, H, W): views, their masks, references, their masks
struct Octave {
    int H, W;
    float *views, *view_masks, *ref, *ref_mask;
    size_t bytes;                                  // of the four, rounded up to 16
};

Octave octave_at(unsigned char* base, int B, int V, int H, int W, int k) {
    Octave o;
    o.H = H >> k; o.W = W >> k;
    const size_t hw = (size_t)o.H * o.W, bv = (size_t)B * V;
    o.views = reinterpret_cast<float*>(base);
    o.view_masks = o.views + bv * hw;
    o.ref = o.view_masks + bv * hw;
    o.ref_mask = o.ref + (size_t)B * hw;
    o.bytes = align16(4 * 2 * (bv + (size_t)B) * hw);
    return o;
}

}  // namespace

bool hrn_mncc_reduce2_grid_fits(size_t planes, int H, int W) {
    return (double)planes * reduce2_plan(H, W).tiles <= 2147483647.0;
}

int hrn_launch_mncc_reduce2(const float* a, const float* a_mask, size_t na, const float* b, const float* b_mask, size_t nb, int H, int W,
                            float* a_out, float* a_out_mask, float* b_out, float* b_out_mask, hipStream_t stream) {
    const Reduce2Plan p = reduce2_plan(H, W);
    const double planes = (double)(na + nb), hw = (double)H * W;
    HrnProfScope prof("mncc_reduce2", 2.0 * 32.0 * planes * hw / 4.0, 4.0 * planes * hw * (1.0 + (a_mask ? 1.0 : 0.0) + 0.5), stream);
    hipLaunchKernelGGL(reduce2_kernel, dim3((unsigned)(na + nb) * p.tiles), dim3(R2_THREADS), 0, stream, a, a_mask, (unsigned)na, b, b_mask, H, W,
                       p.tiles_x, p.tiles, a_out, a_out_mask, b_out, b_out_mask);
    HRN_LAUNCH_CHECK();
    return 0;
}

size_t hrn_mncc_pyramid_workspace_bytes_impl(int B, int V, int H, int W, int P, int octaves) {
    size_t bytes = 0;
    for (int k = 1; k <= octaves; ++k) bytes += octave_at(nullptr, B, V, H, W, k).bytes;
    return bytes + align16(hrn_mncc_scene_workspace_bytes_impl(B, V, H, W, P)) + 16 * (size_t)B * V;
}

int hrn_launch_mncc_search_pyramid(const float* ref, const float* ref_mask, const float* views, const float* view_masks, int B, int V, int H,
                                   int W, int P, int octaves, int levels, float radius, int coarse_levels, float refine_radius, float* shifts,
                                   float* trace, void* workspace, hipStream_t stream) {
    unsigned char* base = static_cast<unsigned char*>(workspace);
    Octave oct[HRN_MNCC_MAX_OCTAVES + 1];
    oct[0].H = H; oct[0].W = W;
    oct[0].views = const_cast<float*>(views); oct[0].view_masks = const_cast<float*>(view_masks);
    oct[0].ref = const_cast<float*>(ref); oct[0].ref_mask = const_cast<float*>(ref_mask);
    const size_t bv = (size_t)B * V;
    for (int k = 1; k <= octaves; ++k) {
        oct[k] = octave_at(base, B, V, H, W, k);
        base += oct[k].bytes;
        const Octave& f = oct[k - 1];
        if (int rc = hrn_launch_mncc_reduce2(f.views, f.view_masks, bv, f.ref, f.ref_mask, (size_t)B, f.H, f.W, oct[k].views, oct[k].view_masks,
                                             oct[k].ref, oct[k].ref_mask, stream))
            return rc;
    }
    void* scene_ws = base;                               // every octave's search carves its own, smaller, plan out of the base size's bytes
    base += align16(hrn_mncc_scene_workspace_bytes_impl(B, V, H, W, P));
    float* found = reinterpret_cast<float*>(base);       // an octave's shifts, and twice them: the centre of the octave below
    float* start = found + 2 * bv;
    const unsigned blocks = (unsigned)((2 * bv + 255) / 256 < 1024 ? (2 * bv + 255) / 256 : 1024);
    for (int k = octaves; k >= 0; --k) {
        const Octave& o = oct[k];
        const bool top = k == octaves;
        if (!top) {
            hipLaunchKernelGGL(double_kernel, dim3(blocks), dim3(256), 0, stream, (const float*)found, start, 2 * bv);
            HRN_LAUNCH_CHECK();
        }
        if (int rc = hrn_launch_mncc_search_scene_from(o.ref, o.ref_mask, o.views, o.view_masks, top ? (const float*)nullptr : start, B, V, o.H, o.W,
                                                       P, k == 0 ? levels : coarse_levels, top ? radius : refine_radius, k == 0 ? shifts : found,
                                                       (float*)nullptr, trace ? trace + 3 * (octaves - k) : (float*)nullptr, 3 * (octaves + 1),
                                                       scene_ws, stream))
            return rc;
    }
    return 0;
}
