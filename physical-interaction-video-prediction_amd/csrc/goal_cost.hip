// Planning on a goal image (include/pivp_goal_cost.h): the weighted squared / absolute error of S x K predicted frames [S][K][3][H][W] to a goal
// image, per frame and folded over the steps, and its gradient with respect to the frames.  Two launches, in the manner of plan_cost (csrc/cem.hip):
//   goal_cost_kernel<VEC, GRAD>   one 256-thread block per (s, k) frame.  It walks channel by channel in groups of four consecutive pixels, group g
//                to thread g % 256: the order of a thread's sum is the same for the 16-byte form (VEC: H*W % 4 == 0 and every pointer on 16 bytes) and
//                the element-wise form, and therefore so are the bits.  Up to 1024 groups per channel (64 x 64) a thread's twelve frame loads are all
//                requested before the first use; the goal (48 KB) and the weights come from L2.  fp64 from the first difference: per-thread sums,
//                the xor-butterfly wave sum, waves in ascending order through LDS, one rounding to fp32.  The gradient goes out with plain stores,
//                every element written by one thread; a frame whose sum is not finite has its gradient rewritten as zeros by the same threads.
//   goal_cost_finish_kernel       one thread per candidate folds the steps in ascending order, in double.
// No atomics, no workspace: the same bits on every launch.  Memory bound: S*K*3*H*W*4 bytes read (14 MB at S = 9, K = 32, 64 x 64), as much again
// written with the gradient.  Stream-ordered, no host synchronisation.
#include <math.h>

#include "../../include/pivp_goal_cost.h"
#include "pivp_kernels.h"

namespace pivp {

constexpr int GC_NT = 256;
constexpr int GC_R = 4;                           // groups per thread and channel requested together
constexpr int GC_STRIDE = 4 * GC_NT;              // a thread's next group lies 1024 pixels on

struct GoalCostArgs {
    const float* frames; const float* goal; const float* pixel_w; const float* step_w;
    float* per_step; float* grad;
    double inv_norm, w_mse, w_l1, scale;
    float bad_cost;
    int per_sample_goal, K, HW;
};

template <bool VEC>
__device__ __forceinline__ f32x4 gc_load(const float* __restrict__ p, int i0, int HW) {
    f32x4 q = {0.f, 0.f, 0.f, 0.f};
    if (VEC) {
        if (i0 < HW) q = *reinterpret_cast<const f32x4*>(p + i0);      // (H*W % 4 == 0: a group is inside the channel or outside it)
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) if (i0 + e < HW) q[e] = p[i0 + e];
    }
    return q;
}

__device__ __forceinline__ double gc_wave_sum(double v) {      // the xor butterfly: every lane ends with the same sum, formed in the same order
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

template <bool VEC, bool GRAD>
__global__ __launch_bounds__(GC_NT) void goal_cost_kernel(GoalCostArgs a) {
    __shared__ double red[GC_NT / 64];
    __shared__ int bad_frame;
    const int tid = threadIdx.x, HW = a.HW;
    const int b = blockIdx.x;                          // s * K + k
    const int s = b / a.K, k = b - s * a.K;
    const size_t frame = (size_t)3 * HW;
    const float* __restrict__ fr = a.frames + (size_t)b * frame;
    const float* __restrict__ gl = a.goal + (a.per_sample_goal ? (size_t)k * frame : 0);
    const float* __restrict__ pw = a.pixel_w;
    float* __restrict__ go = GRAD ? a.grad + (size_t)b * frame : nullptr;
    const double gfac = GRAD ? a.scale * (double)a.step_w[s] * a.inv_norm : 0.0;
    const double k2 = 2.0 * a.w_mse;
    double acc = 0.0;

    // one group of one channel: the goal and the weights are read here (L2 hits), the frame's four values arrive in `f`
    auto group = [&](int c, int i0, const f32x4& f) {
        if (i0 >= HW) return;
        const f32x4 g = gc_load<VEC>(gl + (size_t)c * HW, i0, HW);
        f32x4 w = {1.f, 1.f, 1.f, 1.f};
        if (pw) w = gc_load<VEC>(pw, i0, HW);
        f32x4 out = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (VEC || i0 + e < HW) {
                const double d = (double)f[e] - (double)g[e], we = (double)w[e];
                acc += we * (a.w_mse * (d * d) + a.w_l1 * fabs(d));
                if (GRAD) {
                    const double sg = d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 0.0);
                    out[e] = (float)(gfac * we * (k2 * d + a.w_l1 * sg));
                }
            }
        }
        if (GRAD) {
            float* o = go + (size_t)c * HW + i0;
            if (VEC) *reinterpret_cast<f32x4*>(o) = out;
            else {
#pragma unroll
                for (int e = 0; e < 4; ++e) if (i0 + e < HW) o[e] = out[e];
            }
        }
    };

    if (HW <= GC_R * GC_STRIDE) {      // (block-uniform) the whole frame in twelve requests per thread, all in flight before the first use
        f32x4 f[3][GC_R];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
#pragma unroll
            for (int j = 0; j < GC_R; ++j) f[c][j] = gc_load<VEC>(fr + (size_t)c * HW, tid * 4 + j * GC_STRIDE, HW);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
#pragma unroll
            for (int j = 0; j < GC_R; ++j) group(c, tid * 4 + j * GC_STRIDE, f[c][j]);
        }
    } else {                           // larger frames: the same order (channel, then group), four requests at a time
        for (int c = 0; c < 3; ++c) {
            for (int i0 = tid * 4; i0 < HW; i0 += GC_R * GC_STRIDE) {
                f32x4 f[GC_R];
#pragma unroll
                for (int j = 0; j < GC_R; ++j) f[j] = gc_load<VEC>(fr + (size_t)c * HW, i0 + j * GC_STRIDE, HW);
#pragma unroll
                for (int j = 0; j < GC_R; ++j) group(c, i0 + j * GC_STRIDE, f[j]);
            }
        }
    }

    acc = gc_wave_sum(acc);
    if ((tid & 63) == 0) red[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
        double t = 0.0;
#pragma unroll
        for (int i = 0; i < GC_NT / 64; ++i) t += red[i];
        const float v = (float)(a.inv_norm * t);
        const bool ok = v == v && fabsf(v) <= 3.4028234e38f;
        a.per_step[b] = ok ? v : a.bad_cost;
        bad_frame = ok ? 0 : 1;
    }
    if (GRAD) {
        __syncthreads();
        if (bad_frame) {               // a diverged frame: every thread rewrites the elements it wrote
            for (int c = 0; c < 3; ++c) {
                for (int i0 = tid * 4; i0 < HW; i0 += GC_STRIDE) {
                    float* o = go + (size_t)c * HW + i0;
                    if (VEC) *reinterpret_cast<f32x4*>(o) = f32x4{0.f, 0.f, 0.f, 0.f};
                    else {
#pragma unroll
                        for (int e = 0; e < 4; ++e) if (i0 + e < HW) o[e] = 0.f;
                    }
                }
            }
        }
    }
}

__global__ __launch_bounds__(GC_NT) void goal_cost_finish_kernel(const float* __restrict__ per_step, const float* __restrict__ step_w, double scale,
                                                                 int accumulate, float* __restrict__ cost, int S, int K) {
    const int k = blockIdx.x * GC_NT + threadIdx.x;
    if (k >= K) return;
    double c = 0.0;
    for (int s = 0; s < S; ++s) c += (double)step_w[s] * (double)per_step[(size_t)s * K + k];
    cost[k] = (float)((accumulate ? (double)cost[k] : 0.0) + scale * c);
}

static bool gc_finite(float v) { return v == v && fabsf(v) <= 3.4028234e38f; }

}  // namespace pivp

using namespace pivp;

extern "C" int pivp_goal_image_cost(const float* frames, const float* goal, int G, const float* pixel_w, float inv_norm, const float* step_w,
                                    float w_mse, float w_l1, float bad_cost, float scale, int accumulate, float* cost, float* per_step, float* grad,
                                    int S, int K, int H, int W, void* stream) {
    PIVP_CHECK_ARG(frames && goal && step_w && cost && per_step);
    PIVP_CHECK_ARG(S >= 1 && K >= 1 && H > 1 && W > 1 && W + 4 <= 256 && H <= 32768 && (G == 1 || G == K));
    PIVP_CHECK_ARG((long long)S * K < (1ll << 31) && (long long)S * K * 3 * H * W < (1ll << 40));
    PIVP_CHECK_ARG(gc_finite(w_mse) && gc_finite(w_l1) && gc_finite(bad_cost) && gc_finite(scale) && gc_finite(inv_norm) && inv_norm > 0.f);
    const uintptr_t big = reinterpret_cast<uintptr_t>(frames) | reinterpret_cast<uintptr_t>(goal) | reinterpret_cast<uintptr_t>(grad) |
                          reinterpret_cast<uintptr_t>(pixel_w);
    PIVP_CHECK_ARG(((big | reinterpret_cast<uintptr_t>(step_w) | reinterpret_cast<uintptr_t>(cost) | reinterpret_cast<uintptr_t>(per_step)) & 3) == 0);
    hipStream_t s = (hipStream_t)stream;
    GoalCostArgs a;
    a.frames = frames; a.goal = goal; a.pixel_w = pixel_w; a.step_w = step_w; a.per_step = per_step; a.grad = grad;
    a.inv_norm = (double)inv_norm; a.w_mse = (double)w_mse; a.w_l1 = (double)w_l1; a.scale = (double)scale;
    a.bad_cost = bad_cost; a.per_sample_goal = G != 1; a.K = K; a.HW = H * W;
    const bool vec = ((H * W) & 3) == 0 && (big & 15) == 0;      // every frame, goal and channel then starts on 16 bytes
    const dim3 grid(S * K), block(GC_NT);
    if (vec) {
        if (grad) hipLaunchKernelGGL((goal_cost_kernel<true, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((goal_cost_kernel<true, false>), grid, block, 0, s, a);
    } else {
        if (grad) hipLaunchKernelGGL((goal_cost_kernel<false, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((goal_cost_kernel<false, false>), grid, block, 0, s, a);
    }
    if (hipGetLastError() != hipSuccess) return PIVP_ERR_LAUNCH;
    hipLaunchKernelGGL(goal_cost_finish_kernel, dim3((K + GC_NT - 1) / GC_NT), dim3(GC_NT), 0, s, per_step, step_w, (double)scale, accumulate, cost, S,
                       K);
    return PIVP_LAUNCH_STATUS();
}
