// Guarded Adam step (include/pivp_optim.h): the L2 norms of the flat gradient buffer per parameter tensor, per gradient group and in total, Chainer's
// GradientClipping rate and a non-finite flag -- all from ONE read of the buffer -- and an Adam launch that takes its scale and its go / no-go from
// that device memory, so that neither clipping nor the skip of a poisoned step costs a host synchronisation.
//   pivp_grad_stats, three launches:
//     A  grad_granule_sums_kernel: every 16-lane group of a 256-thread block owns one 64-element GRANULE per iteration: a float4 per lane, fp64 from
//        the product gscale * g on, the lane's four squares added as (0 + 1) + (2 + 3), then the xor tree 8, 4, 2, 1 inside the 16 lanes.  One double
//        per granule goes to the workspace (3 % of the bytes read).  Segment ends are multiples of 64, so a granule never straddles two tensors, and a
//        granule's sum does not depend on which block or iteration formed it.
//     B  grad_segment_sums_kernel: one block per segment; thread t adds granules t, t + 256, ... of the segment in ascending order, then a 256-wide
//        halving tree in LDS.
//     C  grad_stats_finish_kernel: one wave; lane k adds the segments of group k in ascending order, lane 0 the groups in ascending order, forms rate
//        and the flag.
//   Every order above is a function of (n, segment table) alone and nothing is accumulated with atomics: same bytes in, same bits out.  NaN and +-inf
//   need no second pass: inf^2 = inf and NaN ride the sums into exactly the owning segment, its group and the total; a finite fp32 squared is at most
//   1.2e77, so no finite buffer can overflow the fp64 sums.
//   The read of g is the cost (HBM / MALL bound); the fp64 work is 3 flops per element.
//   adam_guarded_kernel is backward.hip's adam_kernel with gk = (g * gscale) * rate: the same operations in the same order, and * 1.0f is exact.
#include <math.h>

#include "../../include/pivp_hip.h"
#include "../../include/pivp_optim.h"
#include "pivp_common.h"

namespace pivp {

constexpr int GS_NT = 256;
constexpr int GS_GRAN = 64;                       // elements per granule = the alignment of every segment start
constexpr int GS_PER_BLOCK = GS_NT / 16;          // granules per block and iteration

__global__ __launch_bounds__(GS_NT) void grad_granule_sums_kernel(const float* __restrict__ g, long long n, long long granules, double gscale,
                                                                  double* __restrict__ gsum) {
    const int sub = threadIdx.x >> 4, l = threadIdx.x & 15;
    for (long long base = (long long)blockIdx.x * GS_PER_BLOCK; base < granules; base += (long long)gridDim.x * GS_PER_BLOCK) {
        const long long q = base + sub, i = q * GS_GRAN + l * 4;      // (the trip count is block-uniform: every lane takes part in the shuffles)
        float e0 = 0.f, e1 = 0.f, e2 = 0.f, e3 = 0.f;
        if (i + 3 < n) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(g + i);
            e0 = v[0]; e1 = v[1]; e2 = v[2]; e3 = v[3];
        } else {                                  // the buffer's last, partial float4 (or a granule past the end): zeros add nothing
            if (i < n) e0 = g[i];
            if (i + 1 < n) e1 = g[i + 1];
            if (i + 2 < n) e2 = g[i + 2];
        }
        const double a0 = (double)e0 * gscale, a1 = (double)e1 * gscale, a2 = (double)e2 * gscale, a3 = (double)e3 * gscale;
        double s = (a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3);
        s += __shfl_xor(s, 8, 16);
        s += __shfl_xor(s, 4, 16);
        s += __shfl_xor(s, 2, 16);
        s += __shfl_xor(s, 1, 16);
        if (l == 0 && q < granules) gsum[q] = s;
    }
}

__global__ __launch_bounds__(GS_NT) void grad_segment_sums_kernel(const double* __restrict__ gsum, const long long* __restrict__ seg_end, int ngroups,
                                                                  double* __restrict__ seg_sum, float* __restrict__ stats) {
    __shared__ double red[GS_NT];
    const int s = blockIdx.x, tid = threadIdx.x;
    const long long e0 = s ? seg_end[s - 1] : 0, e1 = seg_end[s];
    const long long q0 = e0 / GS_GRAN, q1 = (e1 + GS_GRAN - 1) / GS_GRAN;
    double a = 0.0;
    for (long long q = q0 + tid; q < q1; q += GS_NT) a += gsum[q];
    red[tid] = a;
    __syncthreads();
#pragma unroll
    for (int w = GS_NT / 2; w > 0; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    if (tid == 0) {
        seg_sum[s] = red[0];
        stats[PIVP_OPTIM_STATS_HEAD + ngroups + s] = (float)sqrt(red[0]);
    }
}

__global__ __launch_bounds__(64) void grad_stats_finish_kernel(const double* __restrict__ seg_sum, const int* __restrict__ seg_group, int nseg,
                                                               int ngroups, double threshold, float* __restrict__ stats) {
    __shared__ double group_sum[PIVP_GRAD_GROUPS];
    const int k = threadIdx.x;
    if (k < ngroups) {
        double a = 0.0;
        for (int s = 0; s < nseg; ++s)
            if (seg_group[s] == k) a += seg_sum[s];
        group_sum[k] = a;
        stats[PIVP_OPTIM_STATS_HEAD + k] = (float)sqrt(a);
    }
    __syncthreads();
    if (k == 0) {
        double t = 0.0;
        for (int i = 0; i < ngroups; ++i) t += group_sum[i];
        const double norm = sqrt(t), r = threshold / norm;
        stats[0] = (float)norm;
        stats[1] = (threshold > 0.0 && r < 1.0) ? (float)r : 1.0f;      // (a NaN quotient compares false: rate 1)
        stats[2] = __builtin_isfinite(t) ? 0.0f : 1.0f;
    }
}

__global__ __launch_bounds__(256) void adam_guarded_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                           float* __restrict__ v, long n, float lr_t, float omb1, float omb2, float eps,
                                                           float gscale, const float* __restrict__ stats, int skip_nonfinite,
                                                           int* __restrict__ skipped) {
    const float rate = stats[1];
    if (skip_nonfinite && stats[2] != 0.f) {      // grid-uniform: nobody writes p, m, v
        if (blockIdx.x == 0 && threadIdx.x == 0) *skipped = *skipped + 1;
        return;
    }
    for (long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4; i < n; i += (long)gridDim.x * 1024) {
        if (i + 3 < n) {
            f32x4 pp = *reinterpret_cast<f32x4*>(p + i), gg = *reinterpret_cast<const f32x4*>(g + i);
            f32x4 mm = *reinterpret_cast<f32x4*>(m + i), vv = *reinterpret_cast<f32x4*>(v + i);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float gk = (gg[k] * gscale) * rate;
                mm[k] += omb1 * (gk - mm[k]);
                vv[k] += omb2 * (gk * gk - vv[k]);
                pp[k] -= lr_t * mm[k] / (sqrtf(vv[k]) + eps);
            }
            *reinterpret_cast<f32x4*>(p + i) = pp; *reinterpret_cast<f32x4*>(m + i) = mm; *reinterpret_cast<f32x4*>(v + i) = vv;
        } else {
            for (long j = i; j < n; ++j) {
                const float gk = (g[j] * gscale) * rate;
                m[j] += omb1 * (gk - m[j]);
                v[j] += omb2 * (gk * gk - v[j]);
                p[j] -= lr_t * m[j] / (sqrtf(v[j]) + eps);
            }
        }
    }
}

static bool grad_stats_sizes_ok(long long n, int nseg) { return n >= 1 && nseg >= 1 && nseg <= PIVP_OPTIM_MAX_SEGMENTS; }
static long long grad_granules(long long n) { return (n + GS_GRAN - 1) / GS_GRAN; }

}  // namespace pivp

using namespace pivp;

extern "C" long long pivp_grad_stats_ws_bytes(long long n, int nseg) {
    if (!grad_stats_sizes_ok(n, nseg)) return PIVP_ERR_BADARG;
    return (grad_granules(n) + nseg) * (long long)sizeof(double);
}

extern "C" int pivp_grad_stats(const float* g, long long n, const long long* seg_end, const int* seg_group, int nseg, int ngroups, double gscale,
                               double threshold, void* ws, float* stats, void* stream) {
    PIVP_CHECK_ARG(g && seg_end && seg_group && ws && stats);
    PIVP_CHECK_ARG(grad_stats_sizes_ok(n, nseg) && ngroups >= 1 && ngroups <= PIVP_GRAD_GROUPS && __builtin_isfinite(gscale));
    PIVP_CHECK_ARG((reinterpret_cast<uintptr_t>(g) & 15) == 0 && (reinterpret_cast<uintptr_t>(ws) & 7) == 0);
    hipStream_t s = (hipStream_t)stream;
    const long long granules = grad_granules(n);
    double* gsum = static_cast<double*>(ws);
    double* seg_sum = gsum + granules;
    // the grid only shares the granules out: which block forms a granule's sum does not enter the sum
    const long long want = (granules + GS_PER_BLOCK - 1) / GS_PER_BLOCK, cap = 8ll * pivp_cu_count();
    hipLaunchKernelGGL(grad_granule_sums_kernel, dim3((unsigned)(want < cap ? want : cap)), dim3(GS_NT), 0, s, g, n, granules, gscale, gsum);
    hipLaunchKernelGGL(grad_segment_sums_kernel, dim3((unsigned)nseg), dim3(GS_NT), 0, s, gsum, seg_end, ngroups, seg_sum, stats);
    hipLaunchKernelGGL(grad_stats_finish_kernel, dim3(1), dim3(64), 0, s, seg_sum, seg_group, nseg, ngroups, threshold, stats);
    return PIVP_LAUNCH_STATUS();
}

extern "C" int pivp_adam_step_guarded(float* p, const float* g, float* m, float* v, long long n, double lr_t, double beta1, double beta2,
                                      double eps, double gscale, const float* stats, int skip_nonfinite, int* skipped, void* stream) {
    PIVP_CHECK_ARG(p && g && m && v && stats && n >= 1);
    PIVP_CHECK_ARG((skip_nonfinite == 0 || skip_nonfinite == 1) && (skipped || !skip_nonfinite));
    const long long want = (n / 4 + 255) / 256, blocks = want < 1 ? 1 : want < 4096 ? want : 4096;      // (n < 4: the tail loop of one thread)
    // the rounding of the host's scalars is adam_step's (backward.hip)
    hipLaunchKernelGGL(adam_guarded_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, g, m, v, (long)n,
                       (float)lr_t, (float)(1.0 - beta1), (float)(1.0 - beta2), (float)eps, (float)gscale, stats, skip_nonfinite, skipped);
    return PIVP_LAUNCH_STATUS();
}
