// Input gradients of the backward sweep (include/pivp_input_grad.h): d loss / d action of one timestep.
// enc3_state_bwd_kernel (backward_heads.hip) forms d sa[j] = W3s[j] . colsum + sum_o Wcs[o][j] d snew[o] for the ten smeared inputs of enc3 and keeps the
// state half (j = 5..9) as d state_prev; action_grad_kernel forms the action half (j = 0..4) from the same tensors, which that kernel leaves unmodified
// (it writes d e2 and parameter gradients only), so the two launches may run in either order behind the step's d e3 and d snew.
//   colsum[o]  = sum_p (e3[b,p,o] > 0 ? de3[b,p,o] : 0)                                                      (enc3's ReLU mask; 64 channels)
//   dact[b][j] = (use_state ? sum_o w3[64+j][o] colsum[o] : 0) + sum_o wcs[o*(A+S)+j] dsnew[b][o],  j = 0..A-1      (A = S = 5 on the reference's data)
// One 256-thread block per sample: thread (row group r = tid / 16, channel quad q = tid % 16) adds rows r, r + 16, ... of its four channels, a 16-byte
// load of de3 and one of e3 per row, four rows in flight; fp64 from the first add.  The sixteen row groups meet in a fixed tree in LDS, five threads
// finish the two dot products in fp64 in ascending o and round once.  No atomics, no workspace: the value of sample b depends on that sample's bytes, on
// (HW8, use_state) and on the weights alone -- not on B, the stride or the plan's mode.  16 KB per sample at 64 x 64 frames: the launch is its cost.
#include "../../include/pivp_hip.h"
#include "../../include/pivp_input_grad.h"
#include "pivp_common.h"
#include "pivp_kernels.h"

namespace pivp {

__global__ __launch_bounds__(256) void action_grad_kernel(const float* __restrict__ e3, const float* __restrict__ de3, int ldd3,
                                                          const float* __restrict__ w3, const float* __restrict__ wcs,
                                                          const float* __restrict__ dsnew, float* __restrict__ dact, int HW8, int use_state, int A, int S) {
    __shared__ double red[16 * 64];
    __shared__ double colsum[64];
    const int b = blockIdx.x, tid = threadIdx.x, rg = tid >> 4, cq = (tid & 15) * 4;
    const float* const yb = e3 + (size_t)b * HW8 * 64 + cq;
    const float* const db = de3 + (size_t)b * HW8 * ldd3 + cq;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
    for (int p0 = rg; p0 < HW8; p0 += 64) {      // four rows of this row group per pass: eight independent 16-B loads
        f32x4 y[4], d[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int p = p0 + 16 * u;
            const bool ok = p < HW8;
            y[u] = ok ? *reinterpret_cast<const f32x4*>(yb + (size_t)p * 64) : z4;
            d[u] = ok ? *reinterpret_cast<const f32x4*>(db + (size_t)p * ldd3) : z4;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)      // ascending rows: the order is a function of HW8 alone
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] += y[u][e] > 0.f ? (double)d[u][e] : 0.0;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) red[rg * 64 + cq + e] = acc[e];
    __syncthreads();
    if (tid < 64) {      // the sixteen row groups of channel tid: ((0 + 1) + (2 + 3)) + ... as a halving tree
        double v[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) v[r] = red[r * 64 + tid];
#pragma unroll
        for (int w = 8; w >= 1; w >>= 1)
#pragma unroll
            for (int r = 0; r < w; ++r) v[r] = v[2 * r] + v[2 * r + 1];
        colsum[tid] = v[0];
    }
    __syncthreads();
    if (tid < A) {
        double v = 0.0;
        if (use_state) for (int o = 0; o < 64; ++o) v += (double)w3[(64 + tid) * 64 + o] * colsum[o];
        double u = 0.0;
        for (int o = 0; o < S; ++o) u += (double)wcs[o * (A + S) + tid] * (double)dsnew[b * S + o];
        dact[b * A + tid] = (float)(v + u);
    }
}

int action_grad(const float* e3, const float* de3, int ldd3, const float* w3, const float* wcs, const float* dsnew, float* dact, int B, int HW8,
                int use_state, hipStream_t s, int A, int S) {
    PIVP_CHECK_ARG(e3 && de3 && wcs && dsnew && dact && (w3 || !use_state) && B > 0 && HW8 > 0 && ldd3 >= 64 && ldd3 % 4 == 0 && smear_dims_ok(A, S));
    PIVP_CHECK_ARG(!((reinterpret_cast<uintptr_t>(e3) | reinterpret_cast<uintptr_t>(de3)) & 15));
    PIVP_CHECK_ARG(!((reinterpret_cast<uintptr_t>(w3) | reinterpret_cast<uintptr_t>(wcs) | reinterpret_cast<uintptr_t>(dsnew) |
                      reinterpret_cast<uintptr_t>(dact)) & 3));
    hipLaunchKernelGGL(action_grad_kernel, dim3(B), dim3(256), 0, s, e3, de3, ldd3, w3, wcs, dsnew, dact, HW8, use_state, A, S);
    return PIVP_LAUNCH_STATUS();
}

}  // namespace pivp

extern "C" int pivp_action_grad(const float* e3, const float* de3, int ldd3, const float* w3, const float* wcs, const float* dsnew, float* dact,
                                int B, int HW8, int use_state, void* stream) {
    return pivp::action_grad(e3, de3, ldd3, w3, wcs, dsnew, dact, B, HW8, use_state != 0, (hipStream_t)stream);
}
