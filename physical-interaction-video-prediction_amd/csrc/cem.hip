// Planning on the device (Finn & Levine 2017, visual MPC): the two ops `planning.cem_plan` puts around pivp_rollout_predict.
//   plan_cost    expected-distance cost of the tracked planes, each plane read ONCE: one block per (step, candidate, plane) forms the two moments
//                sum(d) and sum(d * |pix - goal|) -- the distance is computed from the pixel's index, nothing but the plane comes from HBM --, a second
//                small launch folds the per-plane expected distances into cost[K].  Memory bound: S*K*P*H*W*4 bytes (4.7 MB at S = 9, K = 32, P = 1, 64 x 64).
//   cem_update   one refit + resample of the cross-entropy method in ONE workgroup (K <= 1024): rank by counting, elite mean / std, the blend with
//                the previous distribution, the best-so-far record, then Philox4x32-10 + Box-Muller samples.  Launch-latency bound.
// Both: fp32 in and out, a fixed summation order (per-thread strided sums, the xor-butterfly wave_sum, waves in ascending order), no atomics: the same
// bits on every launch.  Stream-ordered, no host synchronisation.
#include <math.h>

#include "cem_noise.h"
#include "cem_refit.h"
#include "pivp_kernels.h"

namespace pivp {

constexpr int PC_NT = 256;
constexpr int PC_MAXP = 8;

__global__ __launch_bounds__(PC_NT) void plan_moments_kernel(const float* __restrict__ track, const float* __restrict__ goals, float miss_cost,
                                                             float* __restrict__ mass, float* __restrict__ edist, int P, int W, int HW) {
    __shared__ float red[2][PC_NT / 64];
    const int b = blockIdx.x;                          // (s * K + k) * P + p
    const int p = b % P;
    const float* __restrict__ pl = track + (size_t)b * HW;
    const float gr = goals[2 * p], gc = goals[2 * p + 1];
    const bool vec = (HW & 3) == 0 && (reinterpret_cast<uintptr_t>(track) & 15) == 0;      // every plane then starts on a 16-byte boundary
    float m0 = 0.f, m1 = 0.f;
    // groups of four consecutive pixels, group g to thread g % 256: the order of a thread's sum is the same for the vector and the scalar form
    const int qstep = (4 * PC_NT) / W, rstep = (4 * PC_NT) - qstep * W;      // a thread's next group lies 1024 pixels on: no division in the loop
    int y0 = (threadIdx.x * 4) / W, x0 = threadIdx.x * 4 - y0 * W;
    for (int i0 = threadIdx.x * 4; i0 < HW; i0 += 4 * PC_NT) {
        float v[4];
        if (vec) {
            const f32x4 q = *reinterpret_cast<const f32x4*>(pl + i0);
            v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = i0 + e < HW ? pl[i0 + e] : 0.f;
        }
        int y = y0, x = x0;
        y0 += qstep; x0 += rstep;
        if (x0 >= W) { x0 -= W; ++y0; }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float dr = (float)y - gr, dc = (float)x - gc;
            const float dist = sqrtf(dr * dr + dc * dc);
            m0 += v[e];
            m1 += v[e] * dist;
            if (++x == W) { x = 0; ++y; }
        }
    }
    m0 = wave_sum(m0);
    m1 = wave_sum(m1);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[0][w] = m0; red[1][w] = m1; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float t0 = 0.f, t1 = 0.f;
#pragma unroll
        for (int i = 0; i < PC_NT / 64; ++i) { t0 += red[0][i]; t1 += red[1][i]; }
        const bool ok = t0 > 0.f && t0 <= 3.4028234e38f;      // false for NaN, +inf, zero and negative mass
        mass[b] = t0;
        edist[b] = ok ? t1 / t0 : miss_cost;
    }
}

__global__ __launch_bounds__(PC_NT) void plan_cost_finish_kernel(const float* __restrict__ edist, const float* __restrict__ step_w,
                                                                 const float* __restrict__ plane_w, float* __restrict__ cost, int S, int K, int P) {
    const int k = blockIdx.x * PC_NT + threadIdx.x;
    if (k >= K) return;
    float c = 0.f;
    for (int s = 0; s < S; ++s) {
        float cs = 0.f;
        for (int p = 0; p < P; ++p) cs += plane_w[p] * edist[((size_t)s * K + k) * P + p];
        c += step_w[s] * cs;
    }
    cost[k] = c;
}

int plan_cost(const float* track, const float* goals, const float* step_w, const float* plane_w, float miss_cost, float* cost, float* mass,
              float* edist, int S, int K, int P, int H, int W, hipStream_t s) {
    PIVP_CHECK_ARG(track && goals && step_w && plane_w && cost && mass && edist);
    PIVP_CHECK_ARG(S >= 1 && K >= 1 && P >= 1 && P <= PC_MAXP && H > 1 && W > 1 && W + 4 <= 256 && H <= 32768);
    PIVP_CHECK_ARG(miss_cost == miss_cost && fabsf(miss_cost) <= 3.4028234e38f);
    PIVP_CHECK_ARG((long long)S * K * P < (1ll << 31) && (long long)S * K * P * H * W < (1ll << 40));
    hipLaunchKernelGGL(plan_moments_kernel, dim3(S * K * P), dim3(PC_NT), 0, s, track, goals, miss_cost, mass, edist, P, W, H * W);
    hipLaunchKernelGGL(plan_cost_finish_kernel, dim3((K + PC_NT - 1) / PC_NT), dim3(PC_NT), 0, s, edist, step_w, plane_w, cost, S, K, P);
    return PIVP_LAUNCH_STATUS();
}

// ---- CEM refit + resample --------------------------------------------------------------------------------------------------------------------------
constexpr int CEM_MAXK = 1024;

// Philox4x32-10 and the Box-Muller transform: csrc/cem_noise.h, shared with cem_update_ex_kernel (csrc/mpc.hip)

__global__ __launch_bounds__(CEM_MAXK) void cem_update_kernel(const float* __restrict__ cost, float* __restrict__ actions, float* mean,
                                                              float* stdv, float* __restrict__ best_actions, float* __restrict__ best_cost,
                                                              const float* __restrict__ low, const float* __restrict__ high, int* __restrict__ elite_idx,
                                                              int K, int t0, int Hh, int M, float alpha, float min_std, unsigned seed_lo,
                                                              unsigned seed_hi, unsigned iteration) {
    __shared__ float cs[CEM_MAXK];
    __shared__ int el[CEM_MAXK];
    const int tid = threadIdx.x, nt = blockDim.x;
    float* __restrict__ cand = actions + (size_t)t0 * K * 5;      // rows t0 .. T-2: [Hh][K][5]
    // rank, refit and record: csrc/cem_refit.h, shared with cem_update_ex_kernel
    if (cost) cem_rank_refit_record(cost, cand, mean, stdv, best_actions, best_cost, elite_idx, K, Hh, M, alpha, min_std, cs, el);
    // resample rows t0 .. T-2 (mean / std as this block just wrote them: the phase's last barrier orders the block's own global writes)
    // One thread per (row, candidate): two Philox blocks, three Box-Muller pairs -- d = 4 takes the first normal of the third pair, as the header
    // defines it, and the pair's second normal (z[5]) is dropped.  The row's ten mean / std floats are re-read per candidate: L1 hits in a
    // kernel that the launch, not its loads, bounds.
    for (int i = tid; i < Hh * K; i += nt) {
        const int t = i / K, k = i - t * K;
        const Philox4 a = philox4x32_10((unsigned)k, (unsigned)(t0 + t), iteration, 0u, seed_lo, seed_hi);
        const Philox4 b = philox4x32_10((unsigned)k, (unsigned)(t0 + t), iteration, 1u, seed_lo, seed_hi);
        float z[6];
        box_muller(a.x[0], a.x[1], z[0], z[1]);
        box_muller(a.x[2], a.x[3], z[2], z[3]);
        box_muller(b.x[0], b.x[1], z[4], z[5]);
        float* o = cand + ((size_t)t * K + k) * 5;
#pragma unroll
        for (int d = 0; d < 5; ++d) o[d] = fminf(fmaxf(mean[t * 5 + d] + stdv[t * 5 + d] * z[d], low[d]), high[d]);
    }
}

int cem_update(const float* cost, float* actions, float* mean, float* stdv, float* best_actions, float* best_cost, const float* low,
               const float* high, int* elite_idx, int K, int steps, int t0, int elites, float alpha, float min_std, unsigned long long seed,
               int iteration, hipStream_t s) {
    PIVP_CHECK_ARG(actions && mean && stdv && best_actions && best_cost && low && high);
    PIVP_CHECK_ARG(K >= 1 && K <= CEM_MAXK && steps >= 1 && steps <= 65536 && t0 >= 0 && t0 < steps && iteration >= 0);
    PIVP_CHECK_ARG(elites >= 1 && elites <= K && alpha >= 0.f && alpha <= 1.f && min_std >= 0.f && min_std <= 3.4028234e38f);
    const int nt = K <= 256 ? 256 : CEM_MAXK;
    hipLaunchKernelGGL(cem_update_kernel, dim3(1), dim3(nt), 0, s, cost, actions, mean, stdv, best_actions, best_cost, low, high, elite_idx, K, t0,
                       steps - t0, elites, alpha, min_std, (unsigned)(seed & 0xffffffffull), (unsigned)(seed >> 32), (unsigned)iteration);
    return PIVP_LAUNCH_STATUS();
}

}  // namespace pivp
