// Closed-loop planning (include/pivp_mpc.h): what one CEM planning call hands to the next.
//   cem_update_ex   pivp_cem_update with kept elites, the mean as a candidate and temporally correlated noise.  ONE workgroup like cem_update_kernel
//                (csrc/cem.hip): the rank by counting needs all K costs in LDS, and K <= 1024.  The rank / refit / record phase is ONE function that both
//                kernels call (csrc/cem_refit.h), and so are the random numbers (csrc/cem_noise.h): with the options off the two ops give the same
//                bits.  Behind the phase:
//                  keep     thread (row, j) reads the rank-j elite's five floats of its row into registers, a barrier, then writes slot j -- a block
//                           of nt / keep rows per barrier; rows are independent, so nothing else orders the copies.
//                  beta > 0 Q (n x n, fp64) is built once per launch in LDS: s_j = j^(-beta/2) by the first n/2 + 1 threads, sigma summed by every
//                           thread in the same order, the angle reduced exactly ((j i) mod n) before sincospi.  The white normals go into rows
//                           t0 .. of `actions` (about to be overwritten anyway), a barrier, then each thread owns (k, d) columns: its n normals
//                           into registers, the n sums in ascending order in fp64, mean / std / clamp, store.  No workspace.  The kernel is
//                           instantiated for n <= 16 and n <= 64 so that the short horizons planning uses hold 16 registers, not 64.
//                Launch-latency bound at planning sizes (K = 32, n <= 16); at K = 1024, n = 64 the 5120 columns cost 4096 fp64 multiply-adds each.
//   cem_shift    the receding-horizon shift of mean / std / kept slots / best_actions, in place: ONE 256-thread workgroup walks the elements in
//                ascending (row, column) order, 256 at a time: read (from `shift` rows further on, or the tail value), barrier, write.  A later
//                block only reads rows beyond everything written so far, so the copies are exact whatever `shift`.
// Both: fp32 in and out, stream-ordered, no host synchronisation, no atomics, a fixed order: the same bits on every launch.
#include <math.h>

#include "../../include/pivp_mpc.h"
#include "cem_noise.h"
#include "cem_refit.h"
#include "pivp_kernels.h"

namespace pivp {

constexpr int MPC_MAXK = 1024;
constexpr int MPC_MAXN = PIVP_CEM_MAX_COLORED_STEPS;

struct CemExArgs {
    const float* cost; float* actions; float* mean; float* stdv; float* best_actions; float* best_cost;
    const float* low; const float* high; int* elite_idx;
    int K, t0, Hh, M;
    float alpha, min_std;
    unsigned seed_lo, seed_hi, iteration;
    int keep, kept_in, add_mean;
    float beta;
};

__device__ __forceinline__ void cem_row_normals(int k, int t, const CemExArgs& a, float z[6]) {      // the normals cem_update_kernel draws for (k, t)
    const Philox4 x = philox4x32_10((unsigned)k, (unsigned)t, a.iteration, 0u, a.seed_lo, a.seed_hi);
    const Philox4 y = philox4x32_10((unsigned)k, (unsigned)t, a.iteration, 1u, a.seed_lo, a.seed_hi);
    box_muller(x.x[0], x.x[1], z[0], z[1]);
    box_muller(x.x[2], x.x[3], z[2], z[3]);
    box_muller(y.x[0], y.x[1], z[4], z[5]);
}

// NMAX: 0 = white noise (beta == 0), else the largest n = Hh the instance serves with beta > 0
template <int NMAX>
__global__ __launch_bounds__(MPC_MAXK) void cem_update_ex_kernel(CemExArgs a) {
    __shared__ float cs[MPC_MAXK];
    __shared__ int el[MPC_MAXK];
    __shared__ double Q[NMAX > 0 ? NMAX * NMAX : 1];
    __shared__ double sj[NMAX / 2 + 1];
    const int tid = threadIdx.x, nt = blockDim.x;
    const int K = a.K, Hh = a.Hh, M = a.M, keep = a.keep;
    const float* __restrict__ cost = a.cost;
    const float* __restrict__ low = a.low;
    const float* __restrict__ high = a.high;
    float* mean = a.mean;
    float* stdv = a.stdv;
    float* cand = a.actions + (size_t)a.t0 * K * 5;      // rows t0 .. T-2: [Hh][K][5]; read back after the block's own writes, hence not __restrict__
    if (cost) {
        cem_rank_refit_record(cost, cand, mean, stdv, a.best_actions, a.best_cost, a.elite_idx, K, Hh, M, a.alpha, a.min_std, cs, el);
        if (keep > 0) {
            // slot j <- elite el[j], row by row.  keep <= K <= nt: a pass takes nt / keep whole rows, every thread at most one (row, slot).  All of a
            // pass's reads, the barrier, then its writes; another pass touches other rows.  The last barrier also holds back the sampling below
            // until the last elite has been read.
            const int rows = nt / keep;
            const int r = tid / keep, j = tid - r * keep;
            for (int r0 = 0; r0 < Hh; r0 += rows) {
                const bool on = r < rows && r0 + r < Hh;
                float v[5];
                if (on) {
                    const float* src = cand + ((size_t)(r0 + r) * K + el[j]) * 5;
#pragma unroll
                    for (int d = 0; d < 5; ++d) v[d] = src[d];
                }
                __syncthreads();
                if (on) {
                    float* dst = cand + ((size_t)(r0 + r) * K + j) * 5;
#pragma unroll
                    for (int d = 0; d < 5; ++d) dst[d] = v[d];
                }
            }
        }
    }
    // slots below `fixed` keep what they hold; slot `mean_slot` takes the clamped mean; every other slot is sampled
    const int fixed = (cost || a.kept_in) ? keep : 0;
    const int mean_slot = a.add_mean ? keep : -1;
    for (int i = tid; i < Hh * K; i += nt) {
        const int t = i / K, k = i - t * K;
        if (k < fixed) continue;
        float* o = cand + ((size_t)t * K + k) * 5;
        if (k == mean_slot) {
#pragma unroll
            for (int d = 0; d < 5; ++d) o[d] = fminf(fmaxf(mean[t * 5 + d], low[d]), high[d]);
            continue;
        }
        float z[6], mu[5], sd[5];
#pragma unroll
        for (int d = 0; d < 5; ++d) { mu[d] = mean[t * 5 + d]; sd[d] = stdv[t * 5 + d]; }      // (all ten loads in front of the first store)
        cem_row_normals(k, a.t0 + t, a, z);
#pragma unroll
        for (int d = 0; d < 5; ++d) {
            if (NMAX == 0) o[d] = fminf(fmaxf(mu[d] + sd[d] * z[d], low[d]), high[d]);
            else o[d] = z[d];                                     // the white normal, parked where the sample will go
        }
    }
    if constexpr (NMAX > 0) {
        const int n = Hh;                                         // <= NMAX (the host checks)
        for (int j = tid; j <= n / 2; j += nt) sj[j] = pow((double)(j > 1 ? j : 1), -0.5 * (double)a.beta);
        __syncthreads();
        double s2 = sj[0] * sj[0];
        for (int j = 1; 2 * j < n; ++j) s2 += 2.0 * (sj[j] * sj[j]);
        if (n > 1 && (n & 1) == 0) s2 += sj[n / 2] * sj[n / 2];
        const double sigma = sqrt(s2);
        for (int e = tid; e < n * n; e += nt) {
            const int i = e / n, c = e - i * n;
            double v = sj[0];
            if (c > 0) {
                const int j = (c + 1) / 2;
                const int m = (j * i) % n;                        // the angle 2 pi j i / n, reduced exactly
                double sn, cn;
                sincospi(2.0 * (double)m / (double)n, &sn, &cn);
                if (2 * j == n) v = sj[j] * cn;                   // cos(pi i): +-1
                else v = 1.4142135623730951 * sj[j] * ((c & 1) ? cn : -sn);
            }
            Q[e] = v / sigma;
        }
        __syncthreads();                                          // Q, and the white normals in global memory
        for (int col = tid; col < K * 5; col += nt) {
            const int k = col / 5, d = col - k * 5;
            if (k < fixed || k == mean_slot) continue;
            float z[NMAX > 0 ? NMAX : 1];
#pragma unroll
            for (int c = 0; c < NMAX; ++c) if (c < n) z[c] = cand[(size_t)c * K * 5 + col];
            for (int i = 0; i < n; ++i) {
                const double* q = Q + i * n;
                double s = 0.0;
#pragma unroll
                for (int c = 0; c < NMAX; ++c) if (c < n) s += q[c] * (double)z[c];
                cand[(size_t)i * K * 5 + col] = fminf(fmaxf(mean[i * 5 + d] + stdv[i * 5 + d] * (float)s, low[d]), high[d]);
            }
        }
    }
}

// ---- the receding-horizon shift --------------------------------------------------------------------------------------------------------------------
constexpr int SH_NT = 256;

struct CemShiftArgs {
    float* mean; float* stdv; float* actions; float* best_actions; float* best_cost;
    const float* low; const float* high; const float* tail_mean; const float* tail_std; const float* std_floor;
    int K, t0, n, keep, shift;
};

__global__ __launch_bounds__(SH_NT) void cem_shift_kernel(CemShiftArgs a) {
    const int tid = threadIdx.x;
    const int first_slot = a.best_actions ? 3 : 2;               // column groups of five: mean, std, [best_actions], kept slot 0, 1, ...
    const int cols = (first_slot + a.keep) * 5;
    const long long total = (long long)a.n * cols;
    float* cand = a.actions ? a.actions + (size_t)a.t0 * a.K * 5 : nullptr;
    for (long long base = 0; base < total; base += SH_NT) {
        const long long e = base + tid;
        const bool on = e < total;
        float v = 0.f;
        float* dst = nullptr;
        if (on) {
            const int i = (int)(e / cols), c = (int)(e - (long long)i * cols);
            const int g = c / 5, d = c - g * 5;
            const bool tail = i >= a.n - a.shift;
            float* p;                                             // the group's [rows][stride] array at column d
            size_t stride = 5;
            if (g == 0) p = a.mean + d;
            else if (g == 1) p = a.stdv + d;
            else if (g < first_slot) p = a.best_actions + d;
            else { p = cand + (size_t)(g - first_slot) * 5 + d; stride = (size_t)a.K * 5; }
            dst = p + (size_t)i * stride;
            if (!tail) v = p[(size_t)(i + a.shift) * stride];
            else if (g == 0) v = a.tail_mean[d];
            else if (g == 1) v = a.tail_std[d];
            else v = fminf(fmaxf(a.tail_mean[d], a.low[d]), a.high[d]);
            if (g == 1) v = fmaxf(v, a.std_floor[d]);
        }
        __syncthreads();
        if (on) *dst = v;
    }
    if (tid == 0 && a.best_cost) a.best_cost[0] = __builtin_huge_valf();
}

}  // namespace pivp

using namespace pivp;

extern "C" int pivp_cem_update_ex(const float* cost, float* actions, float* mean, float* std, float* best_actions, float* best_cost,
                                  const float* low, const float* high, int* elite_idx, int K, int steps, int t0, int elites, float alpha,
                                  float min_std, unsigned long long seed, int iteration, int keep, int kept_in, int add_mean, float beta,
                                  void* stream) {
    PIVP_CHECK_ARG(actions && mean && std && best_actions && best_cost && low && high);
    PIVP_CHECK_ARG(K >= 1 && K <= MPC_MAXK && steps >= 1 && steps <= 65536 && t0 >= 0 && t0 < steps && iteration >= 0);
    PIVP_CHECK_ARG(elites >= 1 && elites <= K && alpha >= 0.f && alpha <= 1.f && min_std >= 0.f && min_std <= 3.4028234e38f);
    PIVP_CHECK_ARG(keep >= 0 && keep <= elites && (kept_in == 0 || kept_in == 1) && (add_mean == 0 || add_mean == 1) && keep + add_mean <= K);
    PIVP_CHECK_ARG(beta >= 0.f && beta <= 3.4028234e38f && (beta == 0.f || steps - t0 <= MPC_MAXN));
    CemExArgs a;
    a.cost = cost; a.actions = actions; a.mean = mean; a.stdv = std; a.best_actions = best_actions; a.best_cost = best_cost;
    a.low = low; a.high = high; a.elite_idx = elite_idx;
    a.K = K; a.t0 = t0; a.Hh = steps - t0; a.M = elites; a.alpha = alpha; a.min_std = min_std;
    a.seed_lo = (unsigned)(seed & 0xffffffffull); a.seed_hi = (unsigned)(seed >> 32); a.iteration = (unsigned)iteration;
    a.keep = keep; a.kept_in = kept_in; a.add_mean = add_mean; a.beta = beta;
    const dim3 grid(1), block(K <= 256 ? 256 : MPC_MAXK);
    hipStream_t s = (hipStream_t)stream;
    if (beta == 0.f) hipLaunchKernelGGL((cem_update_ex_kernel<0>), grid, block, 0, s, a);
    else if (a.Hh <= 16) hipLaunchKernelGGL((cem_update_ex_kernel<16>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((cem_update_ex_kernel<MPC_MAXN>), grid, block, 0, s, a);
    return PIVP_LAUNCH_STATUS();
}

extern "C" int pivp_cem_shift(float* mean, float* std, float* actions, float* best_actions, float* best_cost, const float* low,
                              const float* high, const float* tail_mean, const float* tail_std, const float* std_floor, int K, int steps, int t0,
                              int keep, int shift, void* stream) {
    PIVP_CHECK_ARG(mean && std && tail_mean && tail_std && std_floor);
    PIVP_CHECK_ARG(K >= 1 && K <= MPC_MAXK && keep >= 0 && keep <= K && t0 >= 0 && steps > t0 && steps - t0 <= 65536);
    PIVP_CHECK_ARG(shift >= 1 && shift < steps - t0);
    PIVP_CHECK_ARG((actions || keep == 0) && ((!actions && !best_actions) || (low && high)));
    CemShiftArgs a;
    a.mean = mean; a.stdv = std; a.actions = actions; a.best_actions = best_actions; a.best_cost = best_cost;
    a.low = low; a.high = high; a.tail_mean = tail_mean; a.tail_std = tail_std; a.std_floor = std_floor;
    a.K = K; a.t0 = t0; a.n = steps - t0; a.keep = keep; a.shift = shift;
    hipLaunchKernelGGL(cem_shift_kernel, dim3(1), dim3(SH_NT), 0, (hipStream_t)stream, a);
    return PIVP_LAUNCH_STATUS();
}
