// The rank / refit / record phase of the cross-entropy method, shared by cem_update_kernel (csrc/cem.hip) and cem_update_ex_kernel (csrc/mpc.hip).
// One definition, so that with the options off the two ops give the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace pivp {

// One workgroup, every thread of it; cs / el: LDS arrays of at least K floats / ints.  The K costs go into cs (NaN -> +inf), el[r] takes the
// candidate of rank r < M (ascending cost, the lower index first among equals), elite_idx (when given) a copy; mean / std are refitted to the
// elites of cand = [Hh][K][5]; the cheapest candidate becomes best_actions / best_cost[0] if it beats the record.  On return el[0 .. M-1] is
// readable by every thread, and every read of best_cost[0] and of the candidates lies in front of the phase's last barrier.
// No pointer here is __restrict__ -- `cand` least of all: cem_update_ex_kernel reads its own writes through it.  What a kernel promises about its
// own arguments still holds inside the inlined body.
__device__ __forceinline__ void cem_rank_refit_record(const float* cost, const float* cand, float* mean, float* stdv, float* best_actions,
                                                      float* best_cost, int* elite_idx, int K, int Hh, int M, float alpha, float min_std,
                                                      float* cs, int* el) {
    const int tid = threadIdx.x, nt = blockDim.x;
    const float inf = __builtin_huge_valf();
    for (int k = tid; k < K; k += nt) { const float c = cost[k]; cs[k] = c == c ? c : inf; }
    __syncthreads();
    for (int k = tid; k < K; k += nt) {
        const float c = cs[k];
        int rank = 0;
        for (int j = 0; j < K; ++j) { const float cj = cs[j]; rank += (cj < c || (cj == c && j < k)) ? 1 : 0; }
        if (rank < M) el[rank] = k;
    }
    __syncthreads();
    if (elite_idx) for (int m = tid; m < M; m += nt) elite_idx[m] = el[m];
    // the best candidate ever evaluated (read before any resampling overwrites it)
    const float c0 = cs[el[0]];
    const bool better = c0 < best_cost[0];
    // refit: per (t, d), elites in rank order; the sums and the blend in fp64, rounded to fp32 once
    for (int i = tid; i < Hh * 5; i += nt) {
        const int t = i / 5, d = i - t * 5;
        const float* col = cand + (size_t)t * K * 5 + d;
        double sum = 0.0;
        for (int m = 0; m < M; ++m) sum += (double)col[el[m] * 5];
        const double em = sum / (double)M;
        double var = 0.0;
        for (int m = 0; m < M; ++m) { const double dv = (double)col[el[m] * 5] - em; var += dv * dv; }
        const double es = sqrt(var / (double)M);
        const double al = (double)alpha;
        mean[i] = (float)(al * (double)mean[i] + (1.0 - al) * em);
        stdv[i] = fmaxf((float)(al * (double)stdv[i] + (1.0 - al) * es), min_std);
        if (better) best_actions[i] = col[el[0] * 5];
    }
    __syncthreads();                                              // every read of best_cost[0] and of the candidates lies in front of this barrier
    if (better && tid == 0) best_cost[0] = c0;
}

}  // namespace pivp
