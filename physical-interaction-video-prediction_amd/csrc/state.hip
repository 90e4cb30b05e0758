// The recurrent state of a batch as ONE buffer (include/pivp_state.h): for cell i = 0..6, c_i then h_i, each [B][H_i][W_i][C_i] fp32 -- fourteen
// segments.  state_copy_kernel moves such a set of segments in ONE launch, and serves both users:
//   the pack behind a rollout's last step (pivp_plan_set_rollout_state): the last slab's fourteen tensors -> the caller's buffer, identity over samples;
//   pivp_state_copy: sample b of dst = sample index[b] of src, segment by segment (broadcast 1 -> K, selection, permutation).
// Its argument is a table of the fourteen (src base, dst base, floats per sample) and an optional int32 index on the device.
//   Work is cut into RUNS: SC_RUN = 4,096 consecutive floats (16 KB) of one (segment, sample) -- a sample of a segment is contiguous on both sides, so a
//   run is one contiguous read and one contiguous write whatever the index says.  A block takes a run at a time: its 256 threads issue four 16-B loads
//   each at a 4-KB stride (every wave instruction covers 1 KiB, lane after lane: fully coalesced), all four in flight before the first store, then the
//   four 16-B stores.  Per-sample segment sizes are multiples of 4 floats (H, W % 8 == 0, C in {32, 64, 128}), so a run is whole 16-B pieces and only
//   the last run of a small segment (16 x 16 frames: 512 .. 2,048 floats per sample) is short.
//   Grid: the op is bandwidth-bound, so min(runs, 2,048) blocks (8 per CU on 256 CUs) that stride over the runs -- a K = 1,024 state at 64 x 64 is
//   77,824 runs, 38 per block; the pack at B = 32 is 2,432.  The run -> (segment, sample, piece) decode is a scan of the 15-entry prefix table in
//   the kernel's arguments: uniform over the block, scalar registers.  No LDS (nothing is re-ordered), no atomics, every output element written once
//   by a plain store: a packed state stays in the XCD's L2 for the next rollout's first gate convs.
//   Bases that are not 16-byte aligned (a caller's view at an odd float) take the element-wise form of the same run: 4-B accesses, same bits.
//   Every offset into src / dst is 64-bit (K = 1,024 at 64 x 64 is 1.27 GB); index[] is trusted (the host layer validates it).  src and dst may be the
//   same buffer only where no sample moves (the identity).
#include "pivp_kernels.h"

namespace pivp {

constexpr int SC_NT = 256;
constexpr int SC_U = 4;                            // 16-B pieces per thread and run
constexpr int SC_RUN = SC_NT * SC_U * 4;           // floats per run

template <bool VEC>
__global__ __launch_bounds__(SC_NT) void state_copy_kernel(const StateCopyArgs a, const int* __restrict__ index, int runs) {
    const int tid = threadIdx.x;
    for (int r = blockIdx.x; r < runs; r += gridDim.x) {
        int g = 0;
#pragma unroll
        for (int k = 1; k < STATE_SEGMENTS; ++k) g += r >= a.first_run[k] ? 1 : 0;
        const int q = r - a.first_run[g], b = q / a.pieces[g], piece = q - b * a.pieces[g];
        const long long n = a.seg[g].n, at = (long long)piece * SC_RUN;
        const int len = n - at < SC_RUN ? (int)(n - at) : SC_RUN;       // floats of this run
        const long long sb = index ? index[b] : b;
        const float* __restrict__ src = a.seg[g].src + sb * n + at;
        float* __restrict__ dst = a.seg[g].dst + (long long)b * n + at;
        if constexpr (VEC) {
            const int nq = len / 4;
            f32x4 v[SC_U];
#pragma unroll
            for (int u = 0; u < SC_U; ++u)
                if (tid + u * SC_NT < nq) v[u] = reinterpret_cast<const f32x4*>(src)[tid + u * SC_NT];
#pragma unroll
            for (int u = 0; u < SC_U; ++u)
                if (tid + u * SC_NT < nq) reinterpret_cast<f32x4*>(dst)[tid + u * SC_NT] = v[u];
        } else {
            for (int i = tid; i < len; i += SC_NT) dst[i] = src[i];
        }
    }
}

int state_copy(const StateSeg seg[STATE_SEGMENTS], const int* index, int B_dst, hipStream_t s) {
    PIVP_CHECK_ARG(seg && B_dst >= 1);
    StateCopyArgs a;
    long long runs = 0;
    bool vec = true;
    for (int g = 0; g < STATE_SEGMENTS; ++g) {
        PIVP_CHECK_ARG(seg[g].src && seg[g].dst && seg[g].n >= 1);
        const long long pieces = (seg[g].n + SC_RUN - 1) / SC_RUN;
        PIVP_CHECK_ARG(pieces < (1ll << 31) && runs + pieces * B_dst < (1ll << 31));
        a.seg[g] = seg[g];
        a.first_run[g] = (int)runs;
        a.pieces[g] = (int)pieces;
        runs += pieces * B_dst;
        // 16-B accesses need every sample of every segment to start on 16 bytes on both sides
        vec = vec && seg[g].n % 4 == 0 && ((reinterpret_cast<uintptr_t>(seg[g].src) | reinterpret_cast<uintptr_t>(seg[g].dst)) & 15) == 0;
    }
    const dim3 grid((unsigned)(runs < 2048 ? runs : 2048)), block(SC_NT);
    if (vec) hipLaunchKernelGGL((state_copy_kernel<true>), grid, block, 0, s, a, index, (int)runs);
    else hipLaunchKernelGGL((state_copy_kernel<false>), grid, block, 0, s, a, index, (int)runs);
    return PIVP_LAUNCH_STATUS();
}

}  // namespace pivp
