// Gradients through the recurrent state (include/pivp_state_grad.h): moving between the fourteen-segment state layout (include/pivp_state.h: for cell
// i = 0..6, c_i then h_i, each [B][H_i][W_i][C_i] fp32) and the tensors the backward sweep keeps.  state_rows_copy_kernel moves a set of up to
// fourteen ROW segments in ONE launch -- a segment is `rows` rows of C floats with a row stride on either side -- and serves both users:
//   the gather behind the sweep's t = 0 (d loss / d state_in): the seven d c_{-1} are contiguous sources (row stride C), the seven d h_{-1} are the h
//     columns of the cells' input gradients: rows of C floats at row stride cx + C, starting cx floats into the first row;
//   the scatter in front of the sweep (the seed d / d final state): the seven c segments -> the plan's d c buffers, contiguous on both sides; the h
//     segments are read in place by the gate backward and take no part.
// Written as state.hip's copy kernel is: a plain bandwidth kernel.
//   Work is cut into RUNS of SG_RUN = 4,096 consecutive floats of a segment's [rows][C] index space: a block takes a run at a time, its 256 threads
//   issue four 16-B loads each at a 4-KB stride (a wave instruction covers 1 KiB of that index space: whole rows of 128 .. 512 B, each one contiguous),
//   all four in flight before the first store, then the four 16-B stores.  C is a multiple of 4, so a 16-B piece never straddles a row; its row and
//   column come from one division by C / 4 (uniform divisor).  Strided sources cost nothing extra in DRAM traffic that matters: a row of h columns is
//   128 .. 512 contiguous bytes, whole 128-B lines when cx * 4 and (cx + C) * 4 are multiples of 128 (every cell: cx, C in {32, 64, 96, 128}).
//   16-B accesses need the segment's two bases on 16 bytes and its row strides a multiple of 4 floats -- checked on the host per segment, not
//   assumed; a segment that fails takes the element-wise form of the same runs (4-B accesses, same bits), the others keep theirs.
//   Grid: min(runs, 2,048) blocks that stride over the runs (the gather at B = 32, 64 x 64 is 2,432 runs).  The run -> (segment, piece) decode is a
//   scan of the prefix table in the kernel's arguments: uniform over the block.  No LDS, no atomics, every destination element written once by a plain
//   vector store; every offset into src / dst is 64-bit.
#include <string.h>

#include "pivp_kernels.h"

namespace pivp {

constexpr int SG_NT = 256;
constexpr int SG_U = 4;                            // 16-B pieces per thread and run
constexpr int SG_RUN = SG_NT * SG_U * 4;           // floats per run

// ALLVEC: every segment takes 16-B accesses (what the sweep's own buffers give): no per-segment choice in the kernel
template <bool ALLVEC>
__global__ __launch_bounds__(SG_NT) void state_rows_copy_kernel(const StateRowsArgs a, int runs) {
    const int tid = threadIdx.x;
    for (int r = blockIdx.x; r < runs; r += gridDim.x) {
        int g = 0;
#pragma unroll
        for (int k = 1; k < STATE_SEGMENTS; ++k) g += (k < a.nseg && r >= a.first_run[k]) ? 1 : 0;
        const StateRowSeg sg = a.seg[g];
        const long long n = sg.rows * sg.C, at = (long long)(r - a.first_run[g]) * SG_RUN;      // floats of the segment, and in front of this run
        const int len = n - at < SG_RUN ? (int)(n - at) : SG_RUN;                               // floats of this run
        if (ALLVEC || a.vec[g]) {      // (uniform over the block: the segment's choice, made on the host)
            const int nq = len / 4, c4 = sg.C / 4;
            f32x4 v[SG_U];
            long long drow[SG_U];
            int dcol[SG_U];
#pragma unroll
            for (int u = 0; u < SG_U; ++u) {
                const int q = tid + u * SG_NT;
                if (q < nq) {
                    const long long piece = at / 4 + q;
                    drow[u] = piece / c4; dcol[u] = (int)(piece - drow[u] * c4) * 4;
                    v[u] = *reinterpret_cast<const f32x4*>(sg.src + drow[u] * sg.lds + dcol[u]);
                }
            }
#pragma unroll
            for (int u = 0; u < SG_U; ++u)
                if (tid + u * SG_NT < nq) *reinterpret_cast<f32x4*>(sg.dst + drow[u] * sg.ldd + dcol[u]) = v[u];
        } else {
            for (int i = tid; i < len; i += SG_NT) {
                const long long e = at + i, row = e / sg.C;
                const int col = (int)(e - row * sg.C);
                sg.dst[row * sg.ldd + col] = sg.src[row * sg.lds + col];
            }
        }
    }
}

int state_rows_copy(const StateRowSeg* seg, int nseg, hipStream_t s) {
    PIVP_CHECK_ARG(seg && nseg >= 1 && nseg <= STATE_SEGMENTS);
    StateRowsArgs a;
    memset(&a, 0, sizeof(a));
    long long runs = 0;
    bool allvec = true;
    for (int g = 0; g < nseg; ++g) {
        const StateRowSeg& q = seg[g];
        PIVP_CHECK_ARG(q.src && q.dst && q.rows >= 1 && q.C >= 1 && q.lds >= q.C && q.ldd >= q.C);
        PIVP_CHECK_ARG(((reinterpret_cast<uintptr_t>(q.src) | reinterpret_cast<uintptr_t>(q.dst)) & 3) == 0);
        const long long n = q.rows * q.C, pieces = (n + SG_RUN - 1) / SG_RUN;
        PIVP_CHECK_ARG(runs + pieces < (1ll << 31));
        a.seg[g] = q;
        a.first_run[g] = (int)runs;
        runs += pieces;
        // 16-B accesses, segment by segment: every row of the segment starts on 16 bytes on both sides, and is whole 16-B pieces
        a.vec[g] = q.C % 4 == 0 && q.lds % 4 == 0 && q.ldd % 4 == 0 &&
                   ((reinterpret_cast<uintptr_t>(q.src) | reinterpret_cast<uintptr_t>(q.dst)) & 15) == 0;
        allvec = allvec && a.vec[g];
    }
    a.nseg = nseg;
    const dim3 grid((unsigned)(runs < 2048 ? runs : 2048)), block(SG_NT);
    if (allvec) hipLaunchKernelGGL((state_rows_copy_kernel<true>), grid, block, 0, s, a, (int)runs);
    else hipLaunchKernelGGL((state_rows_copy_kernel<false>), grid, block, 0, s, a, (int)runs);
    return PIVP_LAUNCH_STATUS();
}

}  // namespace pivp
