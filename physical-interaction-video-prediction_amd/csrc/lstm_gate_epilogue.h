// The ConvLSTM gate epilogue: how an MFMA accumulator becomes (c, h, gates, LayerNorm partial).  One definition each of the gate
// gather, the cell update with its two activation policies, and the packed-operand kernels' plain-convolution tail and tile partial;
// called by igemm_f32_kernel (igemm_f32.hip: gather and cell only -- its descriptor stores and tile_stats handle rows past M),
// convlstm_bf16_kernel (convlstm_ring.h) and convlstm_x6g_kernel (convlstm_l2direct.h).  Reference op: BasicConvLSTMCell.__call__, TM:262-272.
#pragma once
#include "pivp_kernels.h"

namespace pivp {

// ---- activation policies ---------------------------------------------------------------------------------------------------------
// sigmoid / tanh of the gate epilogue through v_exp_f32 / v_rcp_f32: |error| <= ~2e-7 absolute, an order
// below the fp32 accumulation noise of the K = 1600..4800 dot products in front of them.
// 1 / d as v_rcp_f32 plus one Newton step (3 instructions, error well under 1 ulp) instead of an IEEE division: __frcp_rn expands to
// ~10 instructions (div_scale x2, rcp, 4 fma, div_fmas, div_fixup), 5 times per cell.  The bare 1-ulp v_rcp_f32 is not enough for the
// parity path: through 9 recurrent steps and the STP warp of white-noise frames it moved tests/test_gpu_model.py's STP case past its gate.
__device__ __forceinline__ float fast_rcp(float d) {
    const float r = __builtin_amdgcn_rcpf(d);
    return fmaf(fmaf(-d, r, 1.0f), r, r);
}
// (x is clamped at -87: below that exp(-x) is +inf, v_rcp_f32 returns 0 and the Newton step's inf * 0 is a NaN -- found in round 4 by a range test
// of the split-precision kernels with pre-activations of -150, where this kernel wrote NaN cells; sigmoid(-87) = 1.6e-38)
__device__ __forceinline__ float fast_sigmoid(float x) { return fast_rcp(1.0f + __expf(-fmaxf(x, -87.0f))); }
// tanh: 2 / (1 + exp(-2x)) - 1 carries ~1.2e-7 of ABSOLUTE error at every x (the rounding of a value near 1), i.e. many ulps of a small
// tanh; behind a LayerNorm that divides by the ~0.2 spread of h this was a third of the whole path's error against the float64 oracle
// (scripts/gate_math_study.py: hidden1 3.7e-7 rms with libm's tanh, 4.7e-7 with that formula) and what put the STP fixture over 1e-4.
// Here: |x| < 0.55: x + x^3 P(x^2), a degree-4 least-squares fit (3.3e-8 absolute, < 1 ulp relative); beyond: 1 - 2 / (1 + exp(2|x|)).
__device__ __forceinline__ float fast_tanh(float x) {
    const float a = fminf(fabsf(x), 15.0f);   // tanh(15) rounds to 1; keeps exp finite for the Newton step of fast_rcp
    const float p = a * a;
    float q = fmaf(p, -0.006149096414446831f, 0.02097311243414879f);
    q = fmaf(p, q, -0.053824927657842636f);
    q = fmaf(p, q, 0.13332274556159973f);
    q = fmaf(p, q, -0.3333330452442169f);
    const float small = fmaf(a * p, q, a);
    const float big = fmaf(-2.0f, fast_rcp(1.0f + __expf(2.0f * a)), 1.0f);
    return copysignf(a < 0.55f ? small : big, x);
}
// the packed-operand kernels' forms (bare v_rcp_f32: their operands carry 8-24 bits); b_tanh is also what the gate backward applies to c_t
__device__ __forceinline__ float b_sigmoid(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }
__device__ __forceinline__ float b_tanh(float x) { return 2.0f * __builtin_amdgcn_rcpf(1.0f + __expf(-2.0f * x)) - 1.0f; }
// The two policies are numerically distinct on purpose: the fp32 kernel is held to the float64 oracle, the packed ones to their operands' precision.
struct GateActF32 {
    static __device__ __forceinline__ float sigmoid(float x) { return fast_sigmoid(x); }
    static __device__ __forceinline__ float tanh(float x) { return fast_tanh(x); }
};
struct GateActPacked {
    static __device__ __forceinline__ float sigmoid(float x) { return b_sigmoid(x); }
    static __device__ __forceinline__ float tanh(float x) { return b_tanh(x); }
};

// ---- gate gather -----------------------------------------------------------------------------------------------------------------
// Accumulator row r of a lane is one anchor, its column (gate t * GPT + grp, channel): the 4 gates of a cell sit in the GPT
// lanes lane ^ (x * CPW) and the 4 / GPT tiles (GPT = gates inside one 32-column MFMA tile, CPW = channels per wave: GPT * CPW = 32).
// Lane grp takes rows r = k * GPT + grp: it keeps its own gate of that row and receives the others from its partners in GPT - 1
// xor-shuffles per tile, each partner sending the row its receiver owns.  Every lane then updates one (anchor, channel) per k: no idle
// lanes, 1 (GPT 2) or 3 (GPT 4) shuffles per tile instead of 8 or 16 per cell; GPT = 1 needs no exchange.  Register arrays are only
// indexed statically; per-lane choices are select chains.
template <int GPT>
__device__ __forceinline__ float gate_pick(const float (&v)[GPT], int idx) {
    static_assert(GPT == 1 || GPT == 2 || GPT == 4, "gates per MFMA tile");
    if constexpr (GPT == 1) {
        return v[0];
    } else if constexpr (GPT == 2) {
        return idx ? v[1] : v[0];
    } else {
        const float lo = (idx & 1) ? v[1] : v[0], hi = (idx & 1) ? v[3] : v[2];
        return (idx & 2) ? hi : lo;
    }
}
// rows[g] = accumulator row k * GPT + g of one tile; out[g] = gate (tile * GPT + g) of the cell (row k * GPT + grp, this lane's channel)
template <int GPT, int CPW>
__device__ __forceinline__ void gate_exchange(const float (&rows)[GPT], int grp, float (&out)[GPT]) {
    float val[GPT];
    val[0] = gate_pick<GPT>(rows, grp);
#pragma unroll
    for (int x = 1; x < GPT; ++x) val[x] = __shfl_xor(gate_pick<GPT>(rows, grp ^ x), x * CPW, 64);
#pragma unroll
    for (int g = 0; g < GPT; ++g) out[g] = gate_pick<GPT>(val, g ^ grp);
}

// ---- cell update (TM:269-272) ----------------------------------------------------------------------------------------------------
struct LstmCell { float aj, ai, af, ao, c, h; };
// g4 = the pre-activations in the weights' gate order j, i, f, o; bf carries the forget bias (+ 1) already
template <class Act>
__device__ __forceinline__ LstmCell lstm_cell(const float (&g4)[4], float bj, float bi, float bf, float bo, float c_prev) {
    LstmCell r;
    r.aj = Act::tanh(g4[0] + bj); r.ai = Act::sigmoid(g4[1] + bi);
    r.af = Act::sigmoid(g4[2] + bf); r.ao = Act::sigmoid(g4[3] + bo);
    r.c = c_prev * r.af + r.ai * r.aj;
    r.h = Act::tanh(r.c) * r.ao;
    return r;
}
// the packed kernels' cell stores (the fp32 kernel stores through buffer descriptors that drop rows past M): pixel m, channel ch of C
__device__ __forceinline__ void lstm_cell_store(const IgemmDesc& d, const LstmCell& v, int m, int ch) {
    const int C = d.C;
    const size_t o = (size_t)m * C + ch;
    d.cstate_out[o] = v.c;
    d.hout[o] = v.h;
    if (d.gates_out) {
        float* gp = d.gates_out + (size_t)m * 4 * C + ch;
        gp[0] = v.aj; gp[C] = v.ai; gp[2 * C] = v.af; gp[3 * C] = v.ao;
    }
}

// ---- packed kernels: plain-convolution tail --------------------------------------------------------------------------------------
// Accumulator row = anchor m, column = output channel col; 32 lanes write 128 contiguous bytes.  The epilogue hook's second tensor
// (d.ep_src) is requested for ALL of the lane's outputs first (plain_hook_load) and met at the store (plain_store): read next to each
// store it cost one exposed round trip per accumulator row (the data gradients ran 9-11 us longer per launch with it, more than the pass
// it replaces).  Neutral elements where the hook does not apply: 1 for the mask, 0 for the sum.
__device__ __forceinline__ float plain_hook_load(const IgemmDesc& d, size_t m, int col, int ncols) {
    return (col < ncols && col < d.ep_cols) ? d.ep_src[m * d.ep_ld + col] : (d.ep_mode == 1 ? 1.f : 0.f);
}
__device__ __forceinline__ void plain_store(const IgemmDesc& d, float v, float ev, size_t m, int col, int ncols) {
    if (col < ncols) {                  // the pack's rows past the real column count are zero padding
        float* o = d.out + m * d.ldo + col;
        if (d.ep_mode == 1) v = ev > 0.f ? v : 0.f;      // (unsplit grids only: the launcher clears ep_mode otherwise)
        else if (d.ep_mode == 2) v += ev;
        if (gridDim.y > 1) atomicAdd(o, v);             // the channel groups are split over gridDim.y: partial sums meet in `out`
        else if (d.accum) *o += v;
        else *o = v;
    }
}

// ---- packed kernels: LayerNorm partial of the block's h tile ----------------------------------------------------------------------
// (count, mean, M2) of the h values of each image of the tile, two passes over the NV values a lane holds, fixed summation order
// (bitwise reproducible); one writer per image.  The block's multiplying waves are NWM x NWN (wave = wm + NWM * wn) over anchors x
// channels; with two images per tile the waves wm < NWM / 2 (of every wave column) own image 0, the others image 1 -- a wave's anchors
// lie inside one image.  `red`: 16 floats of LDS that every wave is done with after the first barrier here.  slot: the tile's partial
// within its image's d.ln_nparts.
template <int NWM, int NWN, int NV>
__device__ __forceinline__ void ln_tile_partial(const IgemmDesc& d, const float (&sv)[NV], float* red, bool two_img, int wm, int wn, int lane, int b0, size_t slot) {
    constexpr int NW = NWM * NWN;
    static_assert((NW == 4 || NW == 8) && NWM % 2 == 0, "the fixed orders below");
    const int wave = wm + NWM * wn;
    // per-wave values [at, at + NW) in the kernel's fixed order: one image: the pairwise tree; two: the image's waves in ascending order
    auto combine = [&](int at, int img) -> float {
        if (!two_img) {
            const float lo = (red[at] + red[at + 1]) + (red[at + 2] + red[at + 3]);
            if constexpr (NW == 4) return lo;
            else return lo + ((red[at + 4] + red[at + 5]) + (red[at + 6] + red[at + 7]));
        }
        float s = 0.f;
#pragma unroll
        for (int w = 0; w < NW; ++w) s += ((w % NWM) * 2 / NWM == img) ? red[at + w] : 0.f;
        return s;
    };
    float s1 = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) s1 += sv[i];
    s1 = wave_sum(s1);
    __syncthreads();
    if (lane == 0) red[wave] = s1;
    __syncthreads();
    const int img = two_img ? wm * 2 / NWM : 0;
    const float cnt = 64.f * NV * (two_img ? NW / 2 : NW);
    const float mean = combine(0, img) / cnt;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) { const float dd = sv[i] - mean; q = fmaf(dd, dd, q); }
    q = wave_sum(q);
    if (lane == 0) red[8 + wave] = q;
    __syncthreads();
    if (lane == 0 && wn == 0 && wm == img * (NWM / 2)) {      // one writer per image: its first wave
        float* p = d.ln_part + ((size_t)(b0 + img) * d.ln_nparts + slot) * 4;
        p[0] = cnt; p[1] = mean; p[2] = combine(8, img); p[3] = 0.f;
    }
}

}  // namespace pivp
