// The step's compositing arithmetic (TM:718-728), one definition each: the flat-(num_masks + 1) mask softmax over a band of rows, the STP
// sampling coordinates and bilinear gather, the CDNA blended kernel and its 25-tap apply, the DNA taps with the reference's slice quirk, and
// the band tile staging of composite_kernel / pixel_track_kernel.  Used by composite_kernel (heads.hip), frame_head_kernel (frame_head.hip),
// pixel_track_kernel (pixel_track.hip) and the composite_bwd_* kernels (backward_heads.hip); every reference quirk below lives here only.
// All functions are forceinline and take NP, W, HW, ... by value: the constant-folded kernel instances still see constants.  The sources are
// built with -ffp-contract=off: an a * b + c below is two roundings, an fmaf one, and the order of every chain is part of the contract
// (frame_head == the separate kernels and pixel_track == composite(layer0 = 0), bit for bit).
#pragma once
#include "pivp_kernels.h"

namespace pivp {

// image rows per block of composite_kernel and pixel_track_kernel.  Measured at B = 32, 64x64 (scripts/bench_tail_ops.py): 8 rows 14.3 us,
// 4 rows 12.2, 2 rows 14.2
#ifndef PIVP_CP_TR
#define PIVP_CP_TR 4
#endif
constexpr int BAND_TR = PIVP_CP_TR;
constexpr int CDNA_KL = 11 * 28;   // LDS floats of the CDNA kernel table [11][28]: 25 taps per kernel + 3 pad, 16-B aligned rows

// ---- flat mask softmax (TM:720-722) ------------------------------------------------------------------------------------------------------
// The reference reshapes the NCHW mask tensor to (-1, NP) and softmaxes axis 1: over NP CONSECUTIVE elements of the per-sample planar buffer
// (NP = num_masks + 1), so groups cut across pixels, rows and planes; the group of flat index f is f / NP.  A band of `count` pixels that starts
// at pixel `first_flat` of every plane keeps its logits as lg[NP][win], win = count + 2 (NP - 1) (the band +- NP - 1 flat elements per plane),
// and the groups' max and 1 / sum as gmx / ginv [NP][G], G = count / NP + 2.
struct ExpFast { static __device__ __forceinline__ float of(float x) { return __expf(x); } };
struct ExpLibm { static __device__ __forceinline__ float of(float x) { return expf(x); } };   // composite_bwd_stp_kernel

struct FlatSoftmax {
    int NP;
    unsigned magic;   // exact x / NP for x * NP < 2^32 (flat plane offsets are < 12 * H * W): one v_mul_hi instead of a ~35-instruction division
    __device__ __forceinline__ explicit FlatSoftmax(int NP_) : NP(NP_), magic(0xFFFFFFFFu / (unsigned)NP_ + 1u) {}
    __device__ __forceinline__ int div(int x) const { return (int)__umulhi((unsigned)x, magic); }

    // per-group max and 1 / sum.  CLAMPED: the 12 LDS reads from clamped addresses instead of under a predicate (frame_head_kernel's measured form)
    template <class Exp, bool CLAMPED = false>
    __device__ __forceinline__ void groups(const float* lg, int win, int G, int HW, int first_flat, int count, float* gmx, float* ginv,
                                           int tid, int nthreads) const {
        for (int i = tid; i < NP * G; i += nthreads) {
            const int m = i / G, gi = i - m * G;
            const int gfirst = div(m * HW + first_flat), glast = div(m * HW + first_flat + count - 1);
            if (gfirst + gi <= glast) {
                const float* e = lg + m * win + (gfirst + gi) * NP - (m * HW + first_flat - (NP - 1));
                float ev[12];
#pragma unroll
                for (int u = 0; u < 12; ++u) {               // all reads in flight together
                    const float t = CLAMPED ? e[min(u, NP - 1)] : u < NP ? e[u] : 0.f;
                    ev[u] = u < NP ? t : -3.0e38f;
                }
                float mx = ev[0];
#pragma unroll
                for (int u = 1; u < 12; ++u) mx = fmaxf(mx, ev[u]);
                float sum = 0.f;
#pragma unroll
                for (int u = 0; u < 12; ++u) sum += u < NP ? Exp::of(ev[u] - mx) : 0.f;
                gmx[i] = mx;
                ginv[i] = 1.0f / sum;
            }
        }
    }
    // the softmaxed mask of plane m at pixel pp of the band.  The caller passes the plane's rows (lg + m * win, gmx + m * G, ginv + m * G): with the
    // row offsets formed in here hipcc gave composite_kernel<0 / 1 / 2> 89 / 73 / 130 registers for 79 / 61 / 120 (profiles/r24/NOTES.md)
    template <class Exp>
    __device__ __forceinline__ float at(const float* lgm, const float* gmxm, const float* ginvm, int HW, int first_flat, int m, int pp) const {
        const int gi = div(m * HW + first_flat + pp) - div(m * HW + first_flat);
        return Exp::of(lgm[pp + (NP - 1)] - gmxm[gi]) * ginvm[gi];
    }
};

// ---- STP (TM:465-471): one affine warp per sample, sampled bilinearly ---------------------------------------------------------------------
// Coordinates in fp64 (two dozen flops per pixel): a 1e-5 pixel error is visible at 1e-4 parity.  The two border rules: clamp the sampling
// coordinate and the corner into the frame, or (stp_zero) leave both and let taps outside the frame read 0.
struct StpSample {
    int iu, iv;            // upper-left tap
    float wu1, wv1;        // weights of the right / lower taps
    double xs, ys;         // the pixel's normalised coordinates    } the backward's; dead code in the forward kernels
    bool live_u, live_v;   // the coordinate was not clamped        }
};
__device__ __forceinline__ StpSample stp_sample(const float* th, int x, int y, int H, int W, int stp_zero) {
    StpSample s;
    s.xs = -1.0 + 2.0 * (double)x / (double)(W - 1);
    s.ys = -1.0 + 2.0 * (double)y / (double)(H - 1);
    double gu = (double)th[0] * s.xs + (double)th[1] * s.ys + (double)th[2];
    double gv = (double)th[3] * s.xs + (double)th[4] * s.ys + (double)th[5];
    s.live_u = true; s.live_v = true;
    if (!stp_zero) {
        s.live_u = gu > -1.0 && gu < 1.0; s.live_v = gv > -1.0 && gv < 1.0;
        gu = fmin(fmax(gu, -1.0), 1.0); gv = fmin(fmax(gv, -1.0), 1.0);
    }
    const double u = (gu + 1.0) * (double)(W - 1) * 0.5;
    const double v = (gv + 1.0) * (double)(H - 1) * 0.5;
    double u0 = floor(u), v0 = floor(v);
    if (!stp_zero) { u0 = fmin(fmax(u0, 0.0), (double)(W - 2)); v0 = fmin(fmax(v0, 0.0), (double)(H - 2)); }
    s.wu1 = (float)(u - u0); s.wv1 = (float)(v - v0);
    s.iu = (int)u0; s.iv = (int)v0;
    return s;
}
// the four-tap gather of the plane at base + off: an fmaf chain, lower taps last, taps outside the frame skipped
__device__ __forceinline__ float stp_gather(const float* base, size_t off, const StpSample& s, int H, int W) {
    float t = 0.f;
#pragma unroll
    for (int dv = 0; dv < 2; ++dv)
#pragma unroll
        for (int du = 0; du < 2; ++du) {
            const int uu = s.iu + du, vv = s.iv + dv;
            const float wgt = (dv ? s.wv1 : 1.f - s.wv1) * (du ? s.wu1 : 1.f - s.wu1);
            if ((unsigned)uu < (unsigned)W && (unsigned)vv < (unsigned)H) t = fmaf(wgt, base[off + vv * W + uu], t);
        }
    return t;
}
// all NM - 1 warps are the same warp: sum_{q >= 2} mk[q] weighs it (mk[q >= NP] is 0)
__device__ __forceinline__ float stp_mask_sum(const float (&mk)[12]) {
    float msum = 0.f;
#pragma unroll
    for (int q = 2; q < 12; ++q) msum += mk[q];
    return msum;
}

// ---- CDNA (TM:341-349, TM:725-727): one 5x5 correlation with the per-pixel blended kernel keff = sum_k mk[k + 2] kern_k, an fmaf chain over k
// ascending from keff = 0 -----------------------------------------------------------------------------------------------------------------
// zip truncation: generated kernel k pairs with mask k + 2, and the last of the NM kernels with none
__device__ __forceinline__ bool cdna_kernel_paired(int k, int NM) { return k < NM - 1; }
// keff += mq * kernel, the kernel's taps through seven wave-uniform ds_read_b128 of its row of the [11][28] LDS table.  The caller loops
//   for (k = 0; k < 10; ++k) if (cdna_kernel_paired(k, NM)) cdna_blend_add(mk[k + 2], kl + k * 28, keff);     (static indices keep mk[] in registers)
// itself: with the loop in here hipcc took 82 registers in composite_kernel<0> (occupancy 5 for 6), or, with keff returned by value, 160 more
// v_mov per pixel and 0.5 us of pixel_track_kernel<0>'s 5.3 (profiles/r24/NOTES.md).  (frame_head_kernel forms the same chain on the matrix cores.)
__device__ __forceinline__ void cdna_blend_add(float mq, const float* krow, float (&keff)[25]) {
    float kv[28];
#pragma unroll
    for (int q = 0; q < 7; ++q) {
        const f32x4 t4 = *reinterpret_cast<const f32x4*>(krow + q * 4);
        kv[q * 4] = t4[0]; kv[q * 4 + 1] = t4[1]; kv[q * 4 + 2] = t4[2]; kv[q * 4 + 3] = t4[3];
    }
#pragma unroll
    for (int i = 0; i < 25; ++i) keff[i] = fmaf(mq, kv[i], keff[i]);
}
// 25 taps on a haloed tile: tile[at] = the pixel's upper-left tap, PW floats per tile row.  (Tile and offset, here and in dna_apply and stp_gather:
// composite_kernel and frame_head_kernel compile shorter with the tile's base than with a pointer to the tap, pixel_track_kernel the other way
// round and passes (tap, 0); profiles/r24/NOTES.md.)
__device__ __forceinline__ float taps5x5(const float (&keff)[25], const float* tile, int at, int PW) {
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < 5; ++i)
#pragma unroll
        for (int j = 0; j < 5; ++j) t = fmaf(keff[i * 5 + j], tile[at + i * PW + j], t);
    return t;
}

// ---- DNA (TM:392-415): a per-pixel 25-tap kernel from enc7 ---------------------------------------------------------------------------------
// w[i] = kn[i] * (1 / sum kn), kn[i] = relu(raw(i) - 1e-12) + 1e-12, summed in tap order
template <class Load>
__device__ __forceinline__ void dna_weights(Load raw, float (&w)[25]) {
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < 25; ++i) {
        w[i] = fmaxf(raw(i) - 1e-12f, 0.f) + 1e-12f;
        sum += w[i];
    }
    const float inv = 1.0f / sum;
#pragma unroll
    for (int i = 0; i < 25; ++i) w[i] = w[i] * inv;
}
// the reference's slice quirk (TM:400): the shifted copies are cut at H - xk / W - yk, so tap (xk, yk) of pixel (y, x) reads 0 there
__device__ __forceinline__ float dna_apply(const float (&w)[25], const float* tile, int at, int PW, int y, int x, int H, int W) {
    float t = 0.f;
#pragma unroll
    for (int xk = 0; xk < 5; ++xk)
#pragma unroll
        for (int yk = 0; yk < 5; ++yk) {
            const bool ok = (y + xk < H) && (x + yk < W);
            t = fmaf(w[xk * 5 + yk], ok ? tile[at + xk * PW + yk] : 0.f, t);
        }
    return t;
}

// ---- band tile staging (composite_kernel, pixel_track_kernel; 256 threads) -----------------------------------------------------------------
// tile[P][BAND_TR + 4][W + 4]: P planes of the band with a 2-pixel halo, zero outside the frame.  Two phases, so that the caller can issue EVERY
// global load of the block before its first LDS store (one L2 / MALL round trip per block instead of one per element): request loads BAND_PR
// rows per thread into registers (thread = a column of the padded row; all rows when 256 / (W + 4) >= 3, W <= 81), file stores them and loops
// over the remaining rows of wide frames.  CAP: the plane capacity of the register array (P <= CAP); W + 4 <= 256 (checked by the launchers).
constexpr int BAND_PR = (BAND_TR + 4 + 2) / 3;
template <int CAP>
__device__ __forceinline__ void band_tile_request(float (&tp)[CAP][BAND_PR], const float* pb, int P, bool on, int tid, int y0, int H, int W) {
    const int PW = W + 4, HW = H * W, x = tid % PW, r0 = tid / PW, rstep = 256 / PW;
    const bool prow = on && tid < rstep * PW;
#pragma unroll
    for (int c = 0; c < CAP; ++c)
#pragma unroll
        for (int u = 0; u < BAND_PR; ++u) {
            const int r = r0 + u * rstep, iy = y0 + r - 2, ix = x - 2;
            tp[c][u] = (c < P && prow && r < BAND_TR + 4 && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W)
                           ? pb[(size_t)c * HW + iy * W + ix] : 0.f;
        }
}
template <int CAP>
__device__ __forceinline__ void band_tile_file(const float (&tp)[CAP][BAND_PR], float* tile, const float* pb, int P, bool on, int tid, int y0,
                                               int H, int W) {
    const int PW = W + 4, HW = H * W, x = tid % PW, r0 = tid / PW, rstep = 256 / PW;
    if (!(on && tid < rstep * PW)) return;
    float* col = tile + x;   // the thread's column (through the pointer: 48 address instructions fewer than tile[.. + x] in pixel_track_kernel<0>)
#pragma unroll
    for (int c = 0; c < CAP; ++c)
#pragma unroll
        for (int u = 0; u < BAND_PR; ++u) {
            const int r = r0 + u * rstep;
            if (c < P && r < BAND_TR + 4) col[(c * (BAND_TR + 4) + r) * PW] = tp[c][u];
        }
    for (int r = r0 + BAND_PR * rstep; r < BAND_TR + 4; r += rstep) {   // wide frames: remaining rows
        const int iy = y0 + r - 2, ix = x - 2;
        const bool in = (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
        for (int c = 0; c < P; ++c) col[(c * (BAND_TR + 4) + r) * PW] = in ? pb[(size_t)c * HW + iy * W + ix] : 0.f;
    }
}
// the sample's NM generated kernels [NM][25] into the [11][28] table, pads and rows >= NM zero: two entries per thread, staged the same way
__device__ __forceinline__ void cdna_table_request(float (&tk)[2], const float* aux, int b, int NM, int tid) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int i2 = tid + 256 * u, k = i2 / 28, e = i2 - k * 28;
        tk[u] = (i2 < CDNA_KL && k < NM && e < 25) ? aux[((size_t)b * NM + k) * 25 + e] : 0.f;
    }
}
__device__ __forceinline__ void cdna_table_file(const float (&tk)[2], float* kl, int tid) {
#pragma unroll
    for (int u = 0; u < 2; ++u)
        if (tid + 256 * u < CDNA_KL) kl[tid + 256 * u] = tk[u];
}

// ---- host: bytes of LDS a composite block stages for a W-wide frame with num_masks masks (composite_serves: heads.hip) ----------------------
inline size_t composite_lds_bytes(int W, int num_masks) {
    const int NP = num_masks + 1;
    const int np = BAND_TR * W;
    const int win = np + 2 * (NP - 1);
    const int G = np / NP + 2;
    return sizeof(float) * ((size_t)NP * win + 2 * NP * G + 3 * (BAND_TR + 4) * (W + 4) + CDNA_KL);
}

}  // namespace pivp
