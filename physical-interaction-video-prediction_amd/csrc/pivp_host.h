// Host-side launch helpers shared by the per-op C ABI (pivp_c_api.hip) and the plan (plan.h, plan_setup.hip, plan_forward.hip, plan_backward.hip).
// A helper takes its required core positionally (tensors, channel counts, strides, B, H, W, stream) and everything optional as named fields of ONE
// options struct behind it: callers value-initialise the struct (`T o{};`), assign what they use by name and pass it by reference.
// Value-initialised means every field zero / null; an operand form (Operand, pivp_kernels.h) then is F32.
#pragma once
#include "pivp_kernels.h"
#include "side_lane.h"
#include "sweep_schedule.h"

namespace pivp {

long long view_bytes(int B, int H, int W, int ld);
bool fits31(long long v);

// ---- option groups that recur ----
// an input given as a RAW tensor whose LayerNorm is applied while it is staged: per-element gamma / beta, statistics from the producer's `np` (count, mean, M2)
// partials per sample in `part`
struct LnIn { const float* gamma; const float* beta; const float* part; int np; float eps; };
// the LayerNorm partials of a launch's OUTPUT, written by its epilogue: `cap` slots per sample in `part`; *nparts receives how many were written (0: none)
struct LnPartOut { float* part; int cap; int* nparts; };
// training plans: the launch that applies an input norm also WRITES the normalised tensor (pixel stride ld) and the samples' (mean, rstd)
struct NormKeep { float* out; int ld; float* stat; };
// group 3 (1x1 conv with the smeared action / state) + the state predictor in the epilogue of the conv that feeds them (IgemmDesc::f3_*)
struct Enc3Fuse { const float* w3; const float* b3; const float* action; const float* state; const float* wcs; const float* bcs; float* e3; float* state_out; int use_state; };
// the motion head's finisher carried by a transposed-conv launch as B blocks behind its tiles (IgemmDesc::rd_*): mode 1 CDNA (out = kerns [B][nout],
// vpre [B][256] or null), 2 STP (out = theta [B][6], vpre = relu(Linear(100)) [B][256] or null)
struct MotionRider { int mode, KS, nout; const float* partials; const float* bias; const float* w2; const float* b2; float* out; float* vpre; };
// IgemmDesc::ep_*: a second tensor met in the plain 5x5 bf16 convolution's epilogue (mode 1 ReLU mask, 2 add) on its first `cols` output columns.
// *applied (host) tells the caller whether the launch took it (unsplit grid) or the separate pass is still the caller's to run.
struct EpSpec { const float* src; int ld, cols, mode; int* applied; };

// ---- forward ----
struct ConvLstmOpts {
    int variant;                     // fp32 kernel: 0 auto, 1..4 wave layouts; with w_bf16: channels per block (0 auto, 16, 32)
    float* gates_out;                // training: the gate activations [M][4C]
    LnPartOut ln_out;                // the LayerNorm behind the cell gets its statistics from the cell's epilogue
    Operand operand;                 // F32: the fp32 kernel on w.  Any other form runs on ...
    const unsigned short* w_bf16;    // ... the pack of w in that form (pack_lstm_bf16): one is given exactly when the other is
    const LnIn* ln_in;               // x is raw, normalised while staged (the L2-direct forms' eight-wave kernels: convlstm_ln_in_ok)
};
bool convlstm_ln_in_ok(Operand form, int cx, int ldx, int C, int B, int H, int W);
int run_convlstm(const float* x, int cx, int ldx, const float* h_prev, int C, const float* w, const float* bias,
                 const float* c_in, float* c_out, float* h_out, int B, int H, int W, hipStream_t s, const ConvLstmOpts& o = ConvLstmOpts{});
int run_conv3x3s2(const float* x, int cin, int ldx, const float* w, const float* bias, float* out, int cout,
                  int ldo, int relu, int B, int Hin, int Win, hipStream_t s, int accum);
// conv3x3s2 of LayerNorm(x_raw) with the norm applied while the input is staged (IgemmDesc::in_g); conv3x3s2_ln_ok tells whether the
// geometry qualifies (output tiles of 32 anchors inside one sample)
bool conv3x3s2_ln_ok(int cin, int cout, int B, int Hin, int Win);
struct Conv3x3LnOpts { const Enc3Fuse* fuse3; NormKeep keep; };
int run_conv3x3s2_ln(const float* x_raw, int cin, const float* w, const float* bias, float* out, int cout, int ldo, int relu,
                     int B, int Hin, int Win, hipStream_t s, const LnIn& ln, const Conv3x3LnOpts& o = Conv3x3LnOpts{});
struct DeconvOpts {
    int accum;
    LnPartOut ln_out;
    Operand operand;                 // form of the all-parities tile kernel (deconv_tile.hip), fp32 elsewhere; BF16X6 has none and is refused
    const float* wscale_part;        // FP16X3: absmax_partials(w)
};
int run_deconv3x3s2(const float* x, int cin, int ldx, const float* w, const float* bias, float* out, int cout,
                    int ldo, int relu, int B, int Hin, int Win, hipStream_t s, const DeconvOpts& o = DeconvOpts{});
int run_deconv3x3s2_and_partials(const float* x, int cin, const float* w, const float* bias, float* out, int cout, int ldo, int relu,
                                 int B, int Hin, int Win, hipStream_t s, const float* wt, float* partials, int dbl);   // + motion_partials(x, wt, ...) in the same grid
// deconv3x3s2 of concat(LayerNorm(h_raw) [c_ln channels], x1 [c1 channels, stride ld1]) with the norm applied while the tile kernel stages its
// patch (IgemmDesc::in_g); ln.part = the producer's partials of h_raw, never the same buffer as ln_out.part (the output's)
bool deconv3x3s2_ln_ok(int c_ln, int c1, int cout, int B, int Hin, int Win);
struct DeconvLnOpts {
    const float* x1; int c1, ld1;    // the second source of the concat (null: h_raw alone)
    LnPartOut ln_out;
    Operand operand;                 // as DeconvOpts::operand
    const float* wscale_part;        // as DeconvOpts::wscale_part
    NormKeep keep;
    const MotionRider* rider;
};
int run_deconv3x3s2_ln(const float* h_raw, int c_ln, const float* w, const float* bias, float* out, int cout, int ldo, int relu,
                       int B, int Hin, int Win, hipStream_t s, const LnIn& ln, const DeconvLnOpts& o = DeconvLnOpts{});
struct ConvS1Opts {
    int accum;
    int wN;             // columns of the weight pack when only its first `cout` are wanted
    int dest_zeroed;    // 1: the caller has cleared `out` (see conv_s1_splits_k)
    int no_split;       // 1: never split K (deterministic sweeps: no atomics into `out`)
};
int run_conv_s1(const float* x, int cin, int ldx, const float* w, float* out, int cout, int ldo, int ksize, int B, int H, int W,
                hipStream_t s, const ConvS1Opts& o = ConvS1Opts{});
bool conv_s1_splits_k(int cin, int cout, int ldo, int ksize, int B, int H, int W, int wN, int no_split);
bool conv5x5_bf16_splits_k(int cin, int cout, int ldo, int B, int H, int W, Operand form, int no_split);
struct Conv5x5Bf16Opts {
    Operand operand;             // the pack's form (never F32)
    int dest_zeroed;             // 1: the caller has cleared `out` (see conv5x5_bf16_splits_k)
    const float* ascale_part;    // FP16X3: absmax_partials(x) (the activations' power-of-two scale)
    const EpSpec* ep;
    int no_split;                // 1: never split K (deterministic sweeps)
};
int run_conv5x5_bf16(const float* x, int cin, int ldx, const unsigned short* wb, float* out, int cout, int ldo, int accum,
                     int B, int H, int W, hipStream_t s, const Conv5x5Bf16Opts& o);
struct LayerNormOpts {
    float* stat_out;       // receives the samples' (mean, rstd)
    int fused_nparts;      // > 0: the kernel that produced x already wrote that many (count, mean, M2) partials per sample
};
int run_layernorm(const float* x, const float* g, const float* b, float* out, float* partials, int B, int n, int C,
                  int ldo, float eps, int relu, hipStream_t s, const LayerNormOpts& o = LayerNormOpts{});

// ---- weight gradients: the caller owns the WgradDesc (pivp_kernels.h documents every field) ----
// One geometry filler per case clears the descriptor and sets ONE timestep's sizes for contiguous operands; the caller then assigns the operands (x0, ld0, x1, dy,
// ldy, dw, db) and the options it wants (tcount / ts_*, part / part_overwrite, dy_absmax, form, slot_*) by name; WgradDesc::operand is run_wgrad's to fill.
void lstm_wgrad_geom(WgradDesc& d, int cx, int C, int B, int H, int W);                                 // 5x5 ConvLSTM: x0 = x [cx], x1 = h_prev [C], dy = dG [4C]
void conv3x3s2_wgrad_geom(WgradDesc& d, int mode, int cin, int cout, int B, int Hin, int Win);      // conv3x3s2 (mode 0) / deconv3x3s2 (mode 1)
// The single host entry of every weight gradient.  Completes d (x1 == null: no h operand; a single timestep; the byte extents), asks wgrad_launch (wgrad_form.h)
// for the form and the grid, launches, and where the kernel that ran does not sum dy's columns into d.db itself runs one bias_grad per timestep (dy + j * ts_dy).
// Other than F32, 5x5 ConvLSTM case only: BF16, BF16X6, FP16X3 (needs d.dy_absmax); BF16X3 has no weight-gradient form and is refused.  fixed_order (deterministic
// sweeps): PIVP_ERR_STATE in front of the launch unless the form sums in an order fixed by the shape (wgrad_fixed_order).
int run_wgrad(WgradDesc& d, hipStream_t s, Operand form, bool fixed_order = false);
// floats of WgradDesc::part a conv3x3s2 / deconv3x3s2 weight gradient of these sizes needs
long long conv_backward_part_floats(int mode, int cin, int cout, int B, int Hin, int Win);
bool conv_backward_fixed_order(int mode, int cin, int cout, int B, int Hin, int Win);      // the partial-plane form with its column sums (wgrad3x3s2) serves it
// the fp32 ConvLSTM weight gradient's partial slots (csrc/wgrad5x5p.hip): floats of WgradDesc::part (0: the shape is not served), and the reduction
// (has_h = 0: of launches without an h operand -- the sweep's t = 0 --, which cut the x rows' tiles their own way: reduce before switching)
// slot_ntw / slot_j: WgradDesc::slot_ntw (0 by shape, 1 / 2 = 32 / 64 columns per wave) and WgradDesc::slot_j (0 = by the CU count, > 0 fixed)
long long lstm_wgrad_part_floats(int cx, int C, int B, int H, int W, int slot_ntw, int slot_j);
int lstm_wgrad_reduce(int cx, int C, int has_h, float* part, float* dW, float* db, int B, int H, int W, hipStream_t s, int slot_ntw, int slot_j);

// ---- backward ----
// ConvLSTM cell backward (TM:262-272): gate math, data gradient d[x,h_prev], weight and bias gradients
struct ConvLstmBwdArgs {
    // required
    const float* x; int cx, ldx; const float* h_prev; int C; const float* w; const float* gates;
    const float* c_old; const float* c_new; const float* dh_a; int lda; const float* dh_b; int ldb;      // d h_t = dh_a + dh_b (either may be null)
    float* dc; int dc_valid;      // updated in place to d c_{t-1}
    float* dG; float* wt;
    float* d_in;                  // [M][cx+C]: d x (first cx channels) and d h_{t-1} (last C)
    float* dW; float* db;         // dW == null: the caller batches this layer's weight gradient over several timesteps itself (plan_backward.hip)
    int B, H, W;
    // optional
    int wt_ready;                 // 1: wt (and wt_bf16) already hold the transposed pack
    Operand operand;              // the data gradient's form: F32 = the fp32 kernels on wt; any other runs on ...
    unsigned short* wt_bf16;      // ... the pack of wt in that form: one is given exactly when the other is
    const SideFork* fork;         // the weight gradient on a second stream
    const LnFuse* ln;             // dh_a is formed from the LayerNorm behind the cell
    int dx_only;                  // 1: d h_{t-1} is not needed (the sweep's last timestep): only the cx columns of d_in are computed
    float* dg_absmax;             // 66 floats: receives dG's partial maxima (absmax_partials), the scale of the fp16-piece data gradient (operand FP16X3 needs
                                  // it) and of the fp16-piece weight gradient (WgradDesc::dy_absmax)
    const EpSpec* ep;             // the data gradient's epilogue hook (bf16 / split-precision data gradients on unsplit grids)
    int det;                      // deterministic sweeps: unsplit data gradients (the caller passes dW = null)
};
int run_convlstm_backward(const ConvLstmBwdArgs& a, hipStream_t s);
// conv3x3s2 (mode 0) / deconv3x3s2 (mode 1) backward: dx (optionally accumulated), dW, db
struct ConvBwdArgs {
    // required
    int mode; const float* x; int cin, ldx; const float* w; float* dy; int cout, ldy;
    const float* y; int ldyy;     // y != null: dy is masked in place by (y > 0) (fused ReLU)
    float* wt; float* dx; int lddx, accum_dx;      // dx == null: no data gradient
    float* dW; float* db;         // dW == null: as ConvLstmBwdArgs::dW; the fork's `ready` is recorded
    int B, Hin, Win;
    // optional
    int wt_ready;
    const SideFork* fork;
    float* part;                  // WgradDesc::part
    const float* dy_add; int ld_add;    // a second gradient into the same output, added in the ReLU-mask pass
    Operand operand;              // BF16 (the bf16 precision mode): the data gradient's operands rounded to bf16 where the transposed conv's tile kernel takes it
                                  // (enc1's); the weight gradient stays fp32 (its bf16 form -- transposing LDS reads, 2 MFMAs per 32-pixel chunk -- was built and is
                                  // slower: profiles/r05/NOTES.md)
};
int run_conv_backward(const ConvBwdArgs& a, hipStream_t s);

// run-time wave priority of the main stream's kernels (pivp_common.h): every translation unit with such kernels, on stream s
int main_prio_set_backward(int on, hipStream_t s);
int main_prio_set_backward_heads(int on, hipStream_t s);
int main_prio_set_convlstm_bf16(int on, hipStream_t s);
int main_prio_set_conv5x5_bf16(int on, hipStream_t s);
int main_prio_set_deconv_tile(int on, hipStream_t s);
int main_prio_set_igemm_f32(int on, hipStream_t s);
int main_prio_set_igemm_small(int on, hipStream_t s);
int run_select_frames(const float* gt, const float* gen, const unsigned char* take, float* out, int B, int frame_numel, hipStream_t s);

}  // namespace pivp
