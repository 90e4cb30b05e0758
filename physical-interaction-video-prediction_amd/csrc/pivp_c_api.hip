// C-ABI layer: the host-side launch helpers of pivp_host.h and the per-op entry points declared in include/pivp_hip.h.
// The plan (Model.__init__ / reset_state / __call__ of the reference, TM:484-764), which sequences the whole per-timestep
// op program in native code on one HIP stream, lives in plan_setup.hip / plan_forward.hip / plan_backward.hip (plan.h).
#include <string.h>
#include <string>
#include <vector>

#include "../../include/pivp_hip.h"
#include "../../include/pivp_data.h"
#include "../../include/pivp_conv_forms.h"
#include "pivp_host.h"

using namespace pivp;

namespace pivp {

// extent in bytes of an NHWC view with pixel stride ld (for the kernels' buffer descriptors)
long long view_bytes(int B, int H, int W, int ld) { return (long long)B * H * W * ld * 4; }
bool fits31(long long v) { return v > 0 && v < (1LL << 31); }
int run_convlstm(const float* x, int cx, int ldx, const float* h_prev, int C, const float* w, const float* bias,
                 const float* c_in, float* c_out, float* h_out, int B, int H, int W, hipStream_t s, const ConvLstmOpts& o) {
    const LnIn* const ln_in = o.ln_in;
    const bool l2d = operand_l2_direct(o.operand);
    if ((o.w_bf16 != nullptr) != (o.operand != Operand::F32)) return PIVP_ERR_BADARG;
    IgemmDesc d;
    memset(&d, 0, sizeof(d));
    if (ln_in) {
        if (!convlstm_ln_in_ok(o.operand, cx, ldx, C, B, H, W) || !ln_in->gamma || !ln_in->beta || !ln_in->part || ln_in->np <= 0 || ln_in->part == o.ln_out.part)
            return PIVP_ERR_BADARG;
        d.in_g = ln_in->gamma; d.in_b = ln_in->beta; d.in_part = ln_in->part; d.in_np = ln_in->np; d.in_eps = ln_in->eps;
    }
    // h_prev == nullptr: the recurrent input is identically zero (first timestep after reset_state, TM:254-257);
    // its K range contributes exactly 0 and is skipped
    d.x0 = x; d.c0 = cx; d.ld0 = ldx; d.x1 = h_prev; d.c1 = h_prev ? C : 0; d.ld1 = C; d.wcin = cx + C;
    d.w = w; d.bias = bias;
    d.B = B; d.Hin = H; d.Win = W; d.Hg = H; d.Wg = W; d.in_step = 1;
    d.N = 4 * C; d.M = B * H * W;
    d.nphase = 1; d.deconv = 0; d.ksize = 5; d.pad = 2;
    const long long b0 = view_bytes(B, H, W, ldx), b1 = view_bytes(B, H, W, C), bw = 25LL * (cx + C) * 4 * C * 4;
    if (!fits31(b0) || !fits31(b1) || !fits31(bw) || (o.gates_out && !fits31(4 * b1))) return PIVP_ERR_BADARG;   // (epilogue: 32-bit buffer offsets)
    d.bytes0 = (int)b0; d.bytes1 = (int)b1; d.bytesw = (int)bw;
    d.out_step = 1; d.Hout = H; d.Wout = W;
    d.cstate_in = c_in; d.cstate_out = c_out; d.hout = h_out; d.C = C; d.gates_out = o.gates_out;
    d.ln_part = o.ln_out.part; d.ln_cap = o.ln_out.cap;
    // any form but F32 runs on w_bf16, the pack of w in that form (pack_lstm_bf16); variant then is the kernel's channels per block
    // (the L2-direct forms: a map their tiles do not serve -- 8 wide with an odd batch -- takes the fp32 kernel, which is what those modes stand in for)
    if (l2d && !convlstm_bf16_ok(d)) return w ? igemm_lstm(d, s, 0, o.ln_out.nparts) : PIVP_ERR_BADARG;
    if (o.w_bf16) return convlstm_bf16(d, o.w_bf16, s, o.operand, o.ln_out.nparts, (l2d && o.variant != 16 && o.variant != 32) ? 0 : o.variant);
    return igemm_lstm(d, s, o.variant, o.ln_out.nparts);
}

// the eight-wave L2-direct kernels take it: a 16-wide map, x contiguous in one 64-channel group, and a grid that picks those kernels
bool convlstm_ln_in_ok(Operand form, int cx, int ldx, int C, int B, int H, int W) {
    return operand_l2_direct(form) && cx <= 64 && ldx == cx && cx % 8 == 0 && C % 16 == 0 && H % 8 == 0 && W % 16 == 0;
}
static int conv3x3s2_desc(IgemmDesc& d, const float* x, int cin, int ldx, const float* w, const float* bias, float* out, int cout,
                          int ldo, int relu, int B, int Hin, int Win, int accum) {
    if (Hin % 2 || Win % 2) return PIVP_ERR_BADARG;
    memset(&d, 0, sizeof(d));
    d.x0 = x; d.c0 = cin; d.ld0 = ldx; d.wcin = cin; d.w = w; d.bias = bias;
    d.B = B; d.Hin = Hin; d.Win = Win; d.Hg = Hin / 2; d.Wg = Win / 2; d.in_step = 2;
    d.N = cout; d.M = B * d.Hg * d.Wg;
    d.nphase = 1; d.deconv = 0; d.ksize = 3; d.pad = 1;
    const long long b0 = view_bytes(B, Hin, Win, ldx), bw = 9LL * cin * cout * 4;
    if (!fits31(b0) || !fits31(bw)) return PIVP_ERR_BADARG;
    d.bytes0 = (int)b0; d.bytesw = (int)bw;
    d.out_step = 1; d.Hout = d.Hg; d.Wout = d.Wg; d.out = out; d.ldo = ldo; d.relu = relu; d.accum = accum;
    return PIVP_OK;
}
int run_conv3x3s2(const float* x, int cin, int ldx, const float* w, const float* bias, float* out, int cout,
                  int ldo, int relu, int B, int Hin, int Win, hipStream_t s, int accum) {
    IgemmDesc d;
    int rc = conv3x3s2_desc(d, x, cin, ldx, w, bias, out, cout, ldo, relu, B, Hin, Win, accum);
    if (rc != PIVP_OK) return rc;
    return igemm_conv(d, s);
}

// conv3x3s2 of LayerNorm(x_raw): the norm (per-element gamma / beta, statistics from the producer's partials) is applied while the
// input is staged -- no launch of its own (inference rollouts).  x_raw [B][Hin*Win][cin] contiguous.
static void conv3x3s2_ln_desc(IgemmDesc& d, const float* x_raw, int cin, const float* w, const float* bias, float* out, int cout, int ldo,
                              int relu, int B, int Hin, int Win) {
    memset(&d, 0, sizeof(d));
    d.x0 = x_raw; d.c0 = cin; d.ld0 = cin; d.wcin = cin; d.w = w; d.bias = bias;
    d.B = B; d.Hin = Hin; d.Win = Win; d.Hg = Hin / 2; d.Wg = Win / 2; d.in_step = 2;
    d.N = cout; d.M = B * d.Hg * d.Wg;
    d.nphase = 1; d.deconv = 0; d.ksize = 3; d.pad = 1;
    d.out_step = 1; d.Hout = d.Hg; d.Wout = d.Wg; d.out = out; d.ldo = ldo; d.relu = relu;
}
bool conv3x3s2_ln_ok(int cin, int cout, int B, int Hin, int Win) {
    if (Hin % 2 || Win % 2 || cin % 32 || cout % 32) return false;
    IgemmDesc d;
    conv3x3s2_ln_desc(d, nullptr, cin, nullptr, nullptr, nullptr, cout, cout, 0, B, Hin, Win);
    return igemm_in_ln_ok(d) && fits31(view_bytes(B, Hin, Win, cin)) && fits31(9LL * cin * cout * 4);
}
int run_conv3x3s2_ln(const float* x_raw, int cin, const float* w, const float* bias, float* out, int cout, int ldo, int relu,
                     int B, int Hin, int Win, hipStream_t s, const LnIn& ln, const Conv3x3LnOpts& o) {
    if (!x_raw || !w || !out || !ln.gamma || !ln.beta || !ln.part || ln.np <= 0 || !conv3x3s2_ln_ok(cin, cout, B, Hin, Win)) return PIVP_ERR_BADARG;
    IgemmDesc d;
    conv3x3s2_ln_desc(d, x_raw, cin, w, bias, out, cout, ldo, relu, B, Hin, Win);
    d.bytes0 = (int)view_bytes(B, Hin, Win, cin); d.bytesw = (int)(9LL * cin * cout * 4);
    d.in_g = ln.gamma; d.in_b = ln.beta; d.in_part = ln.part; d.in_np = ln.np; d.in_eps = ln.eps;
    d.in_out = o.keep.out; d.in_out_ld = o.keep.ld; d.in_stat_out = o.keep.stat;
    if (o.fuse3 && o.fuse3->e3) {
        if (cout != 64 || ldo != 64 || !relu || !bias) return PIVP_ERR_BADARG;
        d.f3_w = o.fuse3->w3; d.f3_b = o.fuse3->b3; d.f3_action = o.fuse3->action; d.f3_state = o.fuse3->state; d.f3_wcs = o.fuse3->wcs; d.f3_bcs = o.fuse3->bcs;
        d.f3_out = o.fuse3->e3; d.f3_state_out = o.fuse3->state_out; d.f3_use_state = o.fuse3->use_state;
    }
    int rc = igemm_validate(d, false);
    if (rc != PIVP_OK) return rc;
    return igemm_small(d, s);
}

// IgemmDesc of a transposed 3x3 stride-2 conv of concat(x0 [c0 channels, stride ld0], x1 [c1, ld1]; null: x0 alone): the four output parities as phases over
// the INPUT map's anchors
static int deconv3x3s2_desc(IgemmDesc& d, const float* x0, int c0, int ld0, const float* x1, int c1, int ld1, const float* w, const float* bias,
                            float* out, int cout, int ldo, int relu, int B, int Hin, int Win) {
    memset(&d, 0, sizeof(d));
    d.x0 = x0; d.c0 = c0; d.ld0 = ld0; d.x1 = x1; d.c1 = x1 ? c1 : 0; d.ld1 = ld1; d.wcin = c0 + d.c1; d.w = w; d.bias = bias;
    d.B = B; d.Hin = Hin; d.Win = Win; d.Hg = Hin; d.Wg = Win; d.in_step = 1;
    d.N = cout; d.M = B * Hin * Win;
    d.nphase = 4; d.deconv = 1; d.ksize = 3; d.pad = 1;
    const long long b0 = view_bytes(B, Hin, Win, ld0), b1 = d.c1 ? view_bytes(B, Hin, Win, ld1) : 0, bw = 9LL * d.wcin * cout * 4;
    if (!fits31(b0) || (d.c1 && !fits31(b1)) || !fits31(bw)) return PIVP_ERR_BADARG;
    d.bytes0 = (int)b0; d.bytes1 = (int)b1; d.bytesw = (int)bw;
    d.out_step = 2; d.Hout = 2 * Hin; d.Wout = 2 * Win; d.out = out; d.ldo = ldo; d.relu = relu;
    return PIVP_OK;
}
// the transposed conv's tile kernel has no three-piece form, and its fp16-piece form needs the weights' absmax partials
static bool deconv_form_ok(Operand form, const float* wscale_part) { return form != Operand::BF16X6 && (!operand_needs_scale(form) || wscale_part); }
int run_deconv3x3s2(const float* x, int cin, int ldx, const float* w, const float* bias, float* out, int cout,
                    int ldo, int relu, int B, int Hin, int Win, hipStream_t s, const DeconvOpts& o) {
    if (!deconv_form_ok(o.operand, o.wscale_part)) return PIVP_ERR_BADARG;
    IgemmDesc d;
    int rc = deconv3x3s2_desc(d, x, cin, ldx, nullptr, 0, 0, w, bias, out, cout, ldo, relu, B, Hin, Win);
    if (rc != PIVP_OK) return rc;
    d.wscale_part = o.wscale_part;
    d.operand = o.operand;          // honoured by the all-parities tile kernel (deconv_tile.hip), fp32 otherwise
    d.accum = o.accum;
    d.ln_part = o.ln_out.part; d.ln_cap = o.ln_out.cap;
    return igemm_conv(d, s, o.ln_out.nparts);
}

// run_deconv3x3s2(x, ...) AND motion_partials(x, wt, partials, ...) -- two independent launches that read the same tensor and fill a
// fraction of the chip each (enc4 and the motion head's Linear on hidden5) -- as ONE grid when the conv is igemm_small's (else the two
// launches, in that order).  x [B][Hin*Win][cin] contiguous = the Linear's [B][K] input, K = Hin * Win * cin.
int run_deconv3x3s2_and_partials(const float* x, int cin, const float* w, const float* bias, float* out, int cout, int ldo, int relu,
                                 int B, int Hin, int Win, hipStream_t s, const float* wt, float* partials, int dbl) {
    IgemmDesc d;
    int rc = deconv3x3s2_desc(d, x, cin, cin, nullptr, 0, 0, w, bias, out, cout, ldo, relu, B, Hin, Win);
    if (rc != PIVP_OK) return rc;
    const int K = Hin * Win * cin;
    // (Both in ONE grid -- round 4's igemm_small_partials_kernel -- took 21.4-22.0 us against 12.7 + 9.2 for the two launches, whichever kind of block
    // was dispatched first, and the rollout did not move: profiles/r04/NOTES.md.  Two launches; the fused grid is in the history.)
    rc = igemm_conv(d, s);
    if (rc != PIVP_OK) return rc;
    return motion_partials(x, wt, partials, B, K, dbl, s);
}

// deconv3x3s2 of concat(LayerNorm(h_raw), x1): the norm of the first c_ln channels (per-element gamma / beta, statistics from the
// producer's partials) is applied while the all-parities tile kernel stages its patch -- no launch of its own, and the normalised tensor
// is never written (inference rollouts: [hidden6 | enc1] -> enc5, [hidden7 | enc0] -> enc6).  h_raw [B][Hin*Win][c_ln] contiguous.
bool deconv3x3s2_ln_ok(int c_ln, int c1, int cout, int B, int Hin, int Win) {
    if (c_ln <= 0 || c_ln % 32 || c1 < 0 || c1 % 32 || cout % 32 || Hin % 8 || Win % 16) return false;
    return (long)B * (Hin / 8) * (Win / 16) * (cout / 32) >= 16;
}
int run_deconv3x3s2_ln(const float* h_raw, int c_ln, const float* w, const float* bias, float* out, int cout, int ldo, int relu,
                       int B, int Hin, int Win, hipStream_t s, const LnIn& ln, const DeconvLnOpts& o) {
    const NormKeep& keep = o.keep;
    if (!h_raw || !w || !out || !ln.gamma || !ln.beta || !ln.part || ln.np <= 0 || !deconv3x3s2_ln_ok(c_ln, o.x1 ? o.c1 : 0, cout, B, Hin, Win)) return PIVP_ERR_BADARG;
    if (keep.out && (keep.ld < c_ln || keep.ld % 4 || ((uintptr_t)keep.out & 15))) return PIVP_ERR_BADARG;
    if (o.ln_out.part && o.ln_out.part == ln.part) return PIVP_ERR_BADARG;      // blocks finish (and write their output partial) while others still read the input's
    IgemmDesc d;
    int rc = deconv3x3s2_desc(d, h_raw, c_ln, c_ln, o.x1, o.c1, o.ld1, w, bias, out, cout, ldo, relu, B, Hin, Win);
    if (rc != PIVP_OK) return rc;
    if (!deconv_form_ok(o.operand, o.wscale_part)) return PIVP_ERR_BADARG;
    d.operand = o.operand; d.wscale_part = o.wscale_part;
    d.in_g = ln.gamma; d.in_b = ln.beta; d.in_part = ln.part; d.in_np = ln.np; d.in_eps = ln.eps;
    d.ln_part = o.ln_out.part; d.ln_cap = o.ln_out.cap;
    d.in_out = keep.out; d.in_out_ld = keep.ld; d.in_stat_out = keep.stat;
    if (o.rider && o.rider->mode) {
        d.rd_mode = o.rider->mode; d.rd_blocks = B; d.rd_KS = o.rider->KS; d.rd_nout = o.rider->nout;
        d.rd_partials = o.rider->partials; d.rd_bias = o.rider->bias; d.rd_w2 = o.rider->w2; d.rd_b2 = o.rider->b2; d.rd_out = o.rider->out; d.rd_vpre = o.rider->vpre;
    }
    rc = igemm_validate(d, false);
    if (rc != PIVP_OK) return rc;
    if (!deconv_tile_ok(d)) return PIVP_ERR_BADARG;
    return deconv_tile(d, s, o.ln_out.nparts);
}

// stride-1 K x K "same" convolution through the generic kernel (used as the ConvLSTM data gradient)
static int conv_s1_desc(IgemmDesc& d, const float* x, int cin, int ldx, const float* w, float* out, int cout, int ldo, int ksize, int B, int H, int W,
                        int accum, int wN) {
    memset(&d, 0, sizeof(d));
    d.x0 = x; d.c0 = cin; d.ld0 = ldx; d.wcin = cin; d.w = w; d.bias = nullptr;
    d.B = B; d.Hin = H; d.Win = W; d.Hg = H; d.Wg = W; d.in_step = 1;
    d.N = cout; d.M = B * H * W; d.wN = wN > cout ? wN : 0;
    d.nphase = 1; d.deconv = 0; d.ksize = ksize; d.pad = ksize / 2;
    const long long b0 = view_bytes(B, H, W, ldx), bw = (long long)ksize * ksize * cin * (wN > cout ? wN : cout) * 4;
    if (!fits31(b0) || !fits31(bw)) return PIVP_ERR_BADARG;
    d.bytes0 = (int)b0; d.bytesw = (int)bw;
    d.out_step = 1; d.Hout = H; d.Wout = W; d.out = out; d.ldo = ldo; d.relu = 0; d.accum = accum;
    // fresh output (contiguous, or the leading columns of a buffer whose rest nobody reads): the K-split path is allowed; it needs a zeroed destination
    if (!accum && (ldo == cout || d.wN)) d.ksplit_ok = 1;
    return PIVP_OK;
}
// true when run_conv_s1 with these arguments adds K-split partial sums into `out` (B * H * W * ldo floats to be zeroed first)
bool conv_s1_splits_k(int cin, int cout, int ldo, int ksize, int B, int H, int W, int wN, int no_split) {
    if (no_split) return false;
    IgemmDesc d;
    static float dummy;
    if (conv_s1_desc(d, &dummy, cin, cin, &dummy, &dummy, cout, ldo, ksize, B, H, W, 0, wN) != PIVP_OK) return false;
    return d.ksplit_ok && igemm_conv_ksplit(d) > 1;
}
int run_conv_s1(const float* x, int cin, int ldx, const float* w, float* out, int cout, int ldo, int ksize, int B, int H, int W,
                hipStream_t s, const ConvS1Opts& o) {
    IgemmDesc d;
    int rc = conv_s1_desc(d, x, cin, ldx, w, out, cout, ldo, ksize, B, H, W, o.accum, o.wN);
    if (rc != PIVP_OK) return rc;
    if (o.no_split && d.ksplit_ok) { d.ksplit_ok = 0; d.no_ksplit = 1; }      // deterministic sweeps: an unsplit grid, plain stores
    if (d.ksplit_ok && !o.dest_zeroed && igemm_conv_ksplit(d) > 1 &&
        hipMemsetAsync(out, 0, (size_t)B * H * W * ldo * 4, s) != hipSuccess) return PIVP_ERR_LAUNCH;
    return igemm_conv(d, s);
}

// 5x5 stride-1 "same" convolution with bf16 operands (csrc/convlstm_bf16.hip); wb = pack_lstm_bf16(w, cin, cout, conv5x5_bf16_rows(cout))
static int conv5x5_bf16_desc(IgemmDesc& d, const float* x, int cin, int ldx, float* out, int cout, int ldo, int accum, int B, int H, int W) {
    memset(&d, 0, sizeof(d));
    d.x0 = x; d.c0 = cin; d.ld0 = ldx; d.wcin = cin;
    d.B = B; d.Hin = H; d.Win = W; d.Hg = H; d.Wg = W; d.in_step = 1;
    d.N = cout; d.M = B * H * W; d.nphase = 1; d.ksize = 5; d.pad = 2;
    const long long b0 = view_bytes(B, H, W, ldx);
    if (!fits31(b0)) return PIVP_ERR_BADARG;
    d.bytes0 = (int)b0;
    d.out_step = 1; d.Hout = H; d.Wout = W; d.out = out; d.ldo = ldo; d.accum = accum;
    if (!accum && ldo == cout) d.ksplit_ok = 1;     // contiguous fresh output: the K-split path may be used; it needs a zeroed destination
    return PIVP_OK;
}
bool conv5x5_bf16_splits_k(int cin, int cout, int ldo, int B, int H, int W, Operand form, int no_split) {
    if (no_split) return false;
    IgemmDesc d;
    static float dummy;
    if (conv5x5_bf16_desc(d, &dummy, cin, cin, &dummy, cout, ldo, 0, B, H, W) != PIVP_OK) return false;
    return d.ksplit_ok && conv5x5_bf16_ksplit(d, form) > 1;
}
int run_conv5x5_bf16(const float* x, int cin, int ldx, const unsigned short* wb, float* out, int cout, int ldo, int accum,
                     int B, int H, int W, hipStream_t s, const Conv5x5Bf16Opts& o) {
    const EpSpec* const ep = o.ep;
    IgemmDesc d;
    int rc = conv5x5_bf16_desc(d, x, cin, ldx, out, cout, ldo, accum, B, H, W);
    if (rc != PIVP_OK) return rc;
    if (o.no_split) d.ksplit_ok = 0;      // deterministic sweeps: one block per output tile over the whole K (no atomics)
    d.wscale_part = o.ascale_part;
    if (ep && ep->applied) *ep->applied = 0;
    if (ep && ep->src && ep->mode && !(d.ksplit_ok && conv5x5_bf16_ksplit(d, o.operand) > 1)) {
        d.ep_src = ep->src; d.ep_ld = ep->ld; d.ep_cols = ep->cols < cout ? ep->cols : cout; d.ep_mode = ep->mode;
        if (ep->applied) *ep->applied = 1;
    }
    if (d.ksplit_ok && !o.dest_zeroed && conv5x5_bf16_ksplit(d, o.operand) > 1 &&
        hipMemsetAsync(out, 0, (size_t)B * H * W * cout * 4, s) != hipSuccess) return PIVP_ERR_LAUNCH;
    return conv5x5_bf16(d, wb, s, o.operand);
}

// ---- weight gradients ----
// descriptor of a ConvLSTM weight gradient's ONE-timestep geometry (what the partial buffer's size and the reduction depend on)
void lstm_wgrad_geom(WgradDesc& d, int cx, int C, int B, int H, int W) {
    memset(&d, 0, sizeof(d));
    d.c0 = cx; d.ld0 = cx; d.c1 = C; d.ld1 = C; d.cin = cx + C; d.wcin = cx + C; d.N = 4 * C; d.ldy = 4 * C;
    d.B = B; d.Hx = H; d.Wx = W; d.Hy = H; d.Wy = W; d.Hg = H; d.Wg = W; d.M = B * H * W;
    d.ksize = 5; d.pad = 2; d.stride = 1;
}
// ... of a stride-2 3x3 conv (mode 0: anchors = output pixels) / transposed conv (mode 1: anchors = input pixels)
void conv3x3s2_wgrad_geom(WgradDesc& d, int mode, int cin, int cout, int B, int Hin, int Win) {
    const int Hout = mode ? 2 * Hin : Hin / 2, Wout = mode ? 2 * Win : Win / 2;
    memset(&d, 0, sizeof(d));
    d.c0 = cin; d.ld0 = cin; d.cin = cin; d.wcin = cin; d.N = cout; d.ldy = cout; d.B = B; d.Hx = Hin; d.Wx = Win; d.Hy = Hout; d.Wy = Wout;
    d.deconv = mode; d.ksize = 3; d.pad = 1; d.stride = 2;
    d.Hg = mode ? Hin : Hout; d.Wg = mode ? Win : Wout; d.M = B * d.Hg * d.Wg;
}
int run_wgrad(WgradDesc& d, hipStream_t s, Operand form, bool fixed_order) {
    if (!d.x1) d.c1 = 0;      // (the sweep's t = 0 has no h operand: its launch differentiates the x rows only)
    d.cin = d.c0 + d.c1;
    if (d.tcount < 1) d.tcount = 1;
    const long long b0 = view_bytes(d.B, d.Hx, d.Wx, d.ld0), b1 = d.x1 ? view_bytes(d.B, d.Hx, d.Wx, d.ld1) : 0, by = view_bytes(d.B, d.Hy, d.Wy, d.ldy);
    if (!fits31(b0) || (d.x1 && !fits31(b1)) || !fits31(by)) return PIVP_ERR_BADARG;
    d.bytes0 = (int)b0; d.bytes1 = (int)b1; d.bytesy = (int)by;
    d.operand = form;
    if (form == Operand::F32) { const int rc = igemm_wgrad_check(d); if (rc != PIVP_OK) return rc; }
    const WgradLaunch L = wgrad_launch(d, d.part != nullptr);
    // a deterministic sweep's launch: pivp_plan_set_deterministic (det_supported, plan_setup.hip) asked wgrad_launch the same question through
    // lstm_wgrad_part_floats and conv_backward_fixed_order below, so this does not happen
    if (fixed_order && !wgrad_fixed_order(L.form)) return PIVP_ERR_STATE;
    int rc = igemm_wgrad(d, L, s);
    if (rc != PIVP_OK || !d.db || L.bias_rides) return rc;
    for (int j = 0; j < d.tcount; ++j) {      // the kernel that ran does not sum dy's columns: one bias_grad launch per timestep
        rc = bias_grad(reinterpret_cast<const float*>(reinterpret_cast<const char*>(d.dy) + j * d.ts_dy), d.ldy, d.N, d.B * d.Hy * d.Wy, d.db, s);
        if (rc != PIVP_OK) return rc;
    }
    return PIVP_OK;
}
// the shape's launch with a partial buffer, as the launch itself will ask for it
static WgradLaunch lstm_wgrad_launch(int cx, int C, int has_h, int B, int H, int W, int slot_ntw, int slot_j) {
    WgradDesc d;
    lstm_wgrad_geom(d, cx, C, B, H, W);
    d.slot_ntw = slot_ntw; d.slot_j = slot_j;
    if (!has_h) { d.c1 = 0; d.cin = cx; }
    return wgrad_launch(d, true);
}
long long conv_backward_part_floats(int mode, int cin, int cout, int B, int Hin, int Win) {
    WgradDesc d;
    conv3x3s2_wgrad_geom(d, mode, cin, cout, B, Hin, Win);
    return wgrad_launch(d, true).part_floats;
}
bool conv_backward_fixed_order(int mode, int cin, int cout, int B, int Hin, int Win) {
    WgradDesc d;
    conv3x3s2_wgrad_geom(d, mode, cin, cout, B, Hin, Win);
    return wgrad_fixed_order(wgrad_launch(d, true).form);
}
// (the sweep's t = 0 has no h operand: its launch differentiates the x rows only -- fewer tiles, another partition of the same buffer, reduced on its own)
long long lstm_wgrad_part_floats(int cx, int C, int B, int H, int W, int slot_ntw, int slot_j) {
    WgradDesc d;
    lstm_wgrad_geom(d, cx, C, B, H, W);
    if (!wp_ok_shape(wgrad_shape(d))) return 0;      // in front of wgrad_launch: the entries that size by this hand it unchecked widths, and the other forms' grid rules divide by them
    const WgradLaunch full = lstm_wgrad_launch(cx, C, 1, B, H, W, slot_ntw, slot_j);
    const WgradLaunch xonly = lstm_wgrad_launch(cx, C, 0, B, H, W, slot_ntw, slot_j);
    return full.part_floats > xonly.part_floats ? full.part_floats : xonly.part_floats;
}
int lstm_wgrad_reduce(int cx, int C, int has_h, float* part, float* dW, float* db, int B, int H, int W, hipStream_t s, int slot_ntw, int slot_j) {
    WgradDesc d;
    lstm_wgrad_geom(d, cx, C, B, H, W);
    d.slot_ntw = slot_ntw; d.slot_j = slot_j;
    if (!has_h) { d.c1 = 0; d.cin = cx; }
    d.part = part; d.dw = dW; d.db = db;
    return igemm_wgrad_reduce(d, s);
}

// ---- backward ----
int run_convlstm_backward(const ConvLstmBwdArgs& a, hipStream_t s) {
    const int B = a.B, H = a.H, W = a.W, cx = a.cx, C = a.C, det = a.det;
    const int M = B * H * W, cin = cx + C, N = 4 * C;
    if ((a.wt_bf16 != nullptr) != (a.operand != Operand::F32) || (operand_needs_scale(a.operand) && !a.dg_absmax)) return PIVP_ERR_BADARG;
    // a K-split data gradient adds into d_in: the gate kernel clears it on the side (one launch less than a memset per cell and timestep).
    // det (deterministic sweeps): never split, so that every element of d_in is one block's plain store.
    const bool zero = a.wt_bf16 ? conv5x5_bf16_splits_k(N, cin, cin, B, H, W, a.operand, det)
                                : (a.dx_only ? conv_s1_splits_k(N, cx, cin, 5, B, H, W, cin, det) : conv_s1_splits_k(N, cin, cin, 5, B, H, W, 0, det));
    int rc = lstm_gates_bwd(a.gates, a.c_old, a.c_new, a.dh_a, a.lda, a.dh_b, a.ldb, a.dc, a.dc_valid, a.dG, M, C, s, B, a.ln, zero ? a.d_in : nullptr, (long long)M * cin);
    if (rc != PIVP_OK) return rc;
    if (a.dg_absmax) {      // fp16 pieces: dG's power-of-two scale from its largest |value| (gradients lie far below fp16's normal range); in front of the
        // fork, because the weight gradient on the side stream reads it too.
        // (The maximum taken by the gate backward itself -- an atomic maximum of float bits per wave, behind a "can I raise it" load -- instead of this
        // launch was built and measured: the train step 21.5 ms against 21.1 with the launch, 22.5 with three bf16 pieces.  Removed.)
        rc = absmax_partials(a.dG, (long)M * N, a.dg_absmax, s);
        if (rc != PIVP_OK) return rc;
    }
    // dG is final: the weight gradient can start (on the side stream when forked), next to this layer's own data gradient
    hipStream_t sw;
    rc = fork_begin(a.fork, s, &sw);
    if (rc != PIVP_OK) return rc;
    if (!a.wt_ready) {
        rc = repack_transpose(a.w, a.wt, 25, cin, N, 1, s);                   // [25][cin/32][4C][32] -> flipped [25][4C/32][cin][32]
        if (rc != PIVP_OK) return rc;
    }
    if (a.wt_bf16) {   // the data gradient on bf16 operands or pieces (wt_bf16 = the pack of wt in that form, built here unless wt_ready)
        if (!a.wt_ready) {
            rc = pack_lstm_bf16(a.wt, a.wt_bf16, N, cin, s, a.operand, conv5x5_bf16_rows(cin), 1);      // (L2-direct forms: the fragment-major plain pack, every map width)
            if (rc != PIVP_OK) return rc;
        }
        Conv5x5Bf16Opts o{};
        o.operand = a.operand; o.dest_zeroed = zero; o.ascale_part = a.dg_absmax; o.ep = a.ep; o.no_split = det;
        rc = run_conv5x5_bf16(a.dG, N, N, a.wt_bf16, a.d_in, cin, cin, 0, B, H, W, s, o);
    } else {
        if (a.ep && a.ep->applied) *a.ep->applied = 0;      // (the fp32 data-gradient kernels have no such hook)
        // d[x,h] = conv5x5(dG, W^T flipped); dx_only: the x columns alone (the pack's first cx of cin; the h columns of d_in stay unwritten)
        ConvS1Opts o{};
        o.dest_zeroed = zero; o.no_split = det;
        if (a.dx_only) o.wN = cin;
        rc = run_conv_s1(a.dG, N, N, a.wt, a.d_in, a.dx_only ? cx : cin, cin, 5, B, H, W, s, o);
    }
    if (rc != PIVP_OK) return rc;
    if (!a.dW) return PIVP_OK;   // the caller batches this layer's weight gradient over several timesteps itself (plan_backward.hip)
    // (a single timestep's weight gradient: bf16 operands in that form, the fp32 kernel in every other)
    WgradDesc d;
    lstm_wgrad_geom(d, cx, C, B, H, W);
    d.x0 = a.x; d.ld0 = a.ldx; d.x1 = a.h_prev; d.dy = a.dG; d.dw = a.dW; d.db = a.db;
    rc = run_wgrad(d, sw, a.operand == Operand::BF16 ? Operand::BF16 : Operand::F32);
    if (rc != PIVP_OK) return rc;
    return fork_end(a.fork);
}

int run_layernorm(const float* x, const float* g, const float* b, float* out, float* partials, int B, int n, int C,
                  int ldo, float eps, int relu, hipStream_t s, const LayerNormOpts& o) {
    if (o.fused_nparts <= 0) {
        int rc = ln_stats(x, partials, B, n, s);
        if (rc != PIVP_OK) return rc;
    }
    return ln_apply(x, partials, g, b, out, B, n, C, ldo, eps, relu, s, o.stat_out, o.fused_nparts);
}

__global__ __launch_bounds__(256) void select_frames_kernel(const float* __restrict__ gt, const float* __restrict__ gen,
                                                            const unsigned char* __restrict__ take, float* __restrict__ out,
                                                            int frame_numel) {
    const int b = blockIdx.y;
    const float* src = take[b] ? gt : gen;
    const size_t base = (size_t)b * frame_numel;
    for (int i = (blockIdx.x * 256 + threadIdx.x) * 4; i < frame_numel; i += gridDim.x * 1024)
        *reinterpret_cast<f32x4*>(out + base + i) = *reinterpret_cast<const f32x4*>(src + base + i);
}

int run_select_frames(const float* gt, const float* gen, const unsigned char* take, float* out, int B, int frame_numel, hipStream_t s) {
    if (!gt || !gen || !take || !out || B <= 0 || frame_numel <= 0 || frame_numel % 4) return PIVP_ERR_BADARG;
    hipLaunchKernelGGL(select_frames_kernel, dim3(8, B), dim3(256), 0, s, gt, gen, take, out, frame_numel);
    return PIVP_LAUNCH_STATUS();
}

int run_conv_backward(const ConvBwdArgs& a, hipStream_t s) {
    const int mode = a.mode, B = a.B, Hin = a.Hin, Win = a.Win;
    const int Hout = mode ? 2 * Hin : Hin / 2, Wout = mode ? 2 * Win : Win / 2;
    int rc = PIVP_OK;
    if (a.y) { rc = relu_mask(a.dy, a.ldy, a.y, a.ldyy, a.cout, (long)B * Hout * Wout, s, a.dy_add, a.ld_add); if (rc != PIVP_OK) return rc; }
    else if (a.dy_add) { rc = add_strided(a.dy, a.ldy, a.dy_add, a.ld_add, a.cout, (long)B * Hout * Wout, s); if (rc != PIVP_OK) return rc; }
    hipStream_t sw;
    rc = fork_begin(a.fork, s, &sw);      // dy is final here
    if (rc != PIVP_OK) return rc;
    if (a.dx) {
        if (!a.wt_ready) {
            rc = repack_transpose(a.w, a.wt, 9, a.cin, a.cout, 0, s);
            if (rc != PIVP_OK) return rc;
        }
        DeconvOpts o{};
        o.accum = a.accum_dx; o.operand = a.operand;
        rc = mode ? run_conv3x3s2(a.dy, a.cout, a.ldy, a.wt, nullptr, a.dx, a.cin, a.lddx, 0, B, Hout, Wout, s, a.accum_dx)
                  : run_deconv3x3s2(a.dy, a.cout, a.ldy, a.wt, nullptr, a.dx, a.cin, a.lddx, 0, B, Hout, Wout, s, o);
        if (rc != PIVP_OK) return rc;
    }
    if (!a.dW) return PIVP_OK;     // the caller batches this layer's weight gradient over several timesteps itself (plan_backward.hip); the fork's `ready` is recorded
    WgradDesc d;
    conv3x3s2_wgrad_geom(d, mode, a.cin, a.cout, B, Hin, Win);
    d.x0 = a.x; d.ld0 = a.ldx; d.dy = a.dy; d.ldy = a.ldy; d.dw = a.dW; d.db = a.db; d.part = a.part;
    rc = run_wgrad(d, sw, Operand::F32);
    if (rc != PIVP_OK) return rc;
    return fork_end(a.fork);
}

}  // namespace pivp

#ifndef PIVP_BUILD_DIGEST
#define PIVP_BUILD_DIGEST "unstamped"      // a build that did not go through build.py: _lib.load() refuses it
#endif
extern "C" const char* pivp_build_digest(void) { return PIVP_BUILD_DIGEST; }
#ifndef PIVP_BUILD_FLAGS
#define PIVP_BUILD_FLAGS ""                // the compile flags beyond build.py's standard set (PIVP_EXTRA_FLAGS): "" = the product build
#endif
extern "C" const char* pivp_build_flags(void) { return PIVP_BUILD_FLAGS; }
extern "C" int pivp_abi_version(void) { return 17; }   // 9: + pivp_build_digest, pivp_grad_sum_shards, pivp_frame_head; 8: + pivp_gates_backward_ln (op entry of the norm + gate backward pair); 7: + bf16 gradient payload, batched bf16 weight gradient, partial-plane / dx-only op entries

// the epilogue hook's arguments as the op entries take them: a mode of 0..2, and a source that covers the columns the hook is applied to
static bool ep_args_ok(const float* ep_src, int ep_ld, int ep_cols, int ep_mode, int cout) {
    if (ep_mode < 0 || ep_mode > 2) return false;
    if (!ep_src || !ep_mode) return true;      // the plain conv
    return ep_ld >= (ep_cols < cout ? ep_cols : cout);
}
// a packed-operand form runs on the maps its kernels' tiles serve (pivp_kernels.h): asked in front of an entry's first launch, so that a refusal leaves nothing behind
static bool form_serves_map(Operand form, int B, int H, int W) { return form == Operand::F32 || packed_tiles_serve(H, W, B); }
extern "C" int pivp_convlstm(const float* x, int cx, int ldx, const float* h_prev, int C, const float* w, const float* bias,
                             const float* c_in, float* c_out, float* h_out, int B, int H, int W, void* stream) {
    if (!x || !w || !bias || !c_in || !c_out || !h_out) return PIVP_ERR_BADARG;
    return run_convlstm(x, cx, ldx, h_prev, C, w, bias, c_in, c_out, h_out, B, H, W, (hipStream_t)stream);
}
extern "C" int pivp_convlstm_v(const float* x, int cx, int ldx, const float* h_prev, int C, const float* w, const float* bias,
                               const float* c_in, float* c_out, float* h_out, int B, int H, int W, int variant, void* stream) {
    if (!x || !w || !bias || !c_in || !c_out || !h_out || variant < 0 || variant > 4) return PIVP_ERR_BADARG;
    ConvLstmOpts o{};
    o.variant = variant;
    return run_convlstm(x, cx, ldx, h_prev, C, w, bias, c_in, c_out, h_out, B, H, W, (hipStream_t)stream, o);
}
extern "C" int pivp_convlstm_train(const float* x, int cx, int ldx, const float* h_prev, int C, const float* w, const float* bias,
                                   const float* c_in, float* c_out, float* h_out, float* gates_out, int B, int H, int W, void* stream) {
    if (!x || !w || !bias || !c_in || !c_out || !h_out || !gates_out) return PIVP_ERR_BADARG;
    ConvLstmOpts o{};
    o.gates_out = gates_out;
    return run_convlstm(x, cx, ldx, h_prev, C, w, bias, c_in, c_out, h_out, B, H, W, (hipStream_t)stream, o);
}
// the cell backward of the op entries: everything on `stream`, transposed pack built by the call, weight gradient included
static int convlstm_backward_op(const float* x, int cx, int ldx, const float* h_prev, int C, const float* w, const float* gates,
                                const float* c_old, const float* c_new, const float* dh_a, int lda, const float* dh_b, int ldb,
                                float* dc, int dc_valid, float* dG, float* wt, float* d_in, float* dW, float* db,
                                int B, int H, int W, void* stream, int dx_only) {
    if (!x || !w || !gates || !c_old || !c_new || !dc || !dG || !wt || !d_in || !dW || !db) return PIVP_ERR_BADARG;
    ConvLstmBwdArgs a{};
    a.x = x; a.cx = cx; a.ldx = ldx; a.h_prev = h_prev; a.C = C; a.w = w; a.gates = gates; a.c_old = c_old; a.c_new = c_new;
    a.dh_a = dh_a; a.lda = lda; a.dh_b = dh_b; a.ldb = ldb; a.dc = dc; a.dc_valid = dc_valid; a.dG = dG; a.wt = wt; a.d_in = d_in;
    a.dW = dW; a.db = db; a.B = B; a.H = H; a.W = W;
    a.dx_only = dx_only;
    return run_convlstm_backward(a, (hipStream_t)stream);
}
extern "C" int pivp_convlstm_backward(const float* x, int cx, int ldx, const float* h_prev, int C, const float* w, const float* gates,
                                      const float* c_old, const float* c_new, const float* dh_a, int lda, const float* dh_b, int ldb,
                                      float* dc, int dc_valid, float* dG, float* wt, float* d_in, float* dW, float* db,
                                      int B, int H, int W, void* stream) {
    return convlstm_backward_op(x, cx, ldx, h_prev, C, w, gates, c_old, c_new, dh_a, lda, dh_b, ldb, dc, dc_valid, dG, wt, d_in, dW, db, B, H, W, stream, 0);
}
// conv3x3s2 (mode 0) / deconv3x3s2 (mode 1) backward given dy (already ReLU-masked): dx (optionally accumulated), dW, db
extern "C" int pivp_conv_backward(int mode, const float* x, int cin, int ldx, const float* w, const float* dy, int cout, int ldy,
                                  float* wt, float* dx, int lddx, int accum_dx, float* dW, float* db, int B, int Hin, int Win,
                                  void* stream) {
    if (!x || !w || !dy || !wt || !dW || !db || mode < 0 || mode > 1) return PIVP_ERR_BADARG;
    ConvBwdArgs a{};
    a.mode = mode; a.x = x; a.cin = cin; a.ldx = ldx; a.w = w; a.dy = const_cast<float*>(dy); a.cout = cout; a.ldy = ldy;
    a.wt = wt; a.dx = dx; a.lddx = lddx; a.accum_dx = accum_dx; a.dW = dW; a.db = db; a.B = B; a.Hin = Hin; a.Win = Win;
    return run_conv_backward(a, (hipStream_t)stream);
}
// The weight-gradient half of pivp_conv_backward as the BPTT sweep runs it: `repeats` launches (one per timestep there; here the same
// operands every time) add their tiles into the per-block partial planes `part` (pivp_conv_backward_part_floats floats, zeroed by the
// caller) with plain loads and stores, then ONE reduction sums the pixel splits into dW; db is accumulated on the side by the tap blocks
// that see every dy element once.  Result: dW += repeats * (x^T . dy per tap), db += repeats * column sums of dy.
extern "C" long long pivp_conv_backward_part_floats(int mode, int cin, int cout, int B, int Hin, int Win) {
    if (mode < 0 || mode > 1 || cin <= 0 || cout <= 0 || B <= 0 || Hin <= 0 || Win <= 0) return PIVP_ERR_BADARG;
    return conv_backward_part_floats(mode, cin, cout, B, Hin, Win);
}
extern "C" int pivp_conv_wgrad_partial(int mode, const float* x, int cin, int ldx, const float* dy, int cout, int ldy, float* part,
                                       float* dW, float* db, int B, int Hin, int Win, int repeats, void* stream) {
    if (!x || !dy || !part || !dW || !db || mode < 0 || mode > 1 || repeats < 1) return PIVP_ERR_BADARG;
    WgradDesc desc;
    conv3x3s2_wgrad_geom(desc, mode, cin, cout, B, Hin, Win);
    desc.x0 = x; desc.ld0 = ldx; desc.dy = dy; desc.ldy = ldy; desc.dw = dW; desc.db = db; desc.part = part;
    for (int r = 0; r < repeats; ++r) {
        const int rc = run_wgrad(desc, (hipStream_t)stream, Operand::F32);
        if (rc != PIVP_OK) return rc;
    }
    return igemm_wgrad_reduce(desc, (hipStream_t)stream);
}
// One launch of that weight gradient over a BATCH of timesteps (WgradDesc::tcount; operand j at x + j * x_step_bytes, dy + j * dy_step_bytes,
// negative steps allowed: the sweep walks the forward slabs backwards) into the partial planes -- overwrite != 0: stored, not added (the planes'
// first launch needs no zeroing) -- and the reduction into dW as a call of its own.
extern "C" int pivp_conv_wgrad_partial_batch(int mode, const float* x, int cin, int ldx, long long x_step_bytes, const float* dy, int cout, int ldy,
                                             long long dy_step_bytes, int tcount, int overwrite, float* part, float* dW, float* db, int B, int Hin, int Win,
                                             void* stream) {
    if (!x || !dy || !part || !dW || !db || mode < 0 || mode > 1 || tcount < 1) return PIVP_ERR_BADARG;
    WgradDesc d;
    conv3x3s2_wgrad_geom(d, mode, cin, cout, B, Hin, Win);
    d.x0 = x; d.ld0 = ldx; d.dy = dy; d.ldy = ldy; d.dw = dW; d.db = db;
    d.tcount = tcount; d.ts_x0 = x_step_bytes; d.ts_dy = dy_step_bytes;
    d.part = part; d.part_overwrite = overwrite ? 1 : 0;
    return run_wgrad(d, (hipStream_t)stream, Operand::F32);
}
extern "C" int pivp_conv_wgrad_partial_reduce(int mode, int cin, int cout, float* part, float* dW, float* db, int B, int Hin, int Win, void* stream) {
    if (!part || !dW || !db || mode < 0 || mode > 1) return PIVP_ERR_BADARG;
    WgradDesc d;
    conv3x3s2_wgrad_geom(d, mode, cin, cout, B, Hin, Win);
    d.part = part; d.dw = dW; d.db = db;      // (the nine-tap kernel leaves its column sums in the planes: the reduction adds them into db)
    return igemm_wgrad_reduce(d, (hipStream_t)stream);
}
// The fp32 ConvLSTM weight gradient on its own (the sweep runs it on the side stream): a batch of `tcount` timesteps per launch as pivp_wgrad5x5_bf16_batch.
// part == NULL: the round-2 kernel (atomics straight into dW / db).  part != NULL (pivp_wgrad5x5_f32_part_floats floats): the round-6 kernel adds -- overwrite
// != 0: stores -- its segments into the partial slots; pivp_wgrad5x5_f32_reduce then adds the slots' sum into dW and db (fixed order: bit-reproducible).
// the ConvLSTM weight-gradient entries' common operands: a batch of tcount timesteps, operand j at byte offsets j * ts_*
static void lstm_wgrad_op(WgradDesc& d, const float* x, int cx, int ldx, const float* h_prev, int C, const float* dG, float* dW, float* db,
                          int B, int H, int W, int tcount, long long ts_x, long long ts_h, long long ts_dG) {
    lstm_wgrad_geom(d, cx, C, B, H, W);
    d.x0 = x; d.ld0 = ldx; d.x1 = h_prev; d.dy = dG; d.dw = dW; d.db = db;
    d.tcount = tcount; d.ts_x0 = ts_x; d.ts_x1 = ts_h; d.ts_dy = ts_dG;
}
extern "C" long long pivp_wgrad5x5_f32_part_floats(int cx, int C, int B, int H, int W, int form) {
    if (cx <= 0 || C <= 0 || B <= 0 || H <= 0 || W <= 0 || form < 0 || form > 2) return PIVP_ERR_BADARG;
    return lstm_wgrad_part_floats(cx, C, B, H, W, form, 0);
}
extern "C" int pivp_wgrad5x5_f32_batch(const float* x, int cx, int ldx, const float* h_prev, int C, const float* dG, float* part, int overwrite,
                                       float* dW, float* db, int B, int H, int W, int tcount, long long ts_x, long long ts_h, long long ts_dG, int form,
                                       void* stream) {
    if (!x || !dG || !dW || tcount < 1 || form < 0 || form > 2 || (part && lstm_wgrad_part_floats(cx, C, B, H, W, form, 0) <= 0)) return PIVP_ERR_BADARG;
    WgradDesc d;
    lstm_wgrad_op(d, x, cx, ldx, h_prev, C, dG, dW, db, B, H, W, tcount, ts_x, ts_h, ts_dG);
    d.part = part; d.part_overwrite = overwrite ? 1 : 0;
    d.form = form; d.slot_ntw = form;      // (form: the wave form without part, the slot form's columns per wave with it)
    return run_wgrad(d, (hipStream_t)stream, Operand::F32);
}
extern "C" int pivp_wgrad5x5_f32_reduce(int cx, int C, int has_h, float* part, float* dW, float* db, int B, int H, int W, int form, void* stream) {
    if (!part || !dW || form < 0 || form > 2 || lstm_wgrad_part_floats(cx, C, B, H, W, form, 0) <= 0) return PIVP_ERR_BADARG;
    return lstm_wgrad_reduce(cx, C, has_h, part, dW, db, B, H, W, (hipStream_t)stream, form, 0);      // (slot_j = 0: blocks per XCD by the device's CU count)
}
// The slot kernel's partition walked on the host (no GPU work): geom8 = {blocks per XCD, pixel parts, tile parts, 32-column tiles per wave, tiles, 16-pixel chunks per
// timestep, slots per block, floats per slot}; segs: (block, segment, tile, first chunk, end chunk) per segment in kernel order; slots: (tile, slot) pairs in the
// reduction's order.  The caps bound what is written; the counts are always returned.  tests/test_host.py checks that every (tile, chunk) is covered exactly once and
// that the reduction reads exactly the slots the kernel writes.
extern "C" int pivp_wgrad5x5_f32_partition(int cx, int C, int has_h, int B, int H, int W, int form, int* geom8, int* segs, int seg_cap, int* nsegs,
                                           int* slots, int slot_cap, int* nslots) {
    if (cx <= 0 || C <= 0 || B <= 0 || H <= 0 || W <= 0 || form < 0 || form > 2 || !geom8 || !nsegs || !nslots) return PIVP_ERR_BADARG;
    WgradDesc d;
    lstm_wgrad_geom(d, cx, C, B, H, W);
    d.slot_ntw = form;
    if (!has_h) { d.c1 = 0; d.cin = cx; }
    return wgrad5x5p_partition(d, geom8, segs, seg_cap, nsegs, slots, slot_cap, nslots);
}
// The fp32 ConvLSTM data gradient on its own: a plain 5x5 stride-1 pad-2 convolution of x [B*H*W][cin] with wt (packed [25][cin/32][cout][32]: for the data
// gradient the flipped, transposed weight) into out [B*H*W][cout] (contiguous); tile and K split as the sweep chooses them (out is cleared first when K is split).
extern "C" int pivp_conv5x5_f32(const float* x, int cin, int ldx, const float* wt, float* out, int cout, int B, int H, int W, void* stream) {
    if (!x || !wt || !out) return PIVP_ERR_BADARG;
    return run_conv_s1(x, cin, ldx, wt, out, cout, cout, 5, B, H, W, (hipStream_t)stream);
}
// pivp_convlstm_backward for the sweep's LAST timestep (t = 0): nobody reads d h_{-1}, so only the cx columns of d_in are computed
// (the data gradient runs on the first cx columns of the transposed weight pack) and the h columns of d_in are not computed (left as they are, or cleared with the rest of d_in for a K-split data gradient).
extern "C" int pivp_convlstm_backward_dx_only(const float* x, int cx, int ldx, const float* h_prev, int C, const float* w, const float* gates,
                                              const float* c_old, const float* c_new, const float* dh_a, int lda, const float* dh_b, int ldb,
                                              float* dc, int dc_valid, float* dG, float* wt, float* d_in, float* dW, float* db,
                                              int B, int H, int W, void* stream) {
    return convlstm_backward_op(x, cx, ldx, h_prev, C, w, gates, c_old, c_new, dh_a, lda, dh_b, ldb, dc, dc_valid, dG, wt, d_in, dW, db, B, H, W, stream, 1);
}
// The cell backward with the data gradient in the form of a precision mode, as the sweep's lstmb (plan_backward.hip) fills ConvLstmBwdArgs: the pack of wt in that
// form and dG's partial maxima live in `scratch` (pivp_convlstm_backward_form_scratch_floats), the epilogue hook and det are passed through.  precision 0 is
// pivp_convlstm_backward / _dx_only (scratch and the hook unused).  Everything that is refused is refused in front of the first launch.
extern "C" long long pivp_convlstm_backward_form_scratch_floats(int cx, int C) {
    if (cx <= 0 || C <= 0 || (cx + C) % 32) return PIVP_ERR_BADARG;
    // up to three planes of the pack + the fp16 pack's tail (256 2-byte elements), then 72 floats of partial maxima
    return (3 * (long long)lstm_bf16_weight_elems(4 * C, conv5x5_bf16_rows(cx + C)) + 256) / 2 + 72;
}
extern "C" int pivp_convlstm_backward_form(int precision, const float* x, int cx, int ldx, const float* h_prev, int C, const float* w, const float* gates,
                                           const float* c_old, const float* c_new, const float* dh_a, int lda, const float* dh_b, int ldb,
                                           float* dc, int dc_valid, float* dG, float* wt, float* d_in, float* dW, float* db, float* scratch,
                                           const float* ep_src, int ep_ld, int ep_cols, int ep_mode, int* ep_applied, int det, int dx_only,
                                           int B, int H, int W, void* stream) {
    if (ep_applied) *ep_applied = 0;
    if (precision < 0 || precision > 4 || !x || !w || !gates || !c_old || !c_new || !dc || !dG || !wt || !d_in || !dW || !db || cx <= 0 || C <= 0 ||
        B <= 0 || H <= 0 || W <= 0)
        return PIVP_ERR_BADARG;
    const Operand form = (Operand)precision;
    if ((form != Operand::F32 && (!scratch || (cx + C) % 32)) || !form_serves_map(form, B, H, W) || !ep_args_ok(ep_src, ep_ld, ep_cols, ep_mode, cx + C))
        return PIVP_ERR_BADARG;
    const EpSpec ep{ep_src, ep_ld, ep_cols, ep_mode, ep_applied};
    ConvLstmBwdArgs a{};
    a.x = x; a.cx = cx; a.ldx = ldx; a.h_prev = h_prev; a.C = C; a.w = w; a.gates = gates; a.c_old = c_old; a.c_new = c_new;
    a.dh_a = dh_a; a.lda = lda; a.dh_b = dh_b; a.ldb = ldb; a.dc = dc; a.dc_valid = dc_valid; a.dG = dG; a.wt = wt; a.d_in = d_in;
    a.dW = dW; a.db = db; a.B = B; a.H = H; a.W = W;
    a.dx_only = dx_only ? 1 : 0; a.det = det ? 1 : 0;
    a.operand = form;
    if (form != Operand::F32) {
        a.wt_bf16 = reinterpret_cast<unsigned short*>(scratch);
        if (operand_needs_scale(form)) a.dg_absmax = scratch + pivp_convlstm_backward_form_scratch_floats(cx, C) - 72;
        if (ep_src && ep_mode) a.ep = &ep;
    }
    return run_convlstm_backward(a, (hipStream_t)stream);
}
extern "C" int pivp_layernorm_train(const float* x, const float* gamma, const float* beta, float* out, float* partials, float* stat,
                                    int B, int n, int C, int ldo, float eps, int relu, void* stream) {
    if (!stat) return PIVP_ERR_BADARG;
    LayerNormOpts o{};
    o.stat_out = stat;
    return run_layernorm(x, gamma, beta, out, partials, B, n, C, ldo, eps, relu, (hipStream_t)stream, o);
}
// bf16-operand ConvLSTM (BASELINE.json config 3): weights re-packed to bf16 once, operands rounded to bf16 on the way into LDS,
// fp32 accumulation / gates / state.  nch: 0 automatic, 16 or 32 channels per block.
// Split mode (three bf16 MFMAs per product, 16 bits of product mantissa): weights packed as hi / lo planes, twice the elements.
// the packed-weight ConvLSTM entries' options
static ConvLstmOpts packed_lstm_opts(const void* w_bf16, Operand form, int nch, float* gates_out, float* ln_part, int ln_cap, int* ln_nparts) {
    ConvLstmOpts o{};
    o.w_bf16 = (const unsigned short*)w_bf16; o.operand = form; o.variant = nch; o.gates_out = gates_out;
    o.ln_out.part = ln_part; o.ln_out.cap = ln_cap; o.ln_out.nparts = ln_nparts;
    return o;
}
extern "C" int pivp_pack_lstm_bf16x3(const float* w, void* w_bf16, int cin_total, int C, void* stream) {
    if (C <= 0) return PIVP_ERR_BADARG;
    return pack_lstm_bf16(w, (unsigned short*)w_bf16, cin_total, 4 * C, (hipStream_t)stream, Operand::BF16X3);
}
extern "C" int pivp_convlstm_bf16x3(const float* x, int cx, int ldx, const float* h_prev, int C, const void* w_bf16, const float* bias,
                                    const float* c_in, float* c_out, float* h_out, float* gates_out, float* ln_part, int ln_cap,
                                    int* ln_nparts, int B, int H, int W, int nch, void* stream) {
    if (!x || !w_bf16 || !bias || !c_in || !c_out || !h_out) return PIVP_ERR_BADARG;
    const ConvLstmOpts o = packed_lstm_opts(w_bf16, Operand::BF16X3, nch, gates_out, ln_part, ln_cap, ln_nparts);
    return run_convlstm(x, cx, ldx, h_prev, C, nullptr, bias, c_in, c_out, h_out, B, H, W, (hipStream_t)stream, o);
}
extern "C" int pivp_pack_lstm_bf16x6(const float* w, void* w_bf16, int cin_total, int C, void* stream) {
    if (C <= 0) return PIVP_ERR_BADARG;
    return pack_lstm_bf16(w, (unsigned short*)w_bf16, cin_total, 4 * C, (hipStream_t)stream, Operand::BF16X6);
}
extern "C" int pivp_convlstm_bf16x6(const float* x, int cx, int ldx, const float* h_prev, int C, const void* w_bf16, const float* bias,
                                    const float* c_in, float* c_out, float* h_out, float* gates_out, float* ln_part, int ln_cap,
                                    int* ln_nparts, int B, int H, int W, int nch, void* stream) {
    if (!x || !w_bf16 || !bias || !c_in || !c_out || !h_out || (nch != 0 && nch != 16 && nch != 32)) return PIVP_ERR_BADARG;
    const ConvLstmOpts o = packed_lstm_opts(w_bf16, Operand::BF16X6, nch, gates_out, ln_part, ln_cap, ln_nparts);
    return run_convlstm(x, cx, ldx, h_prev, C, nullptr, bias, c_in, c_out, h_out, B, H, W, (hipStream_t)stream, o);
}
extern "C" int pivp_pack_lstm_fp16x3(const float* w, void* w_bf16, int cin_total, int C, int map_width, void* stream) {
    if (C <= 0 || map_width <= 0) return PIVP_ERR_BADARG;
    // (fragment-major for every map width; map_width is kept in the signature for ABI stability)
    return pack_lstm_bf16(w, (unsigned short*)w_bf16, cin_total, 4 * C, (hipStream_t)stream, Operand::FP16X3);
}
extern "C" int pivp_convlstm_fp16x3(const float* x, int cx, int ldx, const float* h_prev, int C, const void* w_bf16, const float* bias,
                                    const float* c_in, float* c_out, float* h_out, float* gates_out, float* ln_part, int ln_cap,
                                    int* ln_nparts, int B, int H, int W, int nch, void* stream) {
    if (!x || !w_bf16 || !bias || !c_in || !c_out || !h_out || (nch != 0 && nch != 16 && nch != 32 && nch != 256)) return PIVP_ERR_BADARG;
    const ConvLstmOpts o = packed_lstm_opts(w_bf16, Operand::FP16X3, nch, gates_out, ln_part, ln_cap, ln_nparts);
    return run_convlstm(x, cx, ldx, h_prev, C, nullptr, bias, c_in, c_out, h_out, B, H, W, (hipStream_t)stream, o);
}
extern "C" long long pivp_lstm_bf16_weight_elems(int cin_total, int C) {
    if (cin_total <= 0 || cin_total % 32 || C <= 0) return PIVP_ERR_BADARG;
    return (long long)lstm_bf16_weight_elems(cin_total, 4 * C);
}
extern "C" int pivp_pack_lstm_bf16(const float* w, void* w_bf16, int cin_total, int C, void* stream) {
    if (C <= 0) return PIVP_ERR_BADARG;
    return pack_lstm_bf16(w, (unsigned short*)w_bf16, cin_total, 4 * C, (hipStream_t)stream, Operand::BF16);
}
extern "C" int pivp_convlstm_bf16(const float* x, int cx, int ldx, const float* h_prev, int C, const void* w_bf16, const float* bias,
                                  const float* c_in, float* c_out, float* h_out, float* gates_out, float* ln_part, int ln_cap,
                                  int* ln_nparts, int B, int H, int W, int nch, void* stream) {
    if (!x || !w_bf16 || !bias || !c_in || !c_out || !h_out) return PIVP_ERR_BADARG;
    const ConvLstmOpts o = packed_lstm_opts(w_bf16, Operand::BF16, nch, gates_out, ln_part, ln_cap, ln_nparts);
    return run_convlstm(x, cx, ldx, h_prev, C, nullptr, bias, c_in, c_out, h_out, B, H, W, (hipStream_t)stream, o);
}
// Plain 5x5 stride-1 "same" convolution with bf16 operands (the ConvLSTM data gradient of the bf16 mode): w fp32 K-inner packed
// [25][cin/32][cout][32]; w_bf16: scratch of pivp_conv5x5_bf16_weight_elems(cin, cout) 2-byte elements, (re)built by this call.
extern "C" long long pivp_conv5x5_bf16_weight_elems(int cin, int cout) {
    if (cin <= 0 || cin % 32 || cout <= 0) return PIVP_ERR_BADARG;
    return (long long)lstm_bf16_weight_elems(cin, conv5x5_bf16_rows(cout));
}
extern "C" int pivp_conv5x5_bf16(const float* x, int cin, int ldx, const float* w, void* w_bf16, float* out, int cout, int ldo, int accum,
                                 int B, int H, int W, void* stream) {
    if (!x || !w || !w_bf16 || !out || cin <= 0 || cout <= 0 || !form_serves_map(Operand::BF16, B, H, W)) return PIVP_ERR_BADARG;
    int rc = pack_lstm_bf16(w, (unsigned short*)w_bf16, cin, cout, (hipStream_t)stream, Operand::BF16, conv5x5_bf16_rows(cout));
    if (rc != PIVP_OK) return rc;
    Conv5x5Bf16Opts o{};
    o.operand = Operand::BF16;
    return run_conv5x5_bf16(x, cin, ldx, (const unsigned short*)w_bf16, out, cout, ldo, accum, B, H, W, (hipStream_t)stream, o);
}
// split form (two bf16 pieces per operand): w_bf16 holds 2 * pivp_conv5x5_bf16_weight_elems(cin, cout) elements
extern "C" int pivp_conv5x5_bf16x3(const float* x, int cin, int ldx, const float* w, void* w_bf16, float* out, int cout, int ldo, int accum,
                                   int B, int H, int W, void* stream) {
    if (!x || !w || !w_bf16 || !out || cin <= 0 || cout <= 0 || !form_serves_map(Operand::BF16X3, B, H, W)) return PIVP_ERR_BADARG;
    int rc = pack_lstm_bf16(w, (unsigned short*)w_bf16, cin, cout, (hipStream_t)stream, Operand::BF16X3, conv5x5_bf16_rows(cout));
    if (rc != PIVP_OK) return rc;
    Conv5x5Bf16Opts o{};
    o.operand = Operand::BF16X3;
    return run_conv5x5_bf16(x, cin, ldx, (const unsigned short*)w_bf16, out, cout, ldo, accum, B, H, W, (hipStream_t)stream, o);
}
// three-piece form (six MFMAs per product, fp32-grade): w_bf16 holds 3 * pivp_conv5x5_bf16_weight_elems(cin, cout) elements; W % 16 == 0
extern "C" int pivp_conv5x5_bf16x6(const float* x, int cin, int ldx, const float* w, void* w_bf16, float* out, int cout, int ldo, int accum,
                                   int B, int H, int W, void* stream) {
    if (!x || !w || !w_bf16 || !out || cin <= 0 || cout <= 0 || !form_serves_map(Operand::BF16X6, B, H, W)) return PIVP_ERR_BADARG;
    int rc = pack_lstm_bf16(w, (unsigned short*)w_bf16, cin, cout, (hipStream_t)stream, Operand::BF16X6, conv5x5_bf16_rows(cout), 1);
    if (rc != PIVP_OK) return rc;
    Conv5x5Bf16Opts o{};
    o.operand = Operand::BF16X6;
    return run_conv5x5_bf16(x, cin, ldx, (const unsigned short*)w_bf16, out, cout, ldo, accum, B, H, W, (hipStream_t)stream, o);
}
// two-fp16-piece form (three MFMAs per product, fp32-grade; the fp16x3 mode's data gradients): x is staged times the power of two that puts its largest
// |value| into [2^14, 2^15) (gradients lie far below fp16's normal range), w as in pivp_pack_lstm_fp16x3; w_bf16 holds 2 * pivp_conv5x5_bf16_weight_elems
// + 256 elements, scratch 66 floats (x's partial maxima); x contiguous (ldx == cin), W % 16 == 0 or W % 8 == 0 with an even batch
extern "C" int pivp_conv5x5_fp16x3(const float* x, int cin, int ldx, const float* w, void* w_bf16, float* out, int cout, int ldo, int accum,
                                   int B, int H, int W, float* scratch, void* stream) {
    if (!x || !w || !w_bf16 || !out || !scratch || cin <= 0 || cout <= 0 || ldx != cin || B <= 0 || H <= 0 || !form_serves_map(Operand::FP16X3, B, H, W)) return PIVP_ERR_BADARG;
    int rc = pack_lstm_bf16(w, (unsigned short*)w_bf16, cin, cout, (hipStream_t)stream, Operand::FP16X3, conv5x5_bf16_rows(cout), 1);
    if (rc != PIVP_OK) return rc;
    rc = absmax_partials(x, (long)B * H * W * cin, scratch, (hipStream_t)stream);
    if (rc != PIVP_OK) return rc;
    Conv5x5Bf16Opts o{};
    o.operand = Operand::FP16X3; o.ascale_part = scratch;
    return run_conv5x5_bf16(x, cin, ldx, (const unsigned short*)w_bf16, out, cout, ldo, accum, B, H, W, (hipStream_t)stream, o);
}
// Any of the four forms above by its precision code, with the data gradient's epilogue hook (IgemmDesc::ep_*) and the deterministic sweeps' no_split: what
// run_convlstm_backward launches, as an op.  Everything that is refused is refused in front of the first launch.
extern "C" int pivp_conv5x5_ep(int precision, const float* x, int cin, int ldx, const float* w, void* w_bf16, float* out, int cout, int ldo, int accum,
                               const float* ep_src, int ep_ld, int ep_cols, int ep_mode, int no_split, float* scratch, int* applied,
                               int B, int H, int W, void* stream) {
    if (applied) *applied = 0;
    if (precision < 1 || precision > 4 || !x || !w || !w_bf16 || !out || cin <= 0 || cout <= 0 || B <= 0 || H <= 0 || W <= 0) return PIVP_ERR_BADARG;
    const Operand form = (Operand)precision;
    if (!form_serves_map(form, B, H, W) || (operand_needs_scale(form) && (!scratch || ldx != cin)) || !ep_args_ok(ep_src, ep_ld, ep_cols, ep_mode, cout))
        return PIVP_ERR_BADARG;
    int rc = pack_lstm_bf16(w, (unsigned short*)w_bf16, cin, cout, (hipStream_t)stream, form, conv5x5_bf16_rows(cout), operand_l2_direct(form) ? 1 : 0);
    if (rc != PIVP_OK) return rc;
    if (operand_needs_scale(form)) {
        rc = absmax_partials(x, (long)B * H * W * cin, scratch, (hipStream_t)stream);
        if (rc != PIVP_OK) return rc;
    }
    const EpSpec ep{ep_src, ep_ld, ep_cols, ep_mode, applied};
    Conv5x5Bf16Opts o{};
    o.operand = form; o.no_split = no_split ? 1 : 0;
    if (operand_needs_scale(form)) o.ascale_part = scratch;
    if (ep_src && ep_mode) o.ep = &ep;
    return run_conv5x5_bf16(x, cin, ldx, (const unsigned short*)w_bf16, out, cout, ldo, accum, B, H, W, (hipStream_t)stream, o);
}
// host-only: the K split pivp_conv5x5_ep uses for these arguments on the current device (1: one block per output tile, the grid that takes the hook)
extern "C" int pivp_conv5x5_ep_ksplit(int precision, int cin, int cout, int ldo, int accum, int no_split, int B, int H, int W) {
    if (precision < 1 || precision > 4 || cin <= 0 || cout <= 0 || ldo < cout || B <= 0 || H <= 0 || W <= 0) return PIVP_ERR_BADARG;
    IgemmDesc d;
    static float dummy;
    if (conv5x5_bf16_desc(d, &dummy, cin, cin, &dummy, cout, ldo, accum, B, H, W) != PIVP_OK) return PIVP_ERR_BADARG;
    if (no_split) d.ksplit_ok = 0;
    return conv5x5_bf16_ksplit(d, (Operand)precision);
}
// ConvLSTM weight gradient with bf16 operands: dW (K-inner packed like the weight, [25][(cx+C)/32][4C][32]) += x|h^T . dG per tap.
// (one body behind the five entries; each keeps its own argument checks: what an entry refuses is part of its contract)
static int lstm_wgrad_packed_op(Operand operand, const float* x, int cx, int ldx, const float* h_prev, int C, const float* dG, float* dW, float* db, int B, int H,
                                int W, int tcount, long long ts_x, long long ts_h, long long ts_dG, int form, const float* dy_absmax, void* stream) {
    WgradDesc d;
    lstm_wgrad_op(d, x, cx, ldx, h_prev, C, dG, dW, db, B, H, W, tcount, ts_x, ts_h, ts_dG);
    d.form = form;
    if (dy_absmax) { d.dy_absmax = dy_absmax; d.dy_absmax_stride = 72; }
    return run_wgrad(d, (hipStream_t)stream, operand);
}
extern "C" int pivp_wgrad5x5_bf16(const float* x, int cx, int ldx, const float* h_prev, int C, const float* dG, float* dW, float* db,
                                  int B, int H, int W, void* stream) {
    if (!x || !dG || !dW || C <= 0 || cx <= 0) return PIVP_ERR_BADARG;
    return lstm_wgrad_packed_op(Operand::BF16, x, cx, ldx, h_prev, C, dG, dW, db, B, H, W, 1, 0, 0, 0, 0, nullptr, stream);
}
// ... with two fp16 pieces per operand and three MFMAs per product (fp32-grade; the fp16x3 mode's weight gradient), a batch of timesteps as below:
// scratch: 72 * tcount floats (the partial maxima of every timestep's dG: it is staged times a power of two from the largest of the batch)
extern "C" int pivp_wgrad5x5_fp16x3_batch(const float* x, int cx, int ldx, const float* h_prev, int C, const float* dG, float* dW, float* db,
                                          int B, int H, int W, int tcount, long long ts_x, long long ts_h, long long ts_dG, float* scratch, void* stream) {
    if (!x || !dG || !dW || !scratch || C <= 0 || cx <= 0 || tcount < 1 || B <= 0 || H <= 0 || W <= 0) return PIVP_ERR_BADARG;
    if (!form_serves_map(Operand::FP16X3, B, H, W)) return PIVP_ERR_BADARG;      // (in front of the partial maxima's launches)
    for (int j = 0; j < tcount; ++j) {
        const int rc = absmax_partials(reinterpret_cast<const float*>(reinterpret_cast<const char*>(dG) + j * ts_dG), (long)B * H * W * 4 * C,
                                       scratch + (size_t)j * 72, (hipStream_t)stream);
        if (rc != PIVP_OK) return rc;
    }
    return lstm_wgrad_packed_op(Operand::FP16X3, x, cx, ldx, h_prev, C, dG, dW, db, B, H, W, tcount, ts_x, ts_h, ts_dG, 0, scratch, stream);
}
// ... with three bf16 pieces per operand and six MFMAs per product (fp32-grade, fp32's exponent range; the bf16x6 mode's weight gradient)
extern "C" int pivp_wgrad5x5_bf16x6_batch(const float* x, int cx, int ldx, const float* h_prev, int C, const float* dG, float* dW, float* db,
                                          int B, int H, int W, int tcount, long long ts_x, long long ts_h, long long ts_dG, void* stream) {
    if (!x || !dG || !dW || C <= 0 || cx <= 0 || tcount < 1) return PIVP_ERR_BADARG;
    return lstm_wgrad_packed_op(Operand::BF16X6, x, cx, ldx, h_prev, C, dG, dW, db, B, H, W, tcount, ts_x, ts_h, ts_dG, 0, nullptr, stream);
}
// ... of a BATCH of timesteps in one launch (the sum over pixels runs over timesteps too): timestep j reads x + j * ts_x, h_prev + j * ts_h,
// dG + j * ts_dG (byte strides, multiples of 16, may be negative: the backward sweep walks time downwards)
extern "C" int pivp_wgrad5x5_bf16_batch(const float* x, int cx, int ldx, const float* h_prev, int C, const float* dG, float* dW, float* db,
                                        int B, int H, int W, int tcount, long long ts_x, long long ts_h, long long ts_dG, void* stream) {
    if (!x || !dG || !dW || C <= 0 || cx <= 0 || tcount < 1) return PIVP_ERR_BADARG;
    return lstm_wgrad_packed_op(Operand::BF16, x, cx, ldx, h_prev, C, dG, dW, db, B, H, W, tcount, ts_x, ts_h, ts_dG, 0, nullptr, stream);
}
// ... with the block form chosen by the caller: 1 = four-wave blocks (32 channels x 32 columns, about one per CU: they co-reside with the backward sweep's
// small kernels), 2 = eight-wave blocks (32 x 64: half the patch traffic per multiply-add), 0 = by size as pivp_wgrad5x5_bf16_batch does
extern "C" int pivp_wgrad5x5_bf16_batch_form(const float* x, int cx, int ldx, const float* h_prev, int C, const float* dG, float* dW, float* db,
                                             int B, int H, int W, int tcount, long long ts_x, long long ts_h, long long ts_dG, int form, void* stream) {
    if (!x || !dG || !dW || C <= 0 || cx <= 0 || tcount < 1 || form < 0 || form > 2) return PIVP_ERR_BADARG;
    return lstm_wgrad_packed_op(Operand::BF16, x, cx, ldx, h_prev, C, dG, dW, db, B, H, W, tcount, ts_x, ts_h, ts_dG, form, nullptr, stream);
}
static int convlstm_ln_cap(int H, int W, int C) {
    const int tiles = ((H * W + 31) / 32) * (C / 32), slices = ln_stats_slices(H * W * C);
    return tiles > slices ? tiles : slices;
}
extern "C" long long pivp_convlstm_ln_scratch_floats(int B, int H, int W, int C) {
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 32) return PIVP_ERR_BADARG;
    return (long long)B * convlstm_ln_cap(H, W, C) * 4;
}
extern "C" int pivp_convlstm_ln(const float* x, int cx, int ldx, const float* h_prev, int C, const float* w, const float* bias,
                                const float* c_in, float* c_out, float* h_out, const float* gamma, const float* beta,
                                float* ln_out, int ldo, float* partials, float eps, int B, int H, int W, int variant, int* fused,
                                void* stream) {
    if (!x || !w || !bias || !c_in || !c_out || !h_out || !gamma || !beta || !ln_out || !partials || variant < 0 || variant > 4)
        return PIVP_ERR_BADARG;
    if (C <= 0 || C % 32) return PIVP_ERR_BADARG;
    int np = 0;
    ConvLstmOpts o{};
    o.variant = variant; o.ln_out.part = partials; o.ln_out.cap = convlstm_ln_cap(H, W, C); o.ln_out.nparts = &np;
    int rc = run_convlstm(x, cx, ldx, h_prev, C, w, bias, c_in, c_out, h_out, B, H, W, (hipStream_t)stream, o);
    if (rc != PIVP_OK) return rc;
    if (fused) *fused = np > 0;
    LayerNormOpts lo{};
    lo.fused_nparts = np;
    return run_layernorm(h_out, gamma, beta, ln_out, partials, B, H * W * C, C, ldo, eps, 0, (hipStream_t)stream, lo);
}
extern "C" long long pivp_layernorm_backward_scratch_floats(int B, int n) {
    if (B <= 0 || n <= 0) return PIVP_ERR_BADARG;
    return (long long)B * ln_bwd_slices(n) * 2;
}
extern "C" int pivp_layernorm_backward(const float* dy, int lddy, const float* y, int ldy, const float* x, const float* stat,
                                       const float* gamma, float* partials, float* dx, float* dgamma, float* dbeta,
                                       int B, int n, int C, int relu, void* stream) {
    return ln_backward(dy, lddy, y, ldy, x, stat, gamma, partials, dx, dgamma, dbeta, B, n, C, relu, (hipStream_t)stream);
}
// LayerNorm backward of the norm behind a ConvLSTM + the cell's gate backward, the way the BPTT sweep runs the pair (plan_backward.hip:
// lnb_cell + lstmb): sums + parameter planes in one launch (ln_bwd_sums_params_kernel), then the gate kernel forms the norm's dx from the sums on the fly.
extern "C" long long pivp_gates_backward_ln_scratch_floats(int B, int n) {
    if (B <= 0 || n <= 0) return PIVP_ERR_BADARG;
    return (long long)B * ln_bwd_slices(n) * 2 + ln_bwd_param_part_floats(n);
}
extern "C" int pivp_gates_backward_ln(const float* gates, const float* c_old, const float* c_new, const float* dy, int lddy,
                                      const float* gamma, const float* stat, const float* h, const float* dh_b, int ldb, float* dc,
                                      int dc_valid, float* dG, float* dgamma, float* dbeta, float* scratch, int B, int npix, int C,
                                      void* stream) {
    if (!gates || !c_old || !c_new || !dy || !gamma || !stat || !h || !dc || !dG || !dgamma || !dbeta || !scratch) return PIVP_ERR_BADARG;
    if (B <= 0 || npix <= 0 || C <= 0 || C % 4 || lddy < C || lddy % 4) return PIVP_ERR_BADARG;
    hipStream_t s = (hipStream_t)stream;
    const int n = npix * C;
    float* partials = scratch;
    float* part = scratch + (size_t)B * ln_bwd_slices(n) * 2;
    if (hipMemsetAsync(part, 0, (size_t)ln_bwd_param_part_floats(n) * 4, s) != hipSuccess) return PIVP_ERR_LAUNCH;
    LnFuse lf;
    memset(&lf, 0, sizeof(lf));
    lf.dy = dy; lf.lddy = lddy; lf.gamma = gamma; lf.stat = stat; lf.h = h;
    lf.partials = partials; lf.S = ln_bwd_slices(n);
    int rc = ln_backward(dy, lddy, nullptr, 0, h, stat, gamma, partials, nullptr, dgamma, dbeta, B, n, C, 0, s, part);
    if (rc != PIVP_OK) return rc;
    rc = lstm_gates_bwd(gates, c_old, c_new, nullptr, 0, dh_b, ldb, dc, dc_valid, dG, B * npix, C, s, B, &lf);
    if (rc != PIVP_OK) return rc;
    return ln_bwd_params_reduce(part, dgamma, dbeta, B, n, s);
}
// Op entries of the head-side backward kernels (backward_heads.hip), one launcher each: what the BPTT sweep of plan_backward.hip calls, reachable one at a
// time (tests/test_gpu_backward_heads.py).  The SideFork of the sweep (a second stream for the weight gradients) is not exposed: everything on `stream`.
extern "C" int pivp_composite_backward_tiles(int H, int W) {
    if (H <= 0 || W <= 0) return PIVP_ERR_BADARG;
    return composite_bwd_tiles(H, W);
}
extern "C" int pivp_composite_backward(int model_type, const float* prev, const float* mask_logits, const float* layer0, const float* aux,
                                       const float* go, float* dmk, float* dz, float* part, float* dprev, int dprev_accum, int B, int H, int W,
                                       int num_masks, int stp_zero_border, unsigned long long* det_acc, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (model_type == PIVP_MODEL_CDNA) {
        if (det_acc) return PIVP_ERR_BADARG;
        return composite_bwd_cdna(prev, mask_logits, layer0, aux, go, dmk, dz, part, dprev, dprev_accum, B, H, W, num_masks, s);
    }
    if (model_type == PIVP_MODEL_STP) {
        if (dprev && !dprev_accum) return PIVP_ERR_BADARG;      // the scatter only ever adds into d prev
        return composite_bwd_stp(prev, mask_logits, layer0, aux, go, dmk, dz, part, dprev, B, H, W, num_masks, stp_zero_border, s, det_acc);
    }
    if (model_type == PIVP_MODEL_DNA) {
        if (det_acc || num_masks != 1) return PIVP_ERR_BADARG;
        return composite_bwd_dna(prev, mask_logits, aux, go, dmk, dz, dprev, dprev_accum, B, H, W, s);
    }
    return PIVP_ERR_BADARG;
}
extern "C" int pivp_mask_softmax_backward(const float* mask_logits, float* dmk, int B, int HW, int NP, void* stream) {
    return mask_softmax_bwd(mask_logits, dmk, B, HW, NP, (hipStream_t)stream);
}
extern "C" long long pivp_heads_backward_det_floats(int B, int HW, int NP, int NE) {
    if (B <= 0 || HW <= 0 || NP <= 0 || NE <= 0) return PIVP_ERR_BADARG;
    return heads_bwd_det_floats(B, HW, NP, NE);
}
extern "C" int pivp_heads_backward(const float* e6, const float* wm, const float* we, const float* dpm, const float* dpe, float* de6,
                                   float* dwm, float* dbm, float* dwe, float* dbe, int B, int HW, int NP, int NE, float* det_part,
                                   void* stream) {
    if (NP <= 0 || NE <= 0) return PIVP_ERR_BADARG;
    return heads_bwd(e6, wm, we, dpm, dpe, de6, dwm, dbm, dwe, dbe, B, HW, NP, NE, (hipStream_t)stream, det_part);
}
extern "C" int pivp_cdna_kernels_backward(const float* hidden5, const float* wt, const float* vpre, const float* dkpart, int ntiles, float* dv,
                                          float* dhidden5, int accum_dx, float* dwt, float* db, int B, int K, int num_masks, float* det_part,
                                          void* stream) {
    if (ntiles <= 0) return PIVP_ERR_BADARG;
    return cdna_kernels_bwd(hidden5, wt, vpre, dkpart, ntiles, dv, dhidden5, accum_dx, dwt, db, B, K, num_masks, (hipStream_t)stream, nullptr, det_part);
}
extern "C" int pivp_stp_params_backward(const float* hidden5, const float* wt1, const float* s1, const float* w2, const float* dthpart, int ntiles,
                                        float* dv, float* dhidden5, float* dwt1, float* db1, float* dw2, float* db2, int B, int K,
                                        float* det_part, void* stream) {
    if (ntiles <= 0) return PIVP_ERR_BADARG;
    return stp_params_bwd(hidden5, wt1, s1, w2, dthpart, ntiles, dv, dhidden5, dwt1, db1, dw2, db2, B, K, (hipStream_t)stream, det_part);
}
extern "C" long long pivp_enc3_state_backward_det_floats(int B, int HW8, int use_state) {
    if (B <= 0 || HW8 <= 0) return PIVP_ERR_BADARG;
    return enc3_state_bwd_det_floats(B, HW8, use_state);
}
extern "C" int pivp_enc3_state_backward(const float* e2, const float* e3, const float* de3, int ldd3, const float* action, const float* state,
                                        const float* w3, const float* wcs, const float* dsnew, float* de2, float* dw3, float* db3, float* dwcs,
                                        float* dbcs, float* dstate_prev, int B, int HW8, int use_state, int mask_e2, float* det_part,
                                        void* stream) {
    if (ldd3 < 64 || ldd3 % 4) return PIVP_ERR_BADARG;
    return enc3_state_bwd(e2, e3, de3, ldd3, action, state, w3, wcs, dsnew, de2, dw3, db3, dwcs, dbcs, dstate_prev, B, HW8, use_state,
                          (hipStream_t)stream, mask_e2, det_part);
}
extern "C" long long pivp_enc0_backward_det_floats(int B, int H, int W) {
    if (B <= 0 || H <= 1 || W <= 1) return PIVP_ERR_BADARG;
    return enc0_bwd_det_floats(B, H, W);
}
extern "C" int pivp_enc0_backward(const float* img, const float* w, const float* d, float* dw, float* db, float* dimg, int dimg_accum,
                                  int B, int H, int W, float* det_part, void* stream) {
    if (H <= 1 || W <= 1) return PIVP_ERR_BADARG;
    return enc0_bwd(img, w, d, dw, db, dimg, dimg_accum, B, H, W, (hipStream_t)stream, nullptr, det_part);
}
extern "C" int pivp_adam_step(float* p, const float* g, float* m, float* v, long long n, double lr_t, double beta1, double beta2,
                              double eps, double gscale, void* stream) {
    return adam_step(p, g, m, v, (long)n, lr_t, beta1, beta2, eps, gscale, (hipStream_t)stream);
}
extern "C" int pivp_grad_pack_bf16(const float* src, void* dst_bf16, long long n, void* stream) {
    return grad_pack_bf16(src, dst_bf16, (long)n, (hipStream_t)stream);
}
extern "C" int pivp_grad_sum_shards(const void* src, int src_bf16, int nshards, long long shard_len, void* dst, int dst_bf16, void* stream) {
    return grad_sum_shards(src, src_bf16, nshards, (long)shard_len, dst, dst_bf16, (hipStream_t)stream);
}
extern "C" int pivp_grad_unpack_bf16(const void* src_bf16, float* dst, long long n, void* stream) {
    return grad_unpack_bf16(src_bf16, dst, (long)n, (hipStream_t)stream);
}
extern "C" int pivp_conv3x3s2(const float* x, int cin, int ldx, const float* w, const float* bias, float* out, int cout,
                              int ldo, int relu, int B, int Hin, int Win, void* stream) {
    if (!x || !w || !out) return PIVP_ERR_BADARG;
    return run_conv3x3s2(x, cin, ldx, w, bias, out, cout, ldo, relu, B, Hin, Win, (hipStream_t)stream, 0);
}
extern "C" int pivp_deconv3x3s2(const float* x, int cin, int ldx, const float* w, const float* bias, float* out, int cout,
                                int ldo, int relu, int B, int Hin, int Win, void* stream) {
    if (!x || !w || !out) return PIVP_ERR_BADARG;
    return run_deconv3x3s2(x, cin, ldx, w, bias, out, cout, ldo, relu, B, Hin, Win, (hipStream_t)stream);
}
// deconv3x3s2 of concat(LayerNorm(h_raw), x1) in ONE conv launch (the norm applied while the tile kernel stages its patch): what inference
// rollouts run for enc5 / enc6.  The statistics are taken here by ln_stats into `partials` (pivp_layernorm_scratch_floats(B, Hin*Win*c_ln));
// in the rollout they come from the ConvLSTM's epilogue.  precision: 0 fp32, 1 bf16 operands, 2 split.  PIVP_ERR_BADARG for geometries
// the tile kernel does not take (pivp_deconv3x3s2_ln_fits).
extern "C" int pivp_deconv3x3s2_ln_fits(int c_ln, int c1, int cout, int B, int Hin, int Win) {
    return deconv3x3s2_ln_ok(c_ln, c1, cout, B, Hin, Win) ? 1 : 0;
}
extern "C" int pivp_deconv3x3s2_ln(const float* h_raw, int c_ln, const float* x1, int c1, int ld1, const float* w, const float* bias,
                                   const float* gamma, const float* beta, float eps, float* partials, float* out, int cout, int ldo, int relu,
                                   int B, int Hin, int Win, int precision, void* stream) {
    if (!h_raw || !w || !out || !gamma || !beta || !partials || precision < 0 || precision > 2) return PIVP_ERR_BADARG;
    if (!deconv3x3s2_ln_ok(c_ln, x1 ? c1 : 0, cout, B, Hin, Win)) return PIVP_ERR_BADARG;
    const int n = Hin * Win * c_ln;
    int rc = ln_stats(h_raw, partials, B, n, (hipStream_t)stream);
    if (rc != PIVP_OK) return rc;
    const LnIn ln{gamma, beta, partials, ln_stats_slices(n), eps};
    static const Operand form_of[3] = {Operand::F32, Operand::BF16, Operand::BF16X3};      // this entry's precision codes
    DeconvLnOpts o{};
    o.x1 = x1; o.c1 = c1; o.ld1 = ld1; o.operand = form_of[precision];
    return run_deconv3x3s2_ln(h_raw, c_ln, w, bias, out, cout, ldo, relu, B, Hin, Win, (hipStream_t)stream, ln, o);
}
// bf16-operand form (precision mode bf16): x and w rounded to bf16 on the way into LDS, fp32 accumulation / bias / ReLU.  Only maps that the
// all-parities tile kernel takes (Hin % 8 == 0, Win % 16 == 0, at least 16 blocks) run in bf16; others fall to the fp32 kernels.
extern "C" int pivp_deconv3x3s2_bf16(const float* x, int cin, int ldx, const float* w, const float* bias, float* out, int cout,
                                     int ldo, int relu, int B, int Hin, int Win, void* stream) {
    if (!x || !w || !out) return PIVP_ERR_BADARG;
    DeconvOpts o{};
    o.operand = Operand::BF16;
    return run_deconv3x3s2(x, cin, ldx, w, bias, out, cout, ldo, relu, B, Hin, Win, (hipStream_t)stream, o);
}
extern "C" int pivp_deconv3x3s2_bf16x3(const float* x, int cin, int ldx, const float* w, const float* bias, float* out, int cout,
                                       int ldo, int relu, int B, int Hin, int Win, void* stream) {   // split mode: two bf16 pieces per operand
    if (!x || !w || !out) return PIVP_ERR_BADARG;
    DeconvOpts o{};
    o.operand = Operand::BF16X3;
    return run_deconv3x3s2(x, cin, ldx, w, bias, out, cout, ldo, relu, B, Hin, Win, (hipStream_t)stream, o);
}
// two fp16 pieces per operand, three MFMAs per product (precision mode PIVP_PRECISION_FP16X3): scratch = 66 floats (the weights' partial maxima)
extern "C" int pivp_deconv3x3s2_fp16x3(const float* x, int cin, int ldx, const float* w, const float* bias, float* out, int cout,
                                       int ldo, int relu, int B, int Hin, int Win, float* scratch, void* stream) {
    if (!x || !w || !out || !scratch || cin <= 0 || cout <= 0) return PIVP_ERR_BADARG;
    int rc = absmax_partials(w, 9L * cin * cout, scratch, (hipStream_t)stream);
    if (rc != PIVP_OK) return rc;
    DeconvOpts o{};
    o.operand = Operand::FP16X3; o.wscale_part = scratch;
    return run_deconv3x3s2(x, cin, ldx, w, bias, out, cout, ldo, relu, B, Hin, Win, (hipStream_t)stream, o);
}
extern "C" int pivp_conv_enc0(const float* img, const float* w, const float* bias, float* out, int B, int H, int W, void* stream) {
    return conv_enc0(img, w, bias, out, B, H, W, (hipStream_t)stream);
}
// ---- include/pivp_conv_forms.h: the launch forms of the plain convolutions as host-only queries, and op entries for what a rollout reaches mid-step ----
static_assert((int)ConvForm::DeconvTile == PIVP_CONV_FORM_DECONV_TILE && (int)ConvForm::LongKDgrad == PIVP_CONV_FORM_LONG_K_DGRAD &&
              (int)ConvForm::Small1 == PIVP_CONV_FORM_SMALL_1 && (int)ConvForm::Small2 == PIVP_CONV_FORM_SMALL_2 && (int)ConvForm::Small3 == PIVP_CONV_FORM_SMALL_3 &&
              (int)ConvForm::F32_128x32 == PIVP_CONV_FORM_F32_128X32 && (int)ConvForm::F32_128x64 == PIVP_CONV_FORM_F32_128X64 &&
              (int)ConvForm::F32_128x96 == PIVP_CONV_FORM_F32_128X96 && (int)ConvForm::F32_128x128 == PIVP_CONV_FORM_F32_128X128 &&
              (int)ConvForm::F32_64x64 == PIVP_CONV_FORM_F32_64X64 && (int)ConvForm::F32_64x128 == PIVP_CONV_FORM_F32_64X128 &&
              (int)ConvForm::F32_32x128 == PIVP_CONV_FORM_F32_32X128 && (int)Enc0Form::Rows == PIVP_ENC0_FORM_ROWS && (int)Enc0Form::Generic == PIVP_ENC0_FORM_GENERIC,
              "conv_form.h and include/pivp_conv_forms.h disagree on a form's code");
extern "C" int pivp_conv_form(int deconv, int cin, int cout, int B, int Hin, int Win, int aligned) {
    if (deconv < 0 || deconv > 1 || cin <= 0 || cin % 32 || cout <= 0 || cout % 32 || B <= 0 || Hin <= 0 || Win <= 0) return PIVP_ERR_BADARG;
    if (!deconv && (Hin % 2 || Win % 2)) return PIVP_ERR_BADARG;
    if (!fits31(view_bytes(B, Hin, Win, cin)) || !fits31(9LL * cin * cout * 4)) return PIVP_ERR_BADARG;
    // (the ops' descriptors never qualify as long-K data gradients: run_conv3x3s2 / run_deconv3x3s2 allow no K split)
    return (int)conv_form(deconv, cin, cout, B, Hin, Win, aligned ? 1 : 0, 0);
}
extern "C" int pivp_conv_enc0_form(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0 || H % 2 || W % 2) return PIVP_ERR_BADARG;
    return (int)enc0_form(B, H, W, 1);
}
extern "C" int pivp_conv3x3s2_ln_fits(int cin, int cout, int B, int Hin, int Win) {
    if (cin <= 0 || cout <= 0 || B <= 0 || Hin <= 0 || Win <= 0) return 0;
    return conv3x3s2_ln_ok(cin, cout, B, Hin, Win) ? 1 : 0;
}
extern "C" int pivp_conv3x3s2_ln(const float* x_raw, int cin, const float* w, const float* bias, const float* gamma, const float* beta, float eps,
                                 float* partials, float* out, int cout, int ldo, int relu, float* keep_out, int keep_ld, float* stat_out,
                                 const pivp_enc3_epilogue_t* ep, int B, int Hin, int Win, void* stream) {
    if (!x_raw || !w || !gamma || !beta || !partials || !out || !pivp_conv3x3s2_ln_fits(cin, cout, B, Hin, Win)) return PIVP_ERR_BADARG;
    // everything run_conv3x3s2_ln and igemm_small refuse is refused here, in front of the statistics pass
    if (ldo < cout || ldo % 4 || ((uintptr_t)out & 15) || (bias && ((uintptr_t)bias & 15))) return PIVP_ERR_BADARG;
    if (keep_out && (keep_ld < cin || keep_ld % 4 || ((uintptr_t)keep_out & 15) || !fits31((long long)B * Hin * Win * keep_ld))) return PIVP_ERR_BADARG;
    Enc3Fuse f3;
    memset(&f3, 0, sizeof(f3));
    if (ep) {
        if (!ep->w3 || !ep->b3 || !ep->action || !ep->state || !ep->e3_out || (ep->state_out && (!ep->wcs || !ep->bcs))) return PIVP_ERR_BADARG;
        if (cout != 64 || ldo != 64 || !relu || !bias || keep_out) return PIVP_ERR_BADARG;
        f3.w3 = ep->w3; f3.b3 = ep->b3; f3.action = ep->action; f3.state = ep->state; f3.wcs = ep->wcs; f3.bcs = ep->bcs;
        f3.e3 = ep->e3_out; f3.state_out = ep->state_out; f3.use_state = ep->use_state;
    }
    const int n = Hin * Win * cin;
    int rc = ln_stats(x_raw, partials, B, n, (hipStream_t)stream);
    if (rc != PIVP_OK) return rc;
    const LnIn ln{gamma, beta, partials, ln_stats_slices(n), eps};
    Conv3x3LnOpts o{};
    if (ep) o.fuse3 = &f3;
    o.keep = NormKeep{keep_out, keep_ld, stat_out};
    return run_conv3x3s2_ln(x_raw, cin, w, bias, out, cout, ldo, relu, B, Hin, Win, (hipStream_t)stream, ln, o);
}
// the partial slots per sample pivp_conv_layernorm offers the producer: what any of its forms may write, and the separate pass's slices
static int conv_ln_cap(int kind, int cout, int Hin, int Win) {
    const bool up = kind == PIVP_CONV_KIND_DECONV3X3S2;
    const int Hout = up ? 2 * Hin : Hin / 2, Wout = up ? 2 * Win : Win / 2;
    const int tiles = kind == PIVP_CONV_KIND_ENC0 ? (Hout * Wout + 63) / 64 : ((up ? Hin * Win : Hout * Wout) + 31) / 32 * (cout / 32) * (up ? 4 : 1);
    const int slices = ln_stats_slices(Hout * Wout * cout);
    return tiles > slices ? tiles : slices;
}
static bool conv_ln_args_ok(int kind, int cout, int B, int Hin, int Win) {
    if (kind < PIVP_CONV_KIND_ENC0 || kind > PIVP_CONV_KIND_DECONV3X3S2 || cout <= 0 || cout % 32 || B <= 0 || Hin <= 0 || Win <= 0) return false;
    if (kind != PIVP_CONV_KIND_DECONV3X3S2 && (Hin % 2 || Win % 2)) return false;
    const bool up = kind == PIVP_CONV_KIND_DECONV3X3S2;
    const long long n = (long long)(up ? 2 * Hin : Hin / 2) * (up ? 2 * Win : Win / 2) * cout;      // the output, per sample
    return (kind != PIVP_CONV_KIND_ENC0 || cout == 32) && fits31(n * B * 4);
}
extern "C" long long pivp_conv_layernorm_scratch_floats(int kind, int cout, int B, int Hin, int Win) {
    if (!conv_ln_args_ok(kind, cout, B, Hin, Win)) return PIVP_ERR_BADARG;
    return (long long)B * conv_ln_cap(kind, cout, Hin, Win) * 4;
}
extern "C" int pivp_conv_layernorm(int kind, const float* x, int cin, int ldx, const float* w, const float* bias, float* raw_out, int cout, int relu,
                                   const float* gamma, const float* beta, float* ln_out, int ldo, float* partials, float eps, int relu_ln,
                                   int B, int Hin, int Win, int* fused, void* stream) {
    if (fused) *fused = 0;
    if (!x || !w || !raw_out || !gamma || !beta || !ln_out || !partials || !conv_ln_args_ok(kind, cout, B, Hin, Win)) return PIVP_ERR_BADARG;
    if (ldo < cout || ldo % 4) return PIVP_ERR_BADARG;
    if (kind == PIVP_CONV_KIND_ENC0 && (cin != 3 || relu || !bias)) return PIVP_ERR_BADARG;
    hipStream_t s = (hipStream_t)stream;
    const bool up = kind == PIVP_CONV_KIND_DECONV3X3S2;
    const int Hout = up ? 2 * Hin : Hin / 2, Wout = up ? 2 * Win : Win / 2;
    const int cap = conv_ln_cap(kind, cout, Hin, Win);
    int np = 0, rc = PIVP_ERR_BADARG;
    if (kind == PIVP_CONV_KIND_ENC0) {
        rc = conv_enc0(x, w, bias, raw_out, B, Hin, Win, s, partials, cap, &np);
    } else if (kind == PIVP_CONV_KIND_CONV3X3S2) {
        IgemmDesc d;
        rc = conv3x3s2_desc(d, x, cin, ldx, w, bias, raw_out, cout, cout, relu, B, Hin, Win, 0);
        if (rc != PIVP_OK) return rc;
        d.ln_part = partials; d.ln_cap = cap;
        rc = igemm_conv(d, s, &np);
    } else {
        DeconvOpts o{};
        o.ln_out.part = partials; o.ln_out.cap = cap; o.ln_out.nparts = &np;
        rc = run_deconv3x3s2(x, cin, ldx, w, bias, raw_out, cout, cout, relu, B, Hin, Win, s, o);
    }
    if (rc != PIVP_OK) return rc;
    if (fused) *fused = np;
    LayerNormOpts lo{};
    lo.fused_nparts = np;      // (as Rollout::ln: 0 = the statistics pass first)
    return run_layernorm(raw_out, gamma, beta, ln_out, partials, B, Hout * Wout * cout, cout, ldo, eps, relu_ln, s, lo);
}
extern "C" long long pivp_layernorm_scratch_floats(int B, int n) {
    if (B <= 0 || n <= 0) return PIVP_ERR_BADARG;
    return (long long)B * ln_stats_slices(n) * 4;
}
extern "C" int pivp_layernorm(const float* x, const float* gamma, const float* beta, float* out, float* partials,
                              int B, int n, int C, int ldo, float eps, int relu, void* stream) {
    return run_layernorm(x, gamma, beta, out, partials, B, n, C, ldo, eps, relu, (hipStream_t)stream);
}
extern "C" int pivp_enc3_state(const float* e2, const float* action, const float* state, const float* w3, const float* b3,
                               const float* wcs, const float* bcs, float* e3, float* state_out, int B, int HW8, int use_state,
                               void* stream) {
    return enc3_state(e2, action, state, w3, b3, wcs, bcs, e3, state_out, B, HW8, use_state, (hipStream_t)stream);
}
extern "C" int pivp_heads(const float* e6, const float* wm, const float* bm, const float* we, const float* be,
                          float* mask_logits, float* enc7, float* layer0, int B, int HW, int num_masks, int model_type,
                          void* stream) {
    if (model_type < 0 || model_type > 2) return PIVP_ERR_BADARG;
    return heads_1x1(e6, wm, bm, we, be, mask_logits, enc7, layer0, B, HW, num_masks + 1,
                     model_type == PIVP_MODEL_DNA ? 25 : 3, model_type, (hipStream_t)stream);
}
extern "C" long long pivp_linear_scratch_floats(int B, int K) {
    if (B <= 0 || K <= 0) return PIVP_ERR_BADARG;
    return motion_partials_floats(B, K);      // [B][K slices][256] + the tail pivp_frame_head's finisher may read (never summed)
}
extern "C" int pivp_cdna_kernels(const float* hidden5, const float* wt, const float* bias, float* partials, float* kerns,
                                 int B, int K, int num_masks, void* stream) {
    return cdna_kernels(hidden5, wt, bias, partials, kerns, B, K, num_masks, (hipStream_t)stream);
}
extern "C" int pivp_stp_params(const float* hidden5, const float* wt1, const float* b1, const float* w2, const float* b2,
                               float* partials, float* theta, int B, int K, void* stream) {
    return stp_params(hidden5, wt1, b1, w2, b2, partials, theta, B, K, (hipStream_t)stream);
}
extern "C" int pivp_frame_head_fits(int model_type, int B, int H, int W, int num_masks, int K) {
    if (!frame_head_ok(model_type, B, H, W, num_masks)) return 0;
    return (model_type == PIVP_MODEL_DNA || frame_head_finishes(K)) ? 1 : 2;
}
extern "C" int pivp_motion_partials(const float* hidden5, const float* wt, float* partials, int B, int K, int fp64_accumulate, void* stream) {
    return motion_partials(hidden5, wt, partials, B, K, fp64_accumulate, (hipStream_t)stream);
}
extern "C" int pivp_frame_head(const pivp_frame_head_args_t* g, void* stream) {
    if (!g) return PIVP_ERR_BADARG;
    FrameHeadArgs a;
    a.e6raw = g->e6raw; a.ln_part = g->ln_part; a.ln_nparts = g->ln_nparts; a.gamma = g->gamma; a.beta = g->beta; a.eps = g->ln_eps;
    a.wm = g->masks_w; a.bm = g->masks_b; a.we = g->enc7_w; a.be = g->enc7_b; a.prev = g->prev;
    a.partials = g->partials; a.KS = g->kslices; a.hbias = g->head_bias; a.w2 = g->w2; a.b2 = g->b2; a.aux = g->aux;
    a.out = g->out; a.masks_out = g->masks_out; a.enc7 = g->enc7;
    a.logits_out = g->logits_out; a.layer0_out = g->layer0_out; a.y_out = g->enc6_out; a.stat_out = g->stat_out;
    a.kerns_out = g->kerns_out; a.vpre_out = g->vpre_out;
    a.B = g->B; a.H = g->H; a.W = g->W; a.NM = g->num_masks; a.stp_zero = g->stp_zero_border;
    return frame_head(a, g->model_type, (hipStream_t)stream);
}
extern "C" int pivp_composite(const float* prev, const float* mask_logits, const float* layer0, const float* aux, float* out,
                              float* masks_out, int B, int H, int W, int num_masks, int model_type, int stp_zero_border,
                              void* stream) {
    return composite(prev, mask_logits, layer0, aux, out, masks_out, B, H, W, num_masks, model_type, stp_zero_border,
                     (hipStream_t)stream);
}
extern "C" int pivp_pixel_track(const float* planes_in, const float* masks, const float* aux, float* planes_out,
                                int B, int P, int H, int W, int num_masks, int model_type, int stp_zero_border, void* stream) {
    return pixel_track(planes_in, masks, aux, planes_out, B, P, H, W, num_masks, model_type, stp_zero_border, (hipStream_t)stream);
}
extern "C" int pivp_plan_cost(const float* track, const float* goals, const float* step_w, const float* plane_w, float miss_cost, float* cost,
                              float* mass, float* edist, int S, int K, int P, int H, int W, void* stream) {
    return plan_cost(track, goals, step_w, plane_w, miss_cost, cost, mass, edist, S, K, P, H, W, (hipStream_t)stream);
}
extern "C" int pivp_cem_update(const float* cost, float* actions, float* mean, float* std, float* best_actions, float* best_cost,
                               const float* low, const float* high, int* elite_idx, int K, int steps, int t0, int elites, float alpha,
                               float min_std, unsigned long long seed, int iteration, void* stream) {
    return cem_update(cost, actions, mean, std, best_actions, best_cost, low, high, elite_idx, K, steps, t0, elites, alpha, min_std, seed, iteration,
                      (hipStream_t)stream);
}
extern "C" int pivp_frame_metrics(const float* pred, const float* truth, int N, int C, int H, int W, int win, float sigma, float data_range,
                                  float* mse, float* ssim, void* stream) {
    return frame_metrics(pred, truth, N, C, H, W, win, sigma, data_range, mse, ssim, (hipStream_t)stream);
}
extern "C" int pivp_gather_batch(const void* frames, int frames_u8, const float* actions, const float* states, const int* index, int B,
                                 long long N, int T, int H, int W, float* out_images, float* out_actions, float* out_states, void* stream) {
    return gather_batch(frames, frames_u8, actions, states, index, B, N, T, H, W, out_images, out_actions, out_states, (hipStream_t)stream);
}
extern "C" int pivp_resize_images(const float* in, float* out, int planes, int Hin, int Win, int Hout, int Wout, float scale, void* stream) {
    return resize_bilinear(in, out, planes, Hin, Win, Hout, Wout, scale, (hipStream_t)stream);
}
extern "C" int pivp_select_frames(const float* ground_truth, const float* generated, const unsigned char* take_gt, float* out,
                                  int B, int frame_numel, void* stream) {
    if (!ground_truth || !generated || !take_gt || !out || B <= 0 || frame_numel <= 0 || frame_numel % 4) return PIVP_ERR_BADARG;
    return run_select_frames(ground_truth, generated, take_gt, out, B, frame_numel, (hipStream_t)stream);
}
