/* The launch forms of the plain convolutions (enc0, the 3x3 stride-2 convs enc1 / enc2, the transposed convs enc4 / enc5 / enc6), and op entries
 * for the pieces of them a rollout reaches only in the middle of a step: beside the model's C ABI of pivp_hip.h (same conventions: int status
 * PIVP_OK / PIVP_ERR_*, PIVP_ERR_BADARG with nothing launched, caller-owned device memory, stream-ordered, no synchronisation, no allocation).
 * tests/test_gpu_conv_forms.py holds every form to the float64 oracle.  Bound by `_lib.CONV_FORMS_SIGNATURES`; the ABI version of pivp_hip.h covers
 * this header too. */
#ifndef PIVP_CONV_FORMS_H
#define PIVP_CONV_FORMS_H

#include "pivp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* pivp_conv3x3s2 / pivp_deconv3x3s2 do not run one kernel each: the launcher picks a form from the batch and the map size. */
#define PIVP_CONV_FORM_DECONV_TILE 1      /* transposed conv, all four output parities per block: maps of 8 x 16 input patches, >= 16 blocks */
#define PIVP_CONV_FORM_LONG_K_DGRAD 2     /* a long-K data gradient (tile and K split by a cost model): never the answer of pivp_conv_form */
#define PIVP_CONV_FORM_SMALL_1 11         /* 32-anchor tiles with K split over the block's waves, one 32-column tile per block ... */
#define PIVP_CONV_FORM_SMALL_2 12         /* ... two ... */
#define PIVP_CONV_FORM_SMALL_3 13         /* ... three */
#define PIVP_CONV_FORM_F32_128X32 21      /* the main implicit-GEMM kernel's block tiles, anchors x columns (long K, or out / bias not 16-byte aligned) */
#define PIVP_CONV_FORM_F32_128X64 22
#define PIVP_CONV_FORM_F32_128X96 23
#define PIVP_CONV_FORM_F32_128X128 24
#define PIVP_CONV_FORM_F32_64X64 25
#define PIVP_CONV_FORM_F32_64X128 26
#define PIVP_CONV_FORM_F32_32X128 27
/* host only: the form that pivp_hip.h's 3x3 stride-2 conv (deconv = 0) or its transposed conv (deconv = 1) launches for cin -> cout channels (multiples of 32) on a
 * B x Hin x Win input.  aligned: ldo % 4 == 0 and out and bias 16-byte aligned (0: the forms 21 .. 27 serve what 11 .. 13 cannot).
 * pivp_conv3x3s2_ln below launches the LayerNorm-on-load variant of the SMALL_n form this returns with aligned = 1.  PIVP_ERR_BADARG for
 * sizes the ops refuse. */
int pivp_conv_form(int deconv, int cin, int cout, int B, int Hin, int Win, int aligned);

#define PIVP_ENC0_FORM_ROWS 1             /* a block owns whole output rows (64 pixels): W/2 in {8, 16, 32}, H/2 a multiple of 64 / (W/2) */
#define PIVP_ENC0_FORM_GENERIC 2          /* one output pixel per four threads: every other frame */
/* host only: the kernel pivp_conv_enc0 launches on B x 3 x H x W frames (16-byte aligned weights).  Only ROWS reports LayerNorm partials. */
int pivp_conv_enc0_form(int B, int H, int W);

/* The 1x1 conv enc3 on (enc2, action, state) and the state predictor (pivp_enc3_state's operands) as the epilogue of the conv that produces enc2. */
typedef struct pivp_enc3_epilogue {
    const float* w3; const float* b3; const float* action; const float* state; const float* wcs; const float* bcs;
    float* e3_out;          /* [B][Hin/2 * Win/2][64] */
    float* state_out;       /* [B][5], may be NULL */
    int use_state;
} pivp_enc3_epilogue_t;

/* conv3x3s2(LayerNormalizationConv2D(x_raw)) + optional ReLU in ONE conv launch, the norm applied while the conv stages its input (enc1 / enc2 behind
 * hidden2 / hidden4, TM:560-563): bit-identical to pivp_layernorm + pivp_conv3x3s2.  x_raw [B][Hin*Win][cin] contiguous, gamma / beta [Hin*Win][cin],
 * partials: scratch of pivp_layernorm_scratch_floats floats for (B, Hin*Win*cin) (the statistics are taken here by the separate pass; in a rollout they
 * come from the ConvLSTM's epilogue).  Optional, NULL to leave out:
 *   keep_out (pixel stride keep_ld >= cin, 16-byte aligned) receives the normalised input, bit for bit pivp_layernorm's output, and stat_out [B][2]
 *       the samples' (mean, rstd): what a training plan keeps for the backward sweep;
 *   ep: enc3 and the state predictor in the epilogue, bit-identical to pivp_enc3_state on `out`.  Needs cout == 64, ldo == 64, relu, a bias, and no keep_out.
 * Only for geometries pivp_conv3x3s2_ln_fits accepts: cin and cout multiples of 32, even Hin and Win, (Hin/2 * Win/2) % 32 == 0. */
int pivp_conv3x3s2_ln_fits(int cin, int cout, int B, int Hin, int Win);
int pivp_conv3x3s2_ln(const float* x_raw, int cin, const float* w, const float* bias, const float* gamma, const float* beta, float eps,
                      float* partials, float* out, int cout, int ldo, int relu, float* keep_out, int keep_ld, float* stat_out,
                      const pivp_enc3_epilogue_t* ep, int B, int Hin, int Win, void* stream);

#define PIVP_CONV_KIND_ENC0 0             /* x: frames [B][3][H][W], cin = 3, cout = 32, no ReLU; Hin x Win = the frame */
#define PIVP_CONV_KIND_CONV3X3S2 1
#define PIVP_CONV_KIND_DECONV3X3S2 2
/* norm(conv(x)): the producer `kind` with the LayerNorm partials of its output requested from its epilogue, then the LayerNormalizationConv2D that
 * follows it (+ optional ReLU, relu_ln) from those partials, as a rollout runs norm_enc0 and norm_enc6 (TM:595, 601): the plain-conv counterpart of
 * pivp_convlstm_ln.  x / cin / ldx / w / bias / cout / relu as the producer's own entry takes them; raw_out [B][Hout*Wout][cout] contiguous receives
 * the conv's output, ln_out (pixel stride ldo) its norm; gamma / beta [Hout*Wout][cout]; partials: scratch of
 * pivp_conv_layernorm_scratch_floats floats.  *fused (optional) receives the number of partials per sample the producer's epilogue wrote; 0: its
 * tiles straddle samples (or the form writes none) and the separate statistics pass ran -- same result either way. */
long long pivp_conv_layernorm_scratch_floats(int kind, int cout, int B, int Hin, int Win);
int pivp_conv_layernorm(int kind, const float* x, int cin, int ldx, const float* w, const float* bias, float* raw_out, int cout, int relu,
                        const float* gamma, const float* beta, float* ln_out, int ldo, float* partials, float eps, int relu_ln,
                        int B, int Hin, int Win, int* fused, void* stream);

#ifdef __cplusplus
}
#endif
#endif
