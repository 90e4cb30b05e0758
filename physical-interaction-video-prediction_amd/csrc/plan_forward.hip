// The plan's forward side (plan.h): one timestep of the op program, and the two rollouts that sequence it.
#include "plan.h"

using namespace pivp;

// ------------------------------------------------------------------------------------------------------------
// forward, one timestep (TM:659-731)
// ------------------------------------------------------------------------------------------------------------
static int run_step(pivp_plan* p, int t, const float* prev, const float* action, const float* state_prev,
                    float* gen_out, float* state_out, hipStream_t s) {
    const pivp_config_t& c = p->cfg;
    const int B = c.batch, H = c.height, W = c.width;
    float* ws = p->ws;
    const Slab& S = p->slabs[t % p->nslabs];
    const Slab* Sp = t > 0 ? &p->slabs[(t - 1) % p->nslabs] : nullptr;
    float* lnp = ws + p->o_lnpart;
    const float eps = c.ln_eps;
    const bool train = c.keep_activations != 0;
    // t = 0: h == 0, skipped, and c from the zero buffer -- unless the rollout starts from a registered state (pivp_plan_set_rollout_state): then the
    // ordinary two-operand launch on the caller's (c, h)
    const float* const sin = t == 0 ? p->state_in : nullptr;
    auto hp = [&](int i) -> const float* { return Sp ? ws + Sp->h[i] : sin ? sin + state_seg_offset(c, 2 * i + 1) : nullptr; };
    auto cp = [&](int i) -> const float* { return Sp ? ws + Sp->c[i] : sin ? sin + state_seg_offset(c, 2 * i) : ws + p->o_zero; };
    const int ln_cap = ln_partial_cap(H * W);   // partial slots per sample in lnp (see the workspace carve)
    int np = 0;
    const Modes& md = p->mode;
    // cell i on x; ln_in: x is the raw output of the cell in front, normalised while staged -- the partials of this cell's own output then go to part_out
    auto lstm = [&](int i, const float* x, int ldx, const LnIn* ln_in = nullptr, float* part_out = nullptr) {
        const bool prof = p->prof_on && p->prof_used + 2 <= p->prof_ev.size();
        if (prof) (void)hipEventRecord(p->prof_ev[p->prof_used], s);
        const MapSize m = lstm_map(c, i);
        ConvLstmOpts o{};
        if (train) o.gates_out = ws + S.gates[i];
        // the LayerNorm behind every ConvLSTM gets its statistics from the ConvLSTM epilogue (np partials per sample)
        o.ln_out.part = part_out ? part_out : lnp; o.ln_out.cap = ln_cap; o.ln_out.nparts = &np;
        if (md.packs()) { o.w_bf16 = reinterpret_cast<const unsigned short*>(ws + p->o_wbf16[i]); o.operand = md.precision; }
        o.ln_in = ln_in;
        int rc = run_convlstm(x, kLstm[i].cx, ldx, hp(i), kLstm[i].C, P(p, p->i_lstm_w[i]), P(p, p->i_lstm_b[i]),
                              cp(i), ws + S.c[i], ws + S.h[i], B, m.H, m.W, s, o);
        if (prof) {
            (void)hipEventRecord(p->prof_ev[p->prof_used + 1], s);
            p->prof_layer[p->prof_used / 2] = i + (hp(i) ? 0 : 8);   // +8: first-step launch without the h half of K
            p->prof_used += 2;
        }
        return rc;
    };
    auto ln = [&](int j, const float* x, float* out, int n, int C, int ldo, int relu, int fused_nparts) {
        LayerNormOpts o{};
        o.stat_out = ws + S.lnstat + (size_t)j * B * 2; o.fused_nparts = fused_nparts;
        return run_layernorm(x, P(p, p->i_ln_g[j]), P(p, p->i_ln_b[j]), out, lnp, B, n, C, ldo, eps, relu, s, o);
    };
    auto norm_in = [&](int j) { return LnIn{P(p, p->i_ln_g[j]), P(p, p->i_ln_b[j]), lnp, np, eps}; };      // norm j applied by its consumer, from the current partials
    auto keep = [&](int j, float* out, int ld) { return NormKeep{out, ld, ws + S.lnstat + (size_t)j * B * 2}; };      // ... which a training plan has it write
    const int n2 = 32 * p->H2 * p->W2, n4 = 64 * p->H4 * p->W4, n8 = 128 * p->H8 * p->W8;

    // group 0 (TM:595): enc0 -> norm_enc0 -> relu   => cat7[:, 32:64]
    RC(conv_enc0(prev, P(p, p->i_enc_w[0]), P(p, p->i_enc_b[0]), ws + S.e0raw, B, H, W, s, lnp, ln_cap, &np));
    RC(ln(0, ws + S.e0raw, ws + S.cat7 + 32, n2, 32, 64, 1, np));
    // group 1 (TM:596): lstm1 -> hidden1 -> lstm2 -> hidden2 -> enc1 -> relu  => cat6[:, 64:96]
    RC(lstm(0, ws + S.cat7 + 32, 64));
    // Inference rollouts in the L2-direct modes: hidden1 / hidden3 feed only lstm2 / lstm4, whose eight-wave kernels apply the norm while
    // they stage their patch (the partials of their own output go to the second buffer: their blocks finish while others still read the input's).
    float* const lnpA = ws + p->o_lnpart, * const lnpB = ws + p->o_lnpart2;
    auto other = [&](float* q) { return q == lnpA ? lnpB : lnpA; };
    const bool fold_l2 = !train && np > 0 && convlstm_ln_in_ok(md.precision, 32, 32, 32, B, p->H2, p->W2) &&
                         (long)B * (p->H2 / 8) * (p->W2 / 16) >= 128;
    if (fold_l2) {
        const LnIn li = norm_in(1);
        float* q = other(lnp);
        RC(lstm(1, ws + S.h[0], 32, &li, q));
        lnp = q;
    } else {
        RC(ln(1, ws + S.h[0], ws + S.n1, n2, 32, 32, 0, np));
        RC(lstm(1, ws + S.n1, 32));
    }
    // Inference rollouts: hidden2 / hidden4 feed only enc1 / enc2, so their norms are applied while those convs stage their input
    // (run_conv3x3s2_ln) instead of by a launch of their own; training keeps the materialised tensors (the backward sweep reads them).
    // Training plans take the same launch (round 6) and have it WRITE the normalised hidden2 / hidden4 (every input pixel of a stride-2 3x3 conv is the
    // tap (1..2, 1..2) of exactly one anchor) and the samples' (mean, rstd) for the backward sweep: two ln_apply launches per timestep less.
    if (np > 0 && (p->opt[PIVP_OPT_LN_FOLD_TRAIN] || !train) && conv3x3s2_ln_ok(32, 32, B, p->H2, p->W2)) {
        Conv3x3LnOpts o{};
        if (train) o.keep = keep(2, ws + S.n2, 32);
        RC(run_conv3x3s2_ln(ws + S.h[1], 32, P(p, p->i_enc_w[1]), P(p, p->i_enc_b[1]), ws + S.cat6 + 64, 32, 96, 1, B, p->H2, p->W2, s, norm_in(2), o));
    } else {
        RC(ln(2, ws + S.h[1], ws + S.n2, n2, 32, 32, 0, np));
        RC(run_conv3x3s2(ws + S.n2, 32, 32, P(p, p->i_enc_w[1]), P(p, p->i_enc_b[1]), ws + S.cat6 + 64, 32, 96, 1, B, p->H2, p->W2, s, 0));
    }
    // group 2 (TM:597)
    RC(lstm(2, ws + S.cat6 + 64, 96));
    const bool fold_l4 = !train && np > 0 && convlstm_ln_in_ok(md.precision, 64, 64, 64, B, p->H4, p->W4) &&
                         (long)B * (p->H4 / 8) * (p->W4 / 16) >= 64;
    if (fold_l4) {
        const LnIn li = norm_in(3);
        float* q = other(lnp);
        RC(lstm(3, ws + S.h[2], 64, &li, q));
        lnp = q;
    } else {
        RC(ln(3, ws + S.h[2], ws + S.n3, n4, 64, 64, 0, np));
        RC(lstm(3, ws + S.n3, 64));
    }
    bool enc3_done = false;
    if (train && np > 0 && p->opt[PIVP_OPT_LN_FOLD_TRAIN] && conv3x3s2_ln_ok(64, 64, B, p->H4, p->W4)) {
        Conv3x3LnOpts o{};
        o.keep = keep(4, ws + S.n4, 64);
        RC(run_conv3x3s2_ln(ws + S.h[3], 64, P(p, p->i_enc_w[2]), P(p, p->i_enc_b[2]), ws + S.e2, 64, 64, 1, B, p->H4, p->W4, s, norm_in(4), o));
    } else
    if (!train && np > 0 && conv3x3s2_ln_ok(64, 64, B, p->H4, p->W4)) {
        // Inference: group 3 (TM:598) and the state predictor (TM:730) in enc2's epilogue (round 6): enc3_state_kernel's launch
        // disappears; bit-identical to it (the same fmaf chain on the matrix cores).  PIVP_OPT_FUSE_ENC3 = 0: two launches, as before.
        Enc3Fuse f3;
        memset(&f3, 0, sizeof(f3));
        if (p->opt[PIVP_OPT_FUSE_ENC3] && (p->H8 * p->W8) % 32 == 0) {
            f3.w3 = P(p, p->i_enc_w[3]); f3.b3 = P(p, p->i_enc_b[3]); f3.action = action; f3.state = state_prev; f3.wcs = P(p, p->i_cs_w); f3.bcs = P(p, p->i_cs_b);
            f3.e3 = ws + S.e3; f3.state_out = state_out; f3.use_state = c.use_state;
            enc3_done = true;
        }
        Conv3x3LnOpts o{};
        o.fuse3 = &f3;
        RC(run_conv3x3s2_ln(ws + S.h[3], 64, P(p, p->i_enc_w[2]), P(p, p->i_enc_b[2]), ws + S.e2, 64, 64, 1, B, p->H4, p->W4, s, norm_in(4), o));
    } else {
        RC(ln(4, ws + S.h[3], ws + S.n4, n4, 64, 64, 0, np));
        RC(run_conv3x3s2(ws + S.n4, 64, 64, P(p, p->i_enc_w[2]), P(p, p->i_enc_b[2]), ws + S.e2, 64, 64, 1, B, p->H4, p->W4, s, 0));
    }
    // group 3 (TM:598) + state predictor (TM:730)
    if (!enc3_done)
    RC(enc3_state(ws + S.e2, action, state_prev, P(p, p->i_enc_w[3]), P(p, p->i_enc_b[3]), P(p, p->i_cs_w), P(p, p->i_cs_b),
                  ws + S.e3, state_out, B, p->H8 * p->W8, c.use_state, s));
    // group 4 (TM:599)
    RC(lstm(4, ws + S.e3, 64));
    // (hidden5's norm was folded the same way into enc4's four-phase form and the motion head's Linear, which then has to run here, in front
    // of lstm6: the two consumers lost more than the launch saves, rollout 8.52 -> 8.60 ms.  It keeps its own launch.)
    RC(ln(5, ws + S.h[4], ws + S.n5, n8, 128, 128, 0, np));
    // enc4 and the motion head's Linear both read hidden5 and nothing else: when the output side runs as frame_head (which finishes the
    // Linear's partial sums itself), the two share ONE grid here -- 1,024 + 256 blocks that each filled a fraction of the chip
    const bool fh = frame_head_pays(c.model_type, B, H, W, c.num_masks);
    const bool fh_fin = fh && c.model_type != PIVP_MODEL_DNA && frame_head_finishes(p->K5);
    bool partials_done = false;
    if (fh_fin && md.deconv(false) == Operand::F32) {
        RC(run_deconv3x3s2_and_partials(ws + S.n5, 128, P(p, p->i_enc_w[4]), P(p, p->i_enc_b[4]), ws + S.e4, 128, 128, 1, B, p->H8, p->W8, s,
                                        P(p, p->i_head_w), ws + p->o_linpart, c.model_type == PIVP_MODEL_STP ? 1 : 0));
        partials_done = true;
    } else {
        DeconvOpts o{};
        o.operand = md.deconv(false);
        RC(run_deconv3x3s2(ws + S.n5, 128, 128, P(p, p->i_enc_w[4]), P(p, p->i_enc_b[4]), ws + S.e4, 128, 128, 1, B, p->H8, p->W8, s, o));
    }
    // group 5 (TM:600): lstm6 -> hidden6 -> concat(., enc1) -> enc5 -> relu
    RC(lstm(5, ws + S.e4, 128));
    const Operand dform = md.deconv(true);      // enc5 / enc6
    // The norms of hidden6 / hidden7 feed only enc5 / enc6, whose tile kernel applies them while it stages its patch ([hidden6 | enc1],
    // [hidden7 | enc0] as two sources).
    // Training plans take the same launch and have it WRITE the normalised hidden6 / hidden7 (each pixel by the block that owns it) and the
    // samples' (mean, rstd) for the backward sweep: no ln_apply launch there either.
    // Only while the norm is a launch-bound 5-us kernel (<= 6 MB of hidden tensor: 64 x 64 frames at B = 32): the consumer's column blocks
    // each stage the patch and its gamma / beta again, which at config 5's 128 x 128 costs more than one bandwidth-bound ln_apply pass
    // (B = 32, T = 20: rollout 65.5 -> 65.9 ms with the fold, so it is not taken there).
    auto fold_small = [&](long long floats) { return floats * 4 <= 6LL << 20; };
    // The motion head's finisher (sum of the Linear's K-slice partials, bias, activation, normalisation: per-SAMPLE work) rides behind enc5's tiles as
    // B extra blocks (192 tiles on 256 CUs at B = 32) instead of being repeated by each of frame_head's 16 bands per sample (round 6).
    bool finished = false;
    if (np > 0 && fold_small((long long)B * n4) && deconv3x3s2_ln_ok(64, 32, 96, B, p->H4, p->W4)) {
        MotionRider rd;
        memset(&rd, 0, sizeof(rd));
        if (fh_fin && p->opt[PIVP_OPT_FINISH_RIDER]) {
            if (!partials_done) { RC(motion_partials(ws + S.n5, P(p, p->i_head_w), ws + p->o_linpart, B, p->K5, c.model_type == PIVP_MODEL_STP ? 1 : 0, s)); partials_done = true; }
            rd.mode = c.model_type == PIVP_MODEL_STP ? 2 : 1; rd.KS = cdna_kernel_partials_slices(p->K5); rd.nout = 25 * c.num_masks;
            rd.partials = ws + p->o_linpart; rd.bias = P(p, p->i_head_b); rd.vpre = ws + S.vpre;
            if (rd.mode == 2) { rd.w2 = P(p, p->i_head2_w); rd.b2 = P(p, p->i_head2_b); rd.out = ws + S.theta; }
            else rd.out = ws + S.kerns;
            finished = true;
        }
        DeconvLnOpts o{};
        o.x1 = ws + S.cat6 + 64; o.c1 = 32; o.ld1 = 96;
        o.operand = dform; o.wscale_part = ws + p->o_wabs[0];
        if (train) o.keep = keep(6, ws + S.cat6, 96);
        o.rider = &rd;
        RC(run_deconv3x3s2_ln(ws + S.h[5], 64, P(p, p->i_enc_w[5]), P(p, p->i_enc_b[5]), ws + S.e5, 96, 96, 1, B, p->H4, p->W4, s, norm_in(6), o));
    } else {
        RC(ln(6, ws + S.h[5], ws + S.cat6, n4, 64, 96, 0, np));
        DeconvOpts o{};
        o.operand = dform; o.wscale_part = ws + p->o_wabs[0];
        RC(run_deconv3x3s2(ws + S.cat6, 96, 96, P(p, p->i_enc_w[5]), P(p, p->i_enc_b[5]), ws + S.e5, 96, 96, 1, B, p->H4, p->W4, s, o));
    }
    // group 6 (TM:601): lstm7 -> hidden7 -> concat(., enc0) -> enc6 -> norm_enc6 -> relu
    RC(lstm(6, ws + S.e5, 96));
    if (np > 0 && fold_small((long long)B * n2) && deconv3x3s2_ln_ok(32, 32, 64, B, p->H2, p->W2)) {
        // enc6's blocks write the partials of norm_enc6 while others still read hidden7's: the second partial buffer
        float* lnp2 = other(lnp);
        const LnIn li = norm_in(7);      // (np as hidden7's producer left it: the launch overwrites it)
        DeconvLnOpts o{};
        o.x1 = ws + S.cat7 + 32; o.c1 = 32; o.ld1 = 64;
        o.ln_out.part = lnp2; o.ln_out.cap = ln_cap; o.ln_out.nparts = &np;
        o.operand = dform; o.wscale_part = ws + p->o_wabs[1];
        if (train) o.keep = keep(7, ws + S.cat7, 64);
        RC(run_deconv3x3s2_ln(ws + S.h[6], 32, P(p, p->i_enc_w[6]), P(p, p->i_enc_b[6]), ws + S.e6raw, 64, 64, 0, B, p->H2, p->W2, s, li, o));
        lnp = lnp2;
    } else {
        RC(ln(7, ws + S.h[6], ws + S.cat7, n2, 32, 64, 0, np));
        DeconvOpts o{};
        o.ln_out.part = lnp; o.ln_out.cap = ln_cap; o.ln_out.nparts = &np;
        o.operand = dform; o.wscale_part = ws + p->o_wabs[1];
        RC(run_deconv3x3s2(ws + S.cat7, 64, 64, P(p, p->i_enc_w[6]), P(p, p->i_enc_b[6]), ws + S.e6raw, 64, 64, 0, B, p->H2, p->W2, s, o));
    }
    // heads (TM:711-728).  One launch (csrc/frame_head.hip) for norm_enc6 + relu + the 1x1 heads + the motion head's finisher + flat softmax +
    // transform + compositing, behind the Linear's partial sums: bit-identical to the four launches below it, which remain for geometries
    // it does not take or where it is slower (frames wider than 64: frame_head_pays).  The softmaxed masks are kept for the rollout's last step only (pivp_get_tap).
    if (fh && np > 0) {
        const bool fin = !finished && (c.model_type == PIVP_MODEL_DNA || frame_head_finishes(p->K5));
        FrameHeadArgs a;
        memset(&a, 0, sizeof(a));
        if (finished) {
            a.aux = c.model_type == PIVP_MODEL_STP ? ws + S.theta : ws + S.kerns;
        } else if (c.model_type == PIVP_MODEL_CDNA) {
            if (fin) { if (!partials_done) RC(motion_partials(ws + S.n5, P(p, p->i_head_w), ws + p->o_linpart, B, p->K5, 0, s)); }
            else RC(cdna_kernels(ws + S.n5, P(p, p->i_head_w), P(p, p->i_head_b), ws + p->o_linpart, ws + S.kerns, B, p->K5, c.num_masks, s, ws + S.vpre));
            a.aux = ws + S.kerns; a.kerns_out = ws + S.kerns;
        } else if (c.model_type == PIVP_MODEL_STP) {
            if (fin) { if (!partials_done) RC(motion_partials(ws + S.n5, P(p, p->i_head_w), ws + p->o_linpart, B, p->K5, 1, s)); }
            else RC(stp_params(ws + S.n5, P(p, p->i_head_w), P(p, p->i_head_b), P(p, p->i_head2_w), P(p, p->i_head2_b), ws + p->o_linpart,
                               ws + S.theta, B, p->K5, s, ws + S.vpre));
            a.aux = ws + S.theta; a.kerns_out = ws + S.theta; a.w2 = P(p, p->i_head2_w); a.b2 = P(p, p->i_head2_b);
        }
        if (fin && c.model_type != PIVP_MODEL_DNA) {
            a.partials = ws + p->o_linpart; a.KS = cdna_kernel_partials_slices(p->K5); a.hbias = P(p, p->i_head_b); a.aux = nullptr;
            a.vpre_out = ws + S.vpre;
        } else {
            a.kerns_out = nullptr;      // already written by the separate finisher
        }
        a.e6raw = ws + S.e6raw; a.ln_part = lnp; a.ln_nparts = np; a.gamma = P(p, p->i_ln_g[8]); a.beta = P(p, p->i_ln_b[8]); a.eps = eps;
        a.wm = P(p, p->i_masks_w); a.bm = P(p, p->i_masks_b); a.we = P(p, p->i_enc7_w); a.be = P(p, p->i_enc7_b);
        a.prev = prev; a.out = gen_out; a.enc7 = ws + S.enc7;
        a.masks_out = (t == c.seq_len - 2 || p->masks_every_step) ? ws + p->o_masks : nullptr;
        a.stat_out = ws + S.lnstat + (size_t)8 * B * 2;
        if (train) { a.logits_out = ws + S.logits; a.layer0_out = ws + S.layer0; a.y_out = ws + S.e6; }
        a.B = B; a.H = H; a.W = W; a.NM = c.num_masks; a.stp_zero = c.stp_zero_border;
        return frame_head(a, c.model_type, s);
    }
    if (np > 0 && (H * W) % 64 == 0) {
        RC(heads_1x1(ws + S.e6raw, P(p, p->i_masks_w), P(p, p->i_masks_b), P(p, p->i_enc7_w), P(p, p->i_enc7_b),
                     ws + S.logits, ws + S.enc7, ws + S.layer0, B, H * W, p->NP, p->NE, c.model_type, s,
                     lnp, np, P(p, p->i_ln_g[8]), P(p, p->i_ln_b[8]), eps, train ? ws + S.e6 : nullptr,
                     ws + S.lnstat + (size_t)8 * B * 2));
    } else {
        RC(ln(8, ws + S.e6raw, ws + S.e6, 64 * H * W, 64, 64, 1, np));
        RC(heads_1x1(ws + S.e6, P(p, p->i_masks_w), P(p, p->i_masks_b), P(p, p->i_enc7_w), P(p, p->i_enc7_b),
                     ws + S.logits, ws + S.enc7, ws + S.layer0, B, H * W, p->NP, p->NE, c.model_type, s));
    }
    // (The motion head's generator needs hidden5 only and could run on the side stream under lstm6 .. heads: measured, the rollout got
    // SLOWER, 8.68 -> 8.79 ms: the co-running kernels cost the ConvLSTMs more than the 16 us they hide; again with the ConvLSTM waves at
    // priority 3 and the generator at 0: 8.57 -> 8.67 / 8.73 ms; and forked only behind norm(hidden7), i.e. beside enc6 and the heads kernel,
    // no ConvLSTM: 8.60 -> 8.68 / 8.69 ms -- a cross-stream event pair per timestep costs more than the 16 us.  It stays in line.)
    const float* aux = nullptr;
    if (c.model_type == PIVP_MODEL_CDNA) {
        RC(cdna_kernels(ws + S.n5, P(p, p->i_head_w), P(p, p->i_head_b), ws + p->o_linpart, ws + S.kerns, B, p->K5, c.num_masks, s,
                        ws + S.vpre));
        aux = ws + S.kerns;
    } else if (c.model_type == PIVP_MODEL_STP) {
        RC(stp_params(ws + S.n5, P(p, p->i_head_w), P(p, p->i_head_b), P(p, p->i_head2_w), P(p, p->i_head2_b),
                      ws + p->o_linpart, ws + S.theta, B, p->K5, s, ws + S.vpre));
        aux = ws + S.theta;
    } else {
        aux = ws + S.enc7;
    }
    RC(composite(prev, ws + S.logits, ws + S.layer0, aux, gen_out, ws + p->o_masks, B, H, W, c.num_masks,
                 c.model_type, c.stp_zero_border, s));
    return PIVP_OK;
}

// the frame fed to step t (TM:663-673)
const float* pivp::step_input(const pivp_plan* plan, int t, const float* images, const unsigned char* gt_select, const float* gen_images, size_t fr) {
    const int ctx = plan->cfg.context_frames;
    if (t < ctx) return images + t * fr;
    if (!gt_select) return gen_images + (t - 1) * fr;
    return plan->ws + plan->slabs[t % plan->nslabs].prevsel;
}

// in front of a rollout's first timestep (pivp_rollout_forward and pivp_rollout_predict)
static int rollout_prepare_packs(pivp_plan* plan, hipStream_t s) {
    // The precision modes' weight packs: rebuilt at the start of every rollout (the parameters may have changed since the last call: optimizer step,
    // checkpoint load) unless the caller keeps them -- pivp_plan_set_pack_cache(plan, 1) -- and reports every change with pivp_plan_params_changed.
    const bool repack = !(plan->pack_cache && plan->packs_valid);
    const Modes& md = plan->mode;
    if (repack && operand_needs_scale(md.precision)) {  // two fp16 pieces: the enc5 / enc6 weights' scales (their tile kernel splits the fp32 weights while it stages them)
        RC(absmax_partials(P(plan, plan->i_enc_w[5]), 9L * 96 * 96, plan->ws + plan->o_wabs[0], s));
        RC(absmax_partials(P(plan, plan->i_enc_w[6]), 9L * 64 * 64, plan->ws + plan->o_wabs[1], s));
    }
    if (repack && md.precision == Operand::BF16) {      // one bf16 plane: the seven packs in one launch
        WeightPrepJob jobs[7];
        for (int i = 0; i < 7; ++i)
            jobs[i] = WeightPrepJob{1, P(plan, plan->i_lstm_w[i]), plan->ws + plan->o_wbf16[i], kLstm[i].cx + kLstm[i].C, 4 * kLstm[i].C, 4 * kLstm[i].C, 0};
        RC(weight_prep_batch(jobs, 7, s));
    } else if (repack && md.packs())
        for (int i = 0; i < 7; ++i)
            RC(pack_lstm_bf16(P(plan, plan->i_lstm_w[i]), reinterpret_cast<unsigned short*>(plan->ws + plan->o_wbf16[i]),
                              kLstm[i].cx + kLstm[i].C, 4 * kLstm[i].C, s, md.precision));
    plan->packs_valid = 1;
    return PIVP_OK;
}

// behind a rollout's last timestep: the last slab's (c, h) of the seven cells -> the registered state_out, ONE launch (csrc/state.hip)
static int rollout_pack_state(pivp_plan* plan, hipStream_t s) {
    if (!plan->state_out) return PIVP_OK;
    const pivp_config_t& c = plan->cfg;
    const Slab& S = plan->slabs[(c.seq_len - 2) % plan->nslabs];
    StateSeg seg[STATE_SEGMENTS];
    for (int g = 0; g < STATE_SEGMENTS; ++g)
        seg[g] = StateSeg{plan->ws + (g % 2 ? S.h[g / 2] : S.c[g / 2]), plan->state_out + state_seg_offset(c, g), state_seg_floats(c, g)};
    return state_copy(seg, nullptr, c.batch, s);
}

extern "C" int pivp_rollout_forward(pivp_plan_t* plan, const float* images, const float* actions, const float* states,
                                    const unsigned char* gt_select, float* gen_images, float* gen_states, float* results,
                                    void* stream) {
    if (!plan || !images || !actions || !states || !gen_images || !gen_states || !results) return PIVP_ERR_BADARG;
    if (!plan->ws) return PIVP_ERR_STATE;
    for (const ParamInfo& pi : plan->params) if (!pi.ptr) return PIVP_ERR_STATE;
    hipStream_t s = (hipStream_t)stream;
    const pivp_config_t& c = plan->cfg;
    const int B = c.batch, T = c.seq_len, ctx = c.context_frames;
    const size_t fr = (size_t)B * 3 * c.height * c.width;
    plan->last = {};                         // an error below leaves nothing to tap or back-propagate
    RC(rollout_prepare_packs(plan, s));
    for (int t = 0; t < T - 1; ++t) {
        if (t >= ctx && gt_select)                                     // TM:667-670
            RC(run_select_frames(images + t * fr, gen_images + (t - 1) * fr, gt_select + (size_t)t * B,
                                 plan->ws + plan->slabs[t % plan->nslabs].prevsel, B, (int)(fr / B), s));
        const float* prev = step_input(plan, t, images, gt_select, gen_images, fr);
        const float* st_prev = t == 0 ? states : gen_states + (size_t)(t - 1) * B * 5;   // TM:646, TM:730
        RC(run_step(plan, t, prev, actions + (size_t)t * B * 5, st_prev, gen_images + t * fr, gen_states + (size_t)t * B * 5, s));
    }
    RC(rollout_pack_state(plan, s));
    // loss (TM:737-759): frames ctx..T-1 vs gen[ctx-1..T-2]
    const int nf = T - ctx;
    float* lp = plan->ws + plan->o_losspart;
    // target frames and predictions are contiguous over time: when a frame is a whole number of partial chunks, ONE launch over
    // all nf frames leaves the partials in the same per-frame layout as nf launches would
    const bool whole_chunks = loss_partials_count((int)fr + 1) == loss_partials_count((int)fr) + 1;   // fr divisible by the chunk
    if (nf > 0 && (whole_chunks || nf == 1) && fr * nf < (1u << 30)) {
        RC(frame_sqerr_partials(images + (size_t)ctx * fr, gen_images + (size_t)(ctx - 1) * fr, lp, (int)(fr * nf), s));
    } else {
        for (int i = 0; i < nf; ++i)
            RC(frame_sqerr_partials(images + (size_t)(ctx + i) * fr, gen_images + (size_t)(ctx - 1 + i) * fr,
                                    lp + (size_t)i * plan->loss_nparts, (int)fr, s));
    }
    RC(loss_finalize(lp, plan->loss_nparts, nf, (int)fr, states + (size_t)ctx * B * 5, gen_states + (size_t)(ctx - 1) * B * 5,
                     B * 5, (float)(T - ctx), results, s));
    // state_in: what the sweep's t = 0 will read again when it is enabled (pivp_plan_set_state_grad) -- gone if this rollout wrote its final state over it
    plan->last = LastRollout{T - 1, gt_select != nullptr, false, plan->state_in != nullptr, plan->state_in, plan->state_in && plan->state_in == plan->state_out};
    return PIVP_OK;
}

// Open-loop rollout (include/pivp_hip.h): the timesteps of pivp_rollout_forward in feed-self mode, no loss; optionally P tracked planes advected
// behind every step's head into caller-owned memory.
extern "C" int pivp_rollout_predict(pivp_plan_t* plan, const float* context_images, const float* actions, const float* state0,
                                    const float* track_in, int track_planes, int track_frame,
                                    float* gen_images, float* gen_states, float* track_out, void* stream) {
    if (!plan || !context_images || !actions || !state0 || !gen_images || !gen_states) return PIVP_ERR_BADARG;
    const pivp_config_t& c = plan->cfg;
    // the leading steps fed from context_images: the configuration's, or what pivp_plan_set_rollout_state registered (include/pivp_state.h)
    const int B = c.batch, T = c.seq_len, ctx = plan->observed > 0 ? plan->observed : c.context_frames, P = track_planes, f = track_frame;
    if (ctx < 1 || T - 1 < ctx) return PIVP_ERR_BADARG;
    if (track_in ? (P < 1 || P > 8 || !track_out || f < 0 || f > ctx - 1) : P != 0) return PIVP_ERR_BADARG;
    if (!plan->ws) return PIVP_ERR_STATE;
    for (const ParamInfo& pi : plan->params) if (!pi.ptr) return PIVP_ERR_STATE;
    hipStream_t s = (hipStream_t)stream;
    const size_t fr = (size_t)B * 3 * c.height * c.width;
    const size_t pl = (size_t)B * P * c.height * c.width;
    plan->last = {};                         // an error below leaves nothing to tap or back-propagate
    RC(rollout_prepare_packs(plan, s));
    int rc = PIVP_OK;
    for (int t = 0; t < T - 1 && rc == PIVP_OK; ++t) {
        plan->masks_every_step = P > 0 && t >= f;
        const float* prev = t < ctx ? context_images + t * fr : gen_images + (t - 1) * fr;      // TM:663-666
        const float* st_prev = t == 0 ? state0 : gen_states + (size_t)(t - 1) * B * 5;
        rc = run_step(plan, t, prev, actions + (size_t)t * B * 5, st_prev, gen_images + t * fr, gen_states + (size_t)t * B * 5, s);
        if (rc == PIVP_OK && P > 0 && t >= f) {
            const Slab& S = plan->slabs[t % plan->nslabs];
            const float* aux = plan->ws + (c.model_type == PIVP_MODEL_CDNA ? S.kerns : c.model_type == PIVP_MODEL_STP ? S.theta : S.enc7);
            rc = pixel_track(t == f ? track_in : track_out + (size_t)(t - f - 1) * pl, plan->ws + plan->o_masks, aux,
                             track_out + (size_t)(t - f) * pl, B, P, c.height, c.width, c.num_masks, c.model_type, c.stp_zero_border, s);
        }
    }
    plan->masks_every_step = false;
    if (rc != PIVP_OK) return rc;
    RC(rollout_pack_state(plan, s));
    plan->last = LastRollout{T - 1, false, true, plan->state_in != nullptr, nullptr, false};
    return PIVP_OK;
}
