// The plan's forward side (plan.h): one timestep of the op program, and the two rollouts that sequence it.
#include "plan.h"

using namespace pivp;

namespace {

// what varies from one timestep of a rollout to the next
struct StepIn { int t; const float* prev; const float* action; const float* state_prev; float* gen_out; float* state_out; };

// One pivp_rollout_forward / pivp_rollout_predict call: what the rollout passes to its own steps and what a step mutates on the host live here -- the plan
// is read only.  Which forms the launches take is the plan's StepForm (plan.h); a step adds the run-time half, np.
struct Rollout {
    // ---- constants of the call.  ctx: the leading steps fed from the caller's frames; state_in: the registered (c, h) step 0 reads (null: zeros);
    // prof: the plan's profile record (null: profiling is off) ----
    const pivp_plan& p; hipStream_t s; int ctx; const float* state_in; StepProfile* prof;
    bool masks_every_step = false;    // pivp_rollout_predict with tracked planes: the head writes its softmaxed masks at every step
    const pivp_config_t& c = p.cfg; const StepForm& f = p.form; const Modes& md = p.mode;
    float* const ws = p.ws; float* const lnpA = ws + p.o_lnpart; float* const lnpB = ws + p.o_lnpart2;
    const int B = c.batch, H = c.height, W = c.width;
    const float eps = c.ln_eps;
    const int ln_cap = ln_partial_cap(H * W);   // partial slots per sample in lnp (see the workspace carve)
    const int n2 = 32 * p.H2 * p.W2, n4 = 64 * p.H4 * p.W4, n8 = 128 * p.H8 * p.W8;
    // ---- the step in flight: set at the top of step() ----
    int t = 0; const Slab* S = nullptr; const Slab* Sp = nullptr;      // the step's slab and the one below it (t = 0: none)
    float* lnp = nullptr; int np = 0;       // the LayerNorm partials of the tensor last produced: their buffer, and how many per sample its launcher reported (0: none)
    bool enc3_done = false;                 // enc2's epilogue ran enc3 + the state predictor
    bool partials_done = false;             // the partial sums of the motion head's Linear are in o_linpart
    MotionHead motion = MotionHead::None;   // the form the motion head takes in this step: f.motion, or InHead where the rider's launch did not run

    // t = 0: h == 0, skipped, and c from the zero buffer -- unless the rollout starts from a registered state (pivp_plan_set_rollout_state): then the
    // ordinary two-operand launch on the caller's (c, h)
    const float* hp(int i) const { return Sp ? ws + Sp->h[i] : state_in ? state_in + state_seg_offset(c, 2 * i + 1) : nullptr; }
    const float* cp(int i) const { return Sp ? ws + Sp->c[i] : state_in ? state_in + state_seg_offset(c, 2 * i) : ws + p.o_zero; }
    float* other(float* q) const { return q == lnpA ? lnpB : lnpA; }
    // cell i on x; ln_in: x is the raw output of the cell in front, normalised while staged -- the partials of this cell's own output then go to part_out
    int lstm(int i, const float* x, int ldx, const LnIn* ln_in = nullptr, float* part_out = nullptr) {
        if (prof) prof->begin(s);
        const MapSize m = lstm_map(c, i);
        ConvLstmOpts o{};
        if (f.keep) o.gates_out = ws + S->gates[i];
        // the LayerNorm behind every ConvLSTM gets its statistics from the ConvLSTM epilogue (np partials per sample)
        o.ln_out.part = part_out ? part_out : lnp; o.ln_out.cap = ln_cap; o.ln_out.nparts = &np;
        if (md.packs()) { o.w_bf16 = reinterpret_cast<const unsigned short*>(ws + p.o_wbf16[i]); o.operand = md.precision; }
        o.ln_in = ln_in;
        int rc = run_convlstm(x, kLstm[i].cx, ldx, hp(i), kLstm[i].C, P(&p, p.i_lstm_w[i]), P(&p, p.i_lstm_b[i]),
                              cp(i), ws + S->c[i], ws + S->h[i], B, m.H, m.W, s, o);
        if (prof) prof->end(i + (hp(i) ? 0 : 8), s);   // +8: first-step launch without the h half of K
        return rc;
    }
    float* stat(int j) const { return ws + S->lnstat + (size_t)j * B * 2; }      // norm j's (mean, rstd) per sample
    int ln(int j, const float* x, float* out, int n, int C, int ldo, int relu) {      // norm j by a launch of its own, from the current partials (none: ln_stats first)
        LayerNormOpts o{};
        o.stat_out = stat(j); o.fused_nparts = np;
        return run_layernorm(x, P(&p, p.i_ln_g[j]), P(&p, p.i_ln_b[j]), out, lnp, B, n, C, ldo, eps, relu, s, o);
    }
    LnIn norm_in(int j) const { return LnIn{P(&p, p.i_ln_g[j]), P(&p, p.i_ln_b[j]), lnp, np, eps}; }      // norm j applied by its consumer, from the current partials
    NormKeep keep(int j, float* out, int ld) const { return NormKeep{out, ld, stat(j)}; }                 // ... which a training plan has it write
    // cell i (lstm2 / lstm4) behind norm i of the raw h in front of it: applied while the cell stages its patch (the partials of its own output go to the
    // second buffer: its blocks finish while others still read the input's), or written to `normed` by a launch of its own
    int lstm_behind_norm(int i, size_t normed, int n) {
        const int C = kLstm[i].cx;
        const float* raw = ws + S->h[i - 1];
        if (f.norm_inside[i] && np > 0) {
            const LnIn li = norm_in(i);
            float* q = other(lnp);
            RC(lstm(i, raw, C, &li, q));
            lnp = q;
            return PIVP_OK;
        }
        RC(ln(i, raw, ws + normed, n, C, C, 0));
        return lstm(i, ws + normed, C);
    }
    // enc1 / enc2 (layer e, C channels in and out) behind norm j of the raw h in front of it.  Inference rollouts: hidden2 / hidden4 feed only these convs,
    // so the norm is applied while they stage their input (run_conv3x3s2_ln) instead of by a launch of its own.  Training plans take the same launch
    // (round 6) and have it WRITE the normalised tensor (every input pixel of a stride-2 3x3 conv is the tap (1..2, 1..2) of exactly one anchor) and the
    // samples' (mean, rstd) for the backward sweep: two ln_apply launches per timestep less.  f3 (inference): what enc2's epilogue adds, if anything.
    int enc_behind_norm(int e, int j, size_t normed, int n, int C, float* out, int ldo, int Hin, int Win, const Enc3Fuse* f3) {
        const float* raw = ws + S->h[j - 1];
        if (f.norm_inside[j] && np > 0) {
            Conv3x3LnOpts o{};
            if (f.keep) o.keep = keep(j, ws + normed, C);
            else o.fuse3 = f3;
            return run_conv3x3s2_ln(raw, C, P(&p, p.i_enc_w[e]), P(&p, p.i_enc_b[e]), out, C, ldo, 1, B, Hin, Win, s, norm_in(j), o);
        }
        RC(ln(j, raw, ws + normed, n, C, C, 0));
        return run_conv3x3s2(ws + normed, C, C, P(&p, p.i_enc_w[e]), P(&p, p.i_enc_b[e]), out, C, ldo, 1, B, Hin, Win, s, 0);
    }
    // the motion head's output, and the launch that forms it from hidden5 alone
    float* motion_out() const { return ws + (c.model_type == PIVP_MODEL_STP ? S->theta : S->kerns); }
    int motion_dbl() const { return c.model_type == PIVP_MODEL_STP ? 1 : 0; }
    int motion_separate() {
        if (c.model_type == PIVP_MODEL_CDNA)
            return cdna_kernels(ws + S->n5, P(&p, p.i_head_w), P(&p, p.i_head_b), ws + p.o_linpart, ws + S->kerns, B, p.K5, c.num_masks, s, ws + S->vpre);
        return stp_params(ws + S->n5, P(&p, p.i_head_w), P(&p, p.i_head_b), P(&p, p.i_head2_w), P(&p, p.i_head2_b), ws + p.o_linpart,
                          ws + S->theta, B, p.K5, s, ws + S->vpre);
    }
    int linear_partials() {      // ... its Linear's K-slice partial sums alone, for a finisher elsewhere (once per step)
        if (partials_done) return PIVP_OK;
        partials_done = true;
        return motion_partials(ws + S->n5, P(&p, p.i_head_w), ws + p.o_linpart, B, p.K5, motion_dbl(), s);
    }

    int encoder(const StepIn& in);
    int bottleneck(const StepIn& in);
    int decoder();
    int head(const StepIn& in);
    // forward, one timestep (TM:659-731)
    int step(const StepIn& in) {
        t = in.t;
        S = &p.slabs[t % p.nslabs]; Sp = t > 0 ? &p.slabs[(t - 1) % p.nslabs] : nullptr;
        lnp = lnpA; np = 0;
        enc3_done = partials_done = false;
        motion = f.motion;
        RC(encoder(in));
        RC(bottleneck(in));
        RC(decoder());
        return head(in);
    }
};

int Rollout::encoder(const StepIn& in) {
    // group 0 (TM:595): enc0 -> norm_enc0 -> relu   => cat7[:, 32:64]
    RC(conv_enc0(in.prev, P(&p, p.i_enc_w[0]), P(&p, p.i_enc_b[0]), ws + S->e0raw, B, H, W, s, lnp, ln_cap, &np));
    RC(ln(0, ws + S->e0raw, ws + S->cat7 + 32, n2, 32, 64, 1));
    // group 1 (TM:596): lstm1 -> hidden1 -> lstm2 -> hidden2 -> enc1 -> relu  => cat6[:, 64:96]
    RC(lstm(0, ws + S->cat7 + 32, 64));
    RC(lstm_behind_norm(1, S->n1, n2));
    RC(enc_behind_norm(1, 2, S->n2, n2, 32, ws + S->cat6 + 64, 96, p.H2, p.W2, nullptr));
    // group 2 (TM:597)
    RC(lstm(2, ws + S->cat6 + 64, 96));
    RC(lstm_behind_norm(3, S->n3, n4));
    // Inference: group 3 (TM:598) and the state predictor (TM:730) in enc2's epilogue (round 6): enc3_state_kernel's launch
    // disappears; bit-identical to it (the same fmaf chain on the matrix cores).  PIVP_OPT_FUSE_ENC3 = 0: two launches, as before.
    Enc3Fuse f3;
    memset(&f3, 0, sizeof(f3));
    if (f.enc3_in_enc2 && np > 0) {
        f3.w3 = P(&p, p.i_enc_w[3]); f3.b3 = P(&p, p.i_enc_b[3]); f3.action = in.action; f3.state = in.state_prev; f3.wcs = P(&p, p.i_cs_w); f3.bcs = P(&p, p.i_cs_b);
        f3.e3 = ws + S->e3; f3.state_out = in.state_out; f3.use_state = c.use_state;
        enc3_done = true;
    }
    return enc_behind_norm(2, 4, S->n4, n4, 64, ws + S->e2, 64, p.H4, p.W4, &f3);
}

int Rollout::bottleneck(const StepIn& in) {
    // group 3 (TM:598) + state predictor (TM:730)
    if (!enc3_done)
        RC(enc3_state(ws + S->e2, in.action, in.state_prev, P(&p, p.i_enc_w[3]), P(&p, p.i_enc_b[3]), P(&p, p.i_cs_w), P(&p, p.i_cs_b),
                      ws + S->e3, in.state_out, B, p.H8 * p.W8, c.use_state, s, c.action_dim, c.state_dim));
    // group 4 (TM:599)
    RC(lstm(4, ws + S->e3, 64));
    // (hidden5's norm was folded the same way into enc4's four-phase form and the motion head's Linear, which then has to run here, in front
    // of lstm6: the two consumers lost more than the launch saves, rollout 8.52 -> 8.60 ms.  It keeps its own launch.)
    RC(ln(5, ws + S->h[4], ws + S->n5, n8, 128, 128, 0));
    // enc4 and the motion head's Linear both read hidden5 and nothing else: when the output side runs as frame_head (which finishes the
    // Linear's partial sums itself), the two share ONE grid here -- 1,024 + 256 blocks that each filled a fraction of the chip
    if (f.enc4_partials) {
        RC(run_deconv3x3s2_and_partials(ws + S->n5, 128, P(&p, p.i_enc_w[4]), P(&p, p.i_enc_b[4]), ws + S->e4, 128, 128, 1, B, p.H8, p.W8, s,
                                        P(&p, p.i_head_w), ws + p.o_linpart, motion_dbl()));
        partials_done = true;
        return PIVP_OK;
    }
    DeconvOpts o{};
    o.operand = md.deconv(false);
    return run_deconv3x3s2(ws + S->n5, 128, 128, P(&p, p.i_enc_w[4]), P(&p, p.i_enc_b[4]), ws + S->e4, 128, 128, 1, B, p.H8, p.W8, s, o);
}

int Rollout::decoder() {
    // group 5 (TM:600): lstm6 -> hidden6 -> concat(., enc1) -> enc5 -> relu
    RC(lstm(5, ws + S->e4, 128));
    const Operand dform = md.deconv(true);      // enc5 / enc6
    // The norms of hidden6 / hidden7 feed only enc5 / enc6, whose tile kernel applies them while it stages its patch ([hidden6 | enc1],
    // [hidden7 | enc0] as two sources) -- where StepForm::norm_inside says it pays.
    // Training plans take the same launch and have it WRITE the normalised hidden6 / hidden7 (each pixel by the block that owns it) and the
    // samples' (mean, rstd) for the backward sweep: no ln_apply launch there either.
    if (f.norm_inside[6] && np > 0) {
        // MotionHead::Rider: the motion head's finisher (sum of the Linear's K-slice partials, bias, activation, normalisation: per-SAMPLE work) rides behind
        // enc5's tiles as B extra blocks (192 tiles on 256 CUs at B = 32) instead of being repeated by each of frame_head's 16 bands per sample (round 6).
        MotionRider rd;
        memset(&rd, 0, sizeof(rd));
        if (motion == MotionHead::Rider) {
            RC(linear_partials());
            rd.mode = c.model_type == PIVP_MODEL_STP ? 2 : 1; rd.KS = cdna_kernel_partials_slices(p.K5); rd.nout = 25 * c.num_masks;
            rd.partials = ws + p.o_linpart; rd.bias = P(&p, p.i_head_b); rd.vpre = ws + S->vpre;
            if (rd.mode == 2) { rd.w2 = P(&p, p.i_head2_w); rd.b2 = P(&p, p.i_head2_b); }
            rd.out = motion_out();
        }
        DeconvLnOpts o{};
        o.x1 = ws + S->cat6 + 64; o.c1 = 32; o.ld1 = 96;
        o.operand = dform; o.wscale_part = ws + p.o_wabs[0];
        if (f.keep) o.keep = keep(6, ws + S->cat6, 96);
        o.rider = &rd;
        RC(run_deconv3x3s2_ln(ws + S->h[5], 64, P(&p, p.i_enc_w[5]), P(&p, p.i_enc_b[5]), ws + S->e5, 96, 96, 1, B, p.H4, p.W4, s, norm_in(6), o));
    } else {
        if (motion == MotionHead::Rider) motion = MotionHead::InHead;      // no launch to ride on: frame_head finishes, as it does without the option
        RC(ln(6, ws + S->h[5], ws + S->cat6, n4, 64, 96, 0));
        DeconvOpts o{};
        o.operand = dform; o.wscale_part = ws + p.o_wabs[0];
        RC(run_deconv3x3s2(ws + S->cat6, 96, 96, P(&p, p.i_enc_w[5]), P(&p, p.i_enc_b[5]), ws + S->e5, 96, 96, 1, B, p.H4, p.W4, s, o));
    }
    // group 6 (TM:601): lstm7 -> hidden7 -> concat(., enc0) -> enc6 -> norm_enc6 -> relu
    RC(lstm(6, ws + S->e5, 96));
    if (f.norm_inside[7] && np > 0) {
        // enc6's blocks write the partials of norm_enc6 while others still read hidden7's: the second partial buffer
        float* lnp2 = other(lnp);
        const LnIn li = norm_in(7);      // (np as hidden7's producer left it: the launch overwrites it)
        DeconvLnOpts o{};
        o.x1 = ws + S->cat7 + 32; o.c1 = 32; o.ld1 = 64;
        o.ln_out.part = lnp2; o.ln_out.cap = ln_cap; o.ln_out.nparts = &np;
        o.operand = dform; o.wscale_part = ws + p.o_wabs[1];
        if (f.keep) o.keep = keep(7, ws + S->cat7, 64);
        RC(run_deconv3x3s2_ln(ws + S->h[6], 32, P(&p, p.i_enc_w[6]), P(&p, p.i_enc_b[6]), ws + S->e6raw, 64, 64, 0, B, p.H2, p.W2, s, li, o));
        lnp = lnp2;
    } else {
        RC(ln(7, ws + S->h[6], ws + S->cat7, n2, 32, 64, 0));
        DeconvOpts o{};
        o.ln_out.part = lnp; o.ln_out.cap = ln_cap; o.ln_out.nparts = &np;
        o.operand = dform; o.wscale_part = ws + p.o_wabs[1];
        RC(run_deconv3x3s2(ws + S->cat7, 64, 64, P(&p, p.i_enc_w[6]), P(&p, p.i_enc_b[6]), ws + S->e6raw, 64, 64, 0, B, p.H2, p.W2, s, o));
    }
    return PIVP_OK;
}

// heads (TM:711-728)
int Rollout::head(const StepIn& in) {
    // Output::FrameHead: one launch (csrc/frame_head.hip) for norm_enc6 + relu + the 1x1 heads + the motion head's finisher + flat softmax +
    // transform + compositing, behind the Linear's partial sums: bit-identical to the four launches below it, which remain for geometries
    // it does not take or where it is slower.  The softmaxed masks are kept for the rollout's last step only (pivp_get_tap), or where a rollout asks.
    if (f.output == Output::FrameHead && np > 0) {
        FrameHeadArgs a;
        memset(&a, 0, sizeof(a));
        switch (motion) {
        case MotionHead::None: break;
        case MotionHead::Rider: a.aux = motion_out(); break;      // finished behind enc5's tiles
        case MotionHead::InHead:      // frame_head finishes the partial sums, and leaves the result and the Linear's pre-activation
            RC(linear_partials());
            a.partials = ws + p.o_linpart; a.KS = cdna_kernel_partials_slices(p.K5); a.hbias = P(&p, p.i_head_b);
            a.kerns_out = motion_out(); a.vpre_out = ws + S->vpre;
            break;
        case MotionHead::Separate:
            RC(motion_separate());
            a.aux = motion_out();
            break;
        }
        if (c.model_type == PIVP_MODEL_STP && motion != MotionHead::Rider) { a.w2 = P(&p, p.i_head2_w); a.b2 = P(&p, p.i_head2_b); }
        a.e6raw = ws + S->e6raw; a.ln_part = lnp; a.ln_nparts = np; a.gamma = P(&p, p.i_ln_g[8]); a.beta = P(&p, p.i_ln_b[8]); a.eps = eps;
        a.wm = P(&p, p.i_masks_w); a.bm = P(&p, p.i_masks_b); a.we = P(&p, p.i_enc7_w); a.be = P(&p, p.i_enc7_b);
        a.prev = in.prev; a.out = in.gen_out; a.enc7 = ws + S->enc7;
        a.masks_out = (t == c.seq_len - 2 || masks_every_step) ? ws + p.o_masks : nullptr;
        a.stat_out = stat(8);
        if (f.keep) { a.logits_out = ws + S->logits; a.layer0_out = ws + S->layer0; a.y_out = ws + S->e6; }
        a.B = B; a.H = H; a.W = W; a.NM = c.num_masks; a.stp_zero = c.stp_zero_border;
        return frame_head(a, c.model_type, s);
    }
    // Output::Separate, or enc6's launcher left no partials: heads_1x1 (with norm_enc6 inside it, or behind a launch of its own), the motion head by its own
    // launch whatever the step has formed of it so far, composite
    if (f.norm_inside[8] && np > 0) {
        RC(heads_1x1(ws + S->e6raw, P(&p, p.i_masks_w), P(&p, p.i_masks_b), P(&p, p.i_enc7_w), P(&p, p.i_enc7_b),
                     ws + S->logits, ws + S->enc7, ws + S->layer0, B, H * W, p.NP, p.NE, c.model_type, s,
                     lnp, np, P(&p, p.i_ln_g[8]), P(&p, p.i_ln_b[8]), eps, f.keep ? ws + S->e6 : nullptr, stat(8)));
    } else {
        RC(ln(8, ws + S->e6raw, ws + S->e6, 64 * H * W, 64, 64, 1));
        RC(heads_1x1(ws + S->e6, P(&p, p.i_masks_w), P(&p, p.i_masks_b), P(&p, p.i_enc7_w), P(&p, p.i_enc7_b),
                     ws + S->logits, ws + S->enc7, ws + S->layer0, B, H * W, p.NP, p.NE, c.model_type, s));
    }
    // (The motion head's generator needs hidden5 only and could run on the side stream under lstm6 .. heads: measured, the rollout got
    // SLOWER, 8.68 -> 8.79 ms: the co-running kernels cost the ConvLSTMs more than the 16 us they hide; again with the ConvLSTM waves at
    // priority 3 and the generator at 0: 8.57 -> 8.67 / 8.73 ms; and forked only behind norm(hidden7), i.e. beside enc6 and the heads kernel,
    // no ConvLSTM: 8.60 -> 8.68 / 8.69 ms -- a cross-stream event pair per timestep costs more than the 16 us.  It stays in line.)
    const float* aux = ws + S->enc7;
    if (c.model_type != PIVP_MODEL_DNA) {
        RC(motion_separate());
        aux = motion_out();
    }
    return composite(in.prev, ws + S->logits, ws + S->layer0, aux, in.gen_out, ws + p.o_masks, B, H, W, c.num_masks, c.model_type, c.stp_zero_border, s);
}

// the caller's tensors of a rollout, time-major
struct RolloutIo { const float* images; const float* actions; const float* states; const unsigned char* gt_select; float* gen_images; float* gen_states; };

// what step t reads and writes: the frame fed to it (step_input), its action, the state in front of it (TM:646, TM:730) and where its outputs go
StepIn step_in(const pivp_plan& p, const RolloutIo& io, int t, int ctx) {
    const size_t fr = (size_t)p.cfg.batch * 3 * p.cfg.height * p.cfg.width;
    const size_t ac = (size_t)p.cfg.batch * p.cfg.action_dim, st = (size_t)p.cfg.batch * p.cfg.state_dim;
    return StepIn{t, step_input(&p, t, io.images, io.gt_select, io.gen_images, fr, ctx), io.actions + t * ac,
                  t == 0 ? io.states : io.gen_states + (t - 1) * st, io.gen_images + t * fr, io.gen_states + t * st};
}

// in front of a rollout's first timestep
int rollout_prepare_packs(pivp_plan* plan, hipStream_t s) {
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
int rollout_pack_state(const pivp_plan* plan, hipStream_t s) {
    if (!plan->state_out) return PIVP_OK;
    const pivp_config_t& c = plan->cfg;
    const Slab& S = plan->slabs[(c.seq_len - 2) % plan->nslabs];
    StateSeg seg[STATE_SEGMENTS];
    for (int g = 0; g < STATE_SEGMENTS; ++g)
        seg[g] = StateSeg{plan->ws + (g % 2 ? S.h[g / 2] : S.c[g / 2]), plan->state_out + state_seg_offset(c, g), state_seg_floats(c, g)};
    return state_copy(seg, nullptr, c.batch, s);
}

// The prologue of either rollout, behind its own argument checks: a bound workspace and every parameter, no record of an earlier rollout (an error from
// here on leaves nothing to tap or back-propagate), the weight packs.
int rollout_begin(pivp_plan* plan, hipStream_t s) {
    if (!plan->ws) return PIVP_ERR_STATE;
    for (const ParamInfo& pi : plan->params) if (!pi.ptr) return PIVP_ERR_STATE;
    plan->last = {};
    return rollout_prepare_packs(plan, s);
}
// ... and its epilogue, behind the last timestep: the state pack, what the entry still has to launch (tail), and the record of the call, assigned whole
template <class Tail>
int rollout_end(pivp_plan* plan, hipStream_t s, const LastRollout& rec, Tail tail) {
    RC(rollout_pack_state(plan, s));
    RC(tail());
    plan->last = rec;
    return PIVP_OK;
}

}  // namespace

// the frame fed to step t (TM:663-673)
const float* pivp::step_input(const pivp_plan* plan, int t, const float* images, const unsigned char* gt_select, const float* gen_images, size_t fr, int ctx) {
    if (t < (ctx > 0 ? ctx : plan->cfg.context_frames)) return images + t * fr;
    if (!gt_select) return gen_images + (t - 1) * fr;
    return plan->ws + plan->slabs[t % plan->nslabs].prevsel;
}

extern "C" int pivp_rollout_forward(pivp_plan_t* plan, const float* images, const float* actions, const float* states,
                                    const unsigned char* gt_select, float* gen_images, float* gen_states, float* results,
                                    void* stream) {
    if (!plan || !images || !actions || !states || !gen_images || !gen_states || !results) return PIVP_ERR_BADARG;
    hipStream_t s = (hipStream_t)stream;
    RC(rollout_begin(plan, s));
    const pivp_config_t& c = plan->cfg;
    const int B = c.batch, T = c.seq_len, ctx = c.context_frames;
    const size_t fr = (size_t)B * 3 * c.height * c.width;
    Rollout r{*plan, s, ctx, plan->state_in, plan->prof.on ? &plan->prof : nullptr};
    const RolloutIo io{images, actions, states, gt_select, gen_images, gen_states};
    for (int t = 0; t < T - 1; ++t) {
        if (t >= ctx && gt_select)                                     // TM:667-670
            RC(run_select_frames(images + t * fr, gen_images + (t - 1) * fr, gt_select + (size_t)t * B,
                                 plan->ws + plan->slabs[t % plan->nslabs].prevsel, B, (int)(fr / B), s));
        RC(r.step(step_in(*plan, io, t, ctx)));
    }
    // state_in: what the sweep's t = 0 will read again when it is enabled (pivp_plan_set_state_grad) -- gone if this rollout wrote its final state over it
    const LastRollout rec{T - 1, gt_select != nullptr, false, plan->state_in != nullptr, plan->state_in, plan->state_in && plan->state_in == plan->state_out};
    return rollout_end(plan, s, rec, [&] {
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
        return loss_finalize(lp, plan->loss_nparts, nf, (int)fr, states + (size_t)ctx * B * c.state_dim, gen_states + (size_t)(ctx - 1) * B * c.state_dim,
                             B * c.state_dim, (float)(T - ctx), results, s);
    });
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
    hipStream_t s = (hipStream_t)stream;
    RC(rollout_begin(plan, s));
    const size_t pl = (size_t)B * P * c.height * c.width;
    Rollout r{*plan, s, ctx, plan->state_in, plan->prof.on ? &plan->prof : nullptr};
    const RolloutIo io{context_images, actions, state0, nullptr, gen_images, gen_states};
    for (int t = 0; t < T - 1; ++t) {
        r.masks_every_step = P > 0 && t >= f;
        RC(r.step(step_in(*plan, io, t, ctx)));
        if (r.masks_every_step) {
            const Slab& S = plan->slabs[t % plan->nslabs];
            const float* aux = plan->ws + (c.model_type == PIVP_MODEL_CDNA ? S.kerns : c.model_type == PIVP_MODEL_STP ? S.theta : S.enc7);
            RC(pixel_track(t == f ? track_in : track_out + (size_t)(t - f - 1) * pl, plan->ws + plan->o_masks, aux,
                           track_out + (size_t)(t - f) * pl, B, P, c.height, c.width, c.num_masks, c.model_type, c.stp_zero_border, s));
        }
    }
    return rollout_end(plan, s, LastRollout{T - 1, false, true, plan->state_in != nullptr, nullptr, false}, [] { return PIVP_OK; });
}
