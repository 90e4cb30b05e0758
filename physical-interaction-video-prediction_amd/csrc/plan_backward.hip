// The plan's backward sweep (plan.h): the BPTT of pivp_rollout_backward, its side-stream groups, and the gradients through the recurrent state.
#include <mutex>

#include "plan.h"

using namespace pivp;

// ------------------------------------------------------------------------------------------------------------
// backward through time (what loss.backward() does inside Chainer's optimizer.update, TM:950), all three heads.
// Gradients are ACCUMULATED into the buffers registered with pivp_plan_set_grad (same layouts as the parameters).
// ------------------------------------------------------------------------------------------------------------
// side-lane slots whose weight gradients belong to gradient group g (-1: none); a slot of the stride-2 range also names the layer whose partial sums
// the group reduces
static const int kGroupSlots[6][4] = {{SLOT_ENC + 0, SLOT_HEAD, -1, -1}, {SLOT_LSTM + 6, -1, -1, -1}, {SLOT_ENC + 1, SLOT_LSTM + 5, -1, -1},
                                      {SLOT_ENC + 2, SLOT_LSTM + 4, -1, -1}, {SLOT_ENC + 3, SLOT_LSTM + 3, SLOT_LSTM + 2, -1},
                                      {SLOT_ENC + 4, SLOT_LSTM + 1, SLOT_LSTM + 0, SLOT_ENC0_W}};
// Wave priority of the main stream's kernels during this plan's calls (csrc/pivp_common.h): the device word is rewritten only when the wanted value
// differs from what this process last wrote on the device.
// The cache of what the device words hold is process-wide (the words are per device, not per plan): guarded by a mutex, marked unknown while the
// seven copies are being enqueued and valid only once all of them were accepted.  Plans with DIFFERENT wishes driven concurrently on one device (other
// host threads / streams) may each run with either value: the copies are stream-ordered on the enqueuing plan's stream only.  Results never depend on it.
static int apply_main_prio(pivp_plan* p, hipStream_t s) {
    static std::mutex mu;
    static int current[PIVP_MAX_DEV] = {};      // device words start at 0; -1 = unknown (a setter failed midway)
    const int want = p->main_prio < 0 ? (p->grad_cb ? 0 : 1) : (p->main_prio ? 1 : 0);
    const int dev = pivp_current_device();
    std::lock_guard<std::mutex> lock(mu);
    if (current[dev] == want) return PIVP_OK;
    current[dev] = -1;
    RC(main_prio_set_backward(want, s)); RC(main_prio_set_backward_heads(want, s)); RC(main_prio_set_convlstm_bf16(want, s)); RC(main_prio_set_conv5x5_bf16(want, s));
    RC(main_prio_set_deconv_tile(want, s)); RC(main_prio_set_igemm_f32(want, s)); RC(main_prio_set_igemm_small(want, s));
    current[dev] = want;
    return PIVP_OK;
}
extern "C" int pivp_plan_set_main_priority(pivp_plan_t* plan, int mode) {
    if (!plan || mode < -1 || mode > 1) return PIVP_ERR_BADARG;
    plan->main_prio = mode;
    return PIVP_OK;
}
extern "C" int pivp_plan_set_group_join(pivp_plan_t* plan, int join) {
    if (!plan) return PIVP_ERR_BADARG;
    plan->group_join = join != 0;
    return PIVP_OK;
}
extern "C" int pivp_plan_group_wait(pivp_plan_t* plan, int group, void* stream) {
    if (!plan || group < 0 || group >= 6) return PIVP_ERR_BADARG;
    if (!plan->lane.live()) return PIVP_OK;      // no side stream: nothing to wait for
    for (int k = 0; k < 4; ++k) if (kGroupSlots[group][k] >= 0) RC(plan->lane.wait_slot(kGroupSlots[group][k], (hipStream_t)stream));
    return PIVP_OK;
}

namespace {

// what varies from one timestep of the sweep to the next.  ss: the step's place in the dG / dY rings (sweep_schedule.h)
struct StepIn {
    int t; const float* prev; bool prev_has_grad; const float* action; const float* state_prev;
    bool has_go; float* go; float* go_prev; bool last_step; StepSlots ss;
};

// One pivp_rollout_backward call: everything the sweep mutates on the host lives here, value-initialised per call -- the plan is read only.
struct Sweep {
    // ---- constants of the sweep.  lane: where its weight gradients fork to; null = everything on s (the plan has no side stream, or the sweep forms
    // no parameter gradients, pivp_plan_set_sweep_mode: then no fork, join or side launch happens, and what is left to skip are the launches that form
    // nothing but parameter gradients).  wg_batch: timesteps per ConvLSTM weight-gradient launch (<= wg_cap) ----
    const pivp_plan& p; hipStream_t s; const SideLane* lane; bool params; int wg_batch; long long slab_bytes; const Modes& md;
    const pivp_config_t& c = p.cfg;
    const Grads& g = p.g;
    float* const ws = p.ws;
    float* const lnpart = ws + g.lnpart;
    const int B = c.batch, H = c.height, W = c.width, HW = H * W;
    const int n2 = 32 * p.H2 * p.W2, n4 = 64 * p.H4 * p.W4, n8 = 128 * p.H8 * p.W8;
    const long px2 = (long)B * p.H2 * p.W2, px8 = (long)B * p.H8 * p.W8;
    // ---- the open batches ----
    const float* wg_x[7] = {}; const float* wg_h[7] = {};   // ConvLSTM weight gradients: operands of the first timestep of the open batch
    bool lstm_started[7] = {};        // deterministic sweeps: the cell's weight-gradient slots hold this sweep's sums (before: stored, not added)
    bool ln_touched[9] = {};          // norms whose partial parameter gradients still await their reduction
    WgradDesc enc_desc[5] = {}; bool enc_desc_valid[5] = {};     // enc6, enc5, enc4, enc2, enc1: what this sweep launched (for the reduction of the partial sums)
    int enc_cnt[5] = {};              // timesteps in each layer's open batch (enc6 only counts the steps a frame gradient reaches)
    const float* enc_x0[5] = {};      // ... and the forward input of the batch's first timestep
    bool enc_started[5] = {};         // the layer has launched in this sweep: its partial planes hold sums (before: stored, not added)
    // ---- the step in flight: set at the top of step() ----
    int t = 0; bool last_step = false; StepSlots ss = {};
    const Slab* S = nullptr; const Slab* Sp = nullptr;      // the step's slab and the one below it (t = 0: none)
    int par = 0, eq = 0;                                    // timestep parity; the step's slot of the enc dY rings
    float* d_cat6 = nullptr; float* d_e2 = nullptr; float* d_e6raw = nullptr;
    // a rollout that started from a state (the sweep has checked that it is served, include/pivp_state_grad.h): what t = 0 reads, and whether
    // d loss / d (that state) is wanted behind it
    const float* sin = nullptr; bool want_dstate = false;
    LnFuse lf[7] = {};
    SideFork fe = {};

    // a cell's input gradient: this step's buffer (cur) or the one step t + 1 wrote (its h columns are this step's d h)
    float* DIN(int i, bool cur) const { return ws + g.din[i] + (size_t)(i >= 5 ? (cur ? eq : ss.eq_next) : (cur ? par : par ^ 1)) * g.din_sz[i]; }

    int ln_finish(int j) {
        if (!ln_touched[j] || !params) return PIVP_OK;
        ln_touched[j] = false;
        return ln_bwd_params_reduce(ws + g.ln_ppart[j], G(&p, p.i_ln_g[j]), G(&p, p.i_ln_b[j]), B, (int)ln_numel(c, j), s);
    }
    int lnb(int j, const float* dy, int lddy, const float* y, int ldy, const float* x, float* dx, int n, int C, int relu) {
        RC(ln_backward(dy, lddy, y, ldy, x, ws + S->lnstat + (size_t)j * B * 2, P(&p, p.i_ln_g[j]), lnpart, dx,
                       G(&p, p.i_ln_g[j]), G(&p, p.i_ln_b[j]), B, n, C, relu, s, ws + g.ln_ppart[j]));
        ln_touched[j] = true;
        if (t == 0) RC(ln_finish(j));       // the sweep's last timestep: the partial planes become the gradient
        return PIVP_OK;
    }
    // weight-gradient slots (side_lane.h): which of a slot's two events this step uses, its fork, and join = the main stream waits for the slot's last
    // weight-gradient kernels on the buffer this step rewrites
    int ring_of(int slot) const { return slot < SLOT_ENC ? ss.wg_ring : slot_is_ring(slot) ? ss.eg_ring : par; }
    const SideFork* fork_of(int slot, SideFork& f) const {
        if (!lane) return nullptr;
        f = lane->fork(slot, ring_of(slot));
        return &f;
    }
    int join(int slot) const {
        if (!lane) return PIVP_OK;
        // a dY ring: only a batch's first step meets a slot the ring's previous launch (two batches ago) read.  A parity buffer: its last use was two
        // timesteps ago (never recorded: returns at once)
        if (slot_is_ring(slot) && (slot < SLOT_ENC ? ss.wg_slot : ss.eg_slot)) return PIVP_OK;
        return lane->wait_done(slot, ring_of(slot), s);
    }
    // LayerNorm behind ConvLSTM i (hidden<i+1>): one launch leaves the two sums per sample and the norm's partial parameter planes
    // (ln_bwd_sums_params_kernel); the norm's dx is formed inside the cell's gate backward (lstm_gates_bwd_kernel with LnFuse) and never written.
    // (Round 4 also built the sums from the data gradients' epilogues and the parameter gradients inside the gate kernel -- 63 launches fewer per
    // step, and the step got SLOWER: fp32 28.21 -> 28.48 ms, bf16 11.85 -> 11.89, profiles/r04/NOTES.md 2.  Removed in round 5; in the history.)
    int lnb_cell(int i, const float* dy, int lddy, int n, int C) {
        const int j = i + 1;
        memset(&lf[i], 0, sizeof(lf[i]));
        lf[i].dy = dy; lf[i].lddy = lddy; lf[i].gamma = P(&p, p.i_ln_g[j]); lf[i].stat = ws + S->lnstat + (size_t)j * B * 2;
        lf[i].partials = lnpart; lf[i].S = ln_bwd_slices(n); lf[i].h = ws + S->h[i];
        ln_touched[j] = true;
        return ln_backward(dy, lddy, nullptr, 0, ws + S->h[i], lf[i].stat, lf[i].gamma, lnpart, nullptr,
                           G(&p, p.i_ln_g[j]), G(&p, p.i_ln_b[j]), B, n, C, 0, s, ws + g.ln_ppart[j]);
    }
    int lstmb(int i, const float* x, int ldx, const EpSpec* ep = nullptr) {
        const LstmSpec& L = kLstm[i];
        const MapSize m = lstm_map(c, i);
        const int cin = L.cx + L.C, N = 4 * L.C;
        const size_t dG1 = (size_t)B * m.H * m.W * N;                      // floats of one timestep's dG
        float* ring = ws + g.dG[i] + (size_t)ss.wg_ring * p.wg_cap * dG1;
        // t = 0: no recurrent input and c_{-1} = 0 -- unless the rollout started from a state (sin: the one it read, a constant of this sweep)
        const float* h_prev = Sp ? ws + Sp->h[i] : sin ? sin + state_seg_offset(c, 2 * i + 1) : nullptr;
        float* const absmax_ring = ws + g.dg_absmax + (size_t)(i * 2 + ss.wg_ring) * p.wg_cap * 72;      // dG's partial maxima, 72 floats per ring slot
        SideFork f;
        RC(join(SLOT_LSTM + i));      // a new batch: the ring's previous weight-gradient launch (two batches ago) must have read it
        if (ss.wg_slot == 0) { wg_x[i] = x; wg_h[i] = h_prev; }
        ConvLstmBwdArgs a{};
        a.x = x; a.cx = L.cx; a.ldx = ldx; a.h_prev = h_prev; a.C = L.C; a.w = P(&p, p.i_lstm_w[i]); a.gates = ws + S->gates[i];
        a.c_old = Sp ? ws + Sp->c[i] : sin ? sin + state_seg_offset(c, 2 * i) : ws + p.o_zero; a.c_new = ws + S->c[i];
        a.lda = L.C;      // (dh_a = null: formed from the norm behind the cell, a.ln)
        a.ldb = cin; a.dc = ws + g.dc[i];
        if (!last_step) { a.dh_b = DIN(i, false) + L.cx; a.dc_valid = 1; }
        // the sweep's first visited step with a seed (pivp_plan_set_state_grad): d h of the final state read in place, d c scattered into g.dc in front of the sweep
        else if (p.sg_seed) { a.dh_b = p.sg_seed + state_seg_offset(c, 2 * i + 1); a.ldb = L.C; a.dc_valid = 1; }
        a.dG = ring + (size_t)ss.wg_slot * dG1; a.wt = ws + g.wt_lstm[i]; a.d_in = DIN(i, true);
        a.B = B; a.H = m.H; a.W = m.W;      // dW = null: the weight gradient is batched below; only the fork's `ready` (behind the gate math) is used
        a.wt_ready = 1;
        a.operand = md.dgrad(m.H, m.W, B);      // (a map the L2-direct forms' tiles do not serve: the fp32 kernels take the cell, as in the forward)
        if (a.operand != Operand::F32) a.wt_bf16 = reinterpret_cast<unsigned short*>(ws + g.wtb_lstm[i]);
        if (ss.wg_flush) a.fork = fork_of(SLOT_LSTM + i, f);
        a.ln = &lf[i];
        a.dx_only = t == 0 && !want_dstate ? 1 : 0;      // t = 0: nobody reads d h_{-1} -- unless d loss / d state_in is wanted
        if (operand_needs_scale(md.precision)) a.dg_absmax = absmax_ring + (size_t)ss.wg_slot * 72;
        a.ep = ep; a.det = p.det;
        RC(run_convlstm_backward(a, s));
        if (t == 0) RC(ln_finish(i + 1));       // the sweep's last timestep: the norm's partial parameter planes (written by the gate kernel) become its gradient
        if (!ss.wg_flush || !params) return PIVP_OK;
        // weight + bias gradient of the whole batch: timestep j of it reads slab (first - j) and ring slot j; on the side stream it
        // starts as soon as this step's dG exists, next to this step's own data gradient
        hipStream_t sw = lane ? lane->stream : s;
        const int cnt = ss.wg_slot + 1;
        WgradDesc d;
        lstm_wgrad_geom(d, L.cx, L.C, B, m.H, m.W);
        d.x0 = wg_x[i]; d.ld0 = ldx; d.x1 = wg_h[i]; d.dy = ring; d.dw = G(&p, p.i_lstm_w[i]); d.db = G(&p, p.i_lstm_b[i]);
        d.tcount = cnt; d.ts_x0 = -slab_bytes; d.ts_x1 = -slab_bytes; d.ts_dy = (long long)dG1 * 4;
        if (p.det) {
            // deterministic sweeps: the fp32 slot form (wgrad5x5p) in every precision mode -- each launch adds into the cell's slots (the sweep's first
            // stores), the slots are summed in a fixed order once: a t = 0 without h operand cuts the slots another way, so the batches with h are
            // reduced in front of it and its own launch behind it.  After a start from a state t = 0 has the K of the other batches and simply joins them.
            // (the slot form takes every shape pivp_plan_set_deterministic admits, and it sums the columns of dG itself: run_wgrad holds the launch to that)
            float* part = ws + g.lstm_part[i];
            const bool cut = t == 0 && !wg_h[i];
            if (cut && lstm_started[i])
                RC(lstm_wgrad_reduce(L.cx, L.C, 1, part, G(&p, p.i_lstm_w[i]), G(&p, p.i_lstm_b[i]), B, m.H, m.W, sw, 0, DET_SLOT_J));
            d.part = part; d.part_overwrite = (cut || !lstm_started[i]) ? 1 : 0;
            d.slot_j = DET_SLOT_J;
            RC(run_wgrad(d, sw, Operand::F32, true));
            if (t == 0)
                RC(lstm_wgrad_reduce(L.cx, L.C, wg_h[i] ? 1 : 0, part, G(&p, p.i_lstm_w[i]), G(&p, p.i_lstm_b[i]), B, m.H, m.W, sw, 0, DET_SLOT_J));
            else lstm_started[i] = true;
        } else {
            const Operand wform = md.wgrad(m.H, m.W, B);
            if (operand_needs_scale(wform)) d.dy_absmax = absmax_ring;      // dG's partial maxima of the batch (run_convlstm_backward left them there)
            d.dy_absmax_stride = 72;
            d.form = packed_form_hint(B, c.height, c.width);
            RC(run_wgrad(d, sw, wform));
        }
        return lane ? lane->record_done(SLOT_LSTM + i, ss.wg_ring) : PIVP_OK;
    }
    // The side stream's weight gradients read dY buffers that a later step rewrites (enc0 / the motion head: the buffer of two timesteps ago; the stride-2
    // 3x3 layers: a ring slot of two batches ago): each is joined right in front of the first kernel that rewrites its buffer, not here -- at the top of a
    // timestep the side stream still has the previous timestep's last launches (lstm1's and enc0's weight gradients) in front of it, and the main stream
    // sat idle for ~40 us per timestep.
    // Weight gradients of the stride-2 3x3 layers (k = 0..4: enc6, enc5, enc4, enc2, enc1): a step adds itself to the layer's open batch -- its dY sits in slot
    // ss.eg_slot of the ring, its forward input one slab below the previous step's -- and the step that closes the batch launches ONE weight gradient over all of
    // them on the side stream (wgrad3x3s2.hip: per launch a block pays 37-150 KB of partial planes, per timestep nothing).  run_conv_backward (dW = null) has
    // recorded the fork's `ready` behind the final dY and in front of the data gradient.
    void enc_add(int k, const float* x) { if (!enc_cnt[k]++) enc_x0[k] = x; }
    int enc_flush(int k, bool forked) {
        const int cnt = enc_cnt[k];
        if (!cnt) return PIVP_OK;
        const EncSpec& E = kEnc[k];
        const size_t ring0 = (size_t)ss.eg_ring * p.eg_cap;
        const float* dy0 = k == 0 ? ws + g.e6raw + ring0 * g.e6raw_sz : k == 1 ? ws + g.din[6] + ring0 * g.din_sz[6] : k == 2 ? ws + g.din[5] + ring0 * g.din_sz[5]
                         : k == 3 ? ws + g.e2 + ring0 * g.e2_sz : ws + g.cat6 + ring0 * g.cat6_sz + 64;
        const long long dy_step = 4LL * (long long)(k == 0 ? g.e6raw_sz : k == 1 ? g.din_sz[6] : k == 2 ? g.din_sz[5] : k == 3 ? g.e2_sz : g.cat6_sz);
        hipStream_t sw = s;
        if (lane) {
            const SideFork f = lane->fork(SLOT_ENC + k, ss.eg_ring);
            if (forked) sw = f.side; else RC(fork_begin(&f, s, &sw));
        }
        const MapSize m = level_map(c, E.level);
        WgradDesc& d = enc_desc[k];      // kept: the sweep's last step reduces the partial planes by it
        conv3x3s2_wgrad_geom(d, E.mode, E.c, E.c, B, m.H, m.W);
        d.x0 = enc_x0[k]; d.ld0 = E.ldx; d.dy = dy0; d.ldy = E.ldy; d.dw = G(&p, p.i_enc_w[E.layer]); d.db = G(&p, p.i_enc_b[E.layer]);
        d.tcount = cnt; d.ts_x0 = -slab_bytes; d.ts_dy = dy_step;
        d.part = ws + g.wg_part[k]; d.part_overwrite = enc_started[k] ? 0 : 1;
        RC(run_wgrad(d, sw, Operand::F32, p.det != 0));      // (set_deterministic admits only shapes the tile form serves, column sums included)
        if (lane) RC(lane->record_done(SLOT_ENC + k, ss.eg_ring));
        enc_started[k] = true; enc_desc_valid[k] = true; enc_cnt[k] = 0;
        return PIVP_OK;
    }
    // data gradient of stride-2 3x3 layer k (dW = null: its weight gradient is batched by enc_add / enc_flush).  y: the layer's output when its ReLU mask is still
    // to be applied to dy; dy_add: a second gradient into the same output
    int encb(int k, const float* x, float* dy, const float* y, float* dx, int accum_dx, const float* dy_add = nullptr, int ld_add = 0) {
        const EncSpec& E = kEnc[k];
        const MapSize m = level_map(c, E.level);
        if (params) enc_add(k, x);      // (an empty batch: enc_flush launches nothing)
        ConvBwdArgs a{};
        a.mode = E.mode; a.x = x; a.cin = E.c; a.ldx = E.ldx; a.w = P(&p, p.i_enc_w[E.layer]); a.dy = dy; a.cout = E.c; a.ldy = E.ldy;
        a.y = y; a.ldyy = E.ldo;
        a.wt = ws + g.wt_enc[E.layer]; a.dx = dx; a.lddx = E.c; a.accum_dx = accum_dx;
        a.B = B; a.Hin = m.H; a.Win = m.W;
        a.wt_ready = 1;
        if (ss.eg_flush) a.fork = fork_of(SLOT_ENC + k, fe);
        a.dy_add = dy_add; a.ld_add = ld_add;
        a.operand = md.enc_dgrad();
        RC(run_conv_backward(a, s));
        return ss.eg_flush ? enc_flush(k, true) : PIVP_OK;
    }
    // enc conv k's partial weight-gradient sums -> its gradient (once per sweep, behind its last weight-gradient launch)
    int reduce_enc(int k) {
        if (!enc_desc_valid[k]) return PIVP_OK;
        enc_desc_valid[k] = false;
        RC(igemm_wgrad_reduce(enc_desc[k], lane ? lane->stream : s));
        return lane ? lane->record_done(SLOT_ENC + k, ss.eg_ring) : PIVP_OK;      // (t = 0: behind this step's own launch, same ring)
    }
    // t = 0 is the sweep's final timestep: a gradient group is final once the side stream's weight gradients of its layers are in too
    int done(int group) {
        if (!params || t != 0) return PIVP_OK;      // nothing becomes final, nobody is told
        for (int k = 0; k < 4; ++k) {
            const int sl = kGroupSlots[group][k];
            if (sl < 0) continue;
            // the group's partial sums become gradients, listener or not: behind the conv's last weight-gradient launch, on the same stream
            if (slot_enc_layer(sl) >= 0) RC(reduce_enc(slot_enc_layer(sl)));
            if (p.grad_cb && p.group_join && lane) RC(lane->wait_slot(sl, s));
        }
        if (p.grad_cb) p.grad_cb(p.grad_cb_user, group);
        return PIVP_OK;
    }
    int step(const StepIn& in);
};

int Sweep::step(const StepIn& in) {
    t = in.t; last_step = in.last_step; ss = in.ss;
    S = &p.slabs[t]; Sp = t > 0 ? &p.slabs[t - 1] : nullptr;
    par = t & 1;
    eq = ss.eg_ring * p.eg_cap + ss.eg_slot;
    d_cat6 = ws + g.cat6 + (size_t)eq * g.cat6_sz;
    d_e2 = ws + g.e2 + (size_t)eq * g.e2_sz;
    d_e6raw = ws + g.e6raw + (size_t)eq * g.e6raw_sz;
    sin = t == 0 && p.last.carried ? p.last.state_in : nullptr;
    want_dstate = sin && p.sg_dstate_in;
    const float* const prev = in.prev; const float* const action = in.action; const float* const state_prev = in.state_prev;
    const bool prev_has_grad = in.prev_has_grad, has_go = in.has_go;
    float* const go = in.go; float* const go_prev = in.go_prev;
    // ---- heads (TM:711-728) ----
    if (has_go) {
        if (c.model_type == PIVP_MODEL_CDNA)
            RC(composite_bwd_cdna(prev, ws + S->logits, ws + S->layer0, ws + S->kerns, go, ws + g.dmk, ws + g.dz, ws + g.dkpart,
                                  prev_has_grad ? go_prev : nullptr, 1, B, H, W, c.num_masks, s));
        else if (c.model_type == PIVP_MODEL_STP)
            RC(composite_bwd_stp(prev, ws + S->logits, ws + S->layer0, ws + S->theta, go, ws + g.dmk, ws + g.dz, ws + g.dkpart,
                                 prev_has_grad ? go_prev : nullptr, B, H, W, c.num_masks, c.stp_zero_border, s,
                                 p.det ? reinterpret_cast<unsigned long long*>(ws + g.det_stp_acc) : nullptr));
        else
            RC(composite_bwd_dna(prev, ws + S->logits, ws + S->enc7, go, ws + g.dmk, ws + g.dz, prev_has_grad ? go_prev : nullptr, 1,
                                 B, H, W, s));
        RC(mask_softmax_bwd(ws + S->logits, ws + g.dmk, B, HW, p.NP, s));
        RC(heads_bwd(ws + S->e6, P(&p, p.i_masks_w), P(&p, p.i_enc7_w), ws + g.dmk, ws + g.dz, ws + g.e6, G(&p, p.i_masks_w),
                     G(&p, p.i_masks_b), G(&p, p.i_enc7_w), G(&p, p.i_enc7_b), B, HW, p.NP, p.NE, s, p.det ? ws + g.det_heads : nullptr));
        RC(join(SLOT_HEAD));      // d v (the kernel generator's weight gradient reads it)
        if (c.model_type == PIVP_MODEL_CDNA)
            RC(cdna_kernels_bwd(ws + S->n5, P(&p, p.i_head_w), ws + S->vpre, ws + g.dkpart, composite_bwd_tiles(H, W), ws + g.dv[par], ws + g.n5, 0,
                                G(&p, p.i_head_w), G(&p, p.i_head_b), B, p.K5, c.num_masks, s, fork_of(SLOT_HEAD, fe), p.det ? ws + g.det_dv : nullptr));
        else if (c.model_type == PIVP_MODEL_STP)
            RC(stp_params_bwd(ws + S->n5, P(&p, p.i_head_w), ws + S->vpre, P(&p, p.i_head2_w), ws + g.dkpart, composite_bwd_tiles(H, W),
                              ws + g.dv[par], ws + g.n5, G(&p, p.i_head_w), G(&p, p.i_head_b), G(&p, p.i_head2_w), G(&p, p.i_head2_b),
                              B, p.K5, s, p.det ? ws + g.det_stp : nullptr));
        else if (hipMemsetAsync(ws + g.n5, 0, (size_t)px8 * 128 * 4, s) != hipSuccess) return PIVP_ERR_LAUNCH;   // DNA: no hidden5 head
        // group 6 (TM:601), reversed: norm_enc6 (+relu) <- enc6 deconv <- [hidden7 | enc0]
        RC(join(SLOT_ENC + 0));       // d e6raw
        RC(lnb(8, ws + g.e6, 64, ws + S->e6, 64, ws + S->e6raw, d_e6raw, 64 * HW, 64, 1));
        RC(encb(0, ws + S->cat7, d_e6raw, nullptr, ws + g.cat7, 0));
    } else {
        if (ss.eg_flush) RC(enc_flush(0, false));      // a batch whose last steps no frame gradient reaches
        // no gradient reaches this step's frame: only the recurrent paths are live
        if (hipMemsetAsync(ws + g.cat7, 0, (size_t)px2 * 64 * 4, s) != hipSuccess) return PIVP_ERR_LAUNCH;
        if (hipMemsetAsync(ws + g.n5, 0, (size_t)px8 * 128 * 4, s) != hipSuccess) return PIVP_ERR_LAUNCH;
    }
    if (t == 0) RC(ln_finish(8));   // norm_enc6's backward does not run in a step no gradient reaches (the usual t = 0): finish it here
    RC(done(0));
    RC(lnb_cell(6, ws + g.cat7, 64, n2, 32));
    RC(join(SLOT_ENC + 1));           // enc5's dY = the x part of lstm7's d_in: a ring slot (a batch's first step waits for the ring's previous weight-gradient launch)
    // The x columns of a cell's input gradient are the dY of the enc conv in front of the cell: its ReLU mask (enc5, enc4) or the second gradient path into
    // the same tensor (enc0: + enc6's concat part) is met in the data gradient's epilogue where that kernel has the hook and its grid is unsplit (the bf16 /
    // split-precision forms: 27 relu_mask / add_strided launches fewer per train step at B = 32); otherwise the separate pass runs as before.
    int ep_ok6 = 0, ep_ok5 = 0, ep_ok0 = 0;
    const EpSpec ep6{ws + S->e5, 96, 96, 1, &ep_ok6}, ep5{ws + S->e4, 128, 128, 1, &ep_ok5}, ep0{ws + g.cat7 + 32, 64, 32, 2, &ep_ok0};
    RC(lstmb(6, ws + S->e5, 96, &ep6));
    RC(done(1));
    RC(join(SLOT_ENC + 4));          // enc1's dY lives in d cat6, which enc5's data gradient rewrites
    // group 5 (TM:600): d e5 = x-part of lstm7's d_in (ReLU fused in enc5) <- enc5 deconv <- [hidden6 | enc1]
    RC(encb(1, ws + S->cat6, DIN(6, true), ep_ok6 ? nullptr : ws + S->e5, d_cat6, 0));
    RC(lnb_cell(5, d_cat6, 96, n4, 64));
    RC(join(SLOT_ENC + 2));           // enc4's dY = the x part of lstm6's d_in, likewise
    RC(lstmb(5, ws + S->e4, 128, &ep5));
    RC(done(2));
    // group 4 (TM:599): d e4 = x-part of lstm6's d_in <- enc4 deconv <- hidden5 (also read by the CDNA kernel generator)
    RC(encb(2, ws + S->n5, DIN(5, true), ep_ok5 ? nullptr : ws + S->e4, ws + g.n5, 1));
    RC(lnb_cell(4, ws + g.n5, 128, n8, 128));
    RC(lstmb(4, ws + S->e3, 64));
    RC(done(3));
    // group 3 (TM:598) + state predictor (TM:730): d e3 = x-part of lstm5's d_in (ld 192)
    RC(join(SLOT_ENC + 3));          // d e2
    RC(enc3_state_bwd(ws + S->e2, ws + S->e3, DIN(4, true), 192, action, state_prev, P(&p, p.i_enc_w[3]), P(&p, p.i_cs_w),
                      ws + g.dstate + (size_t)t * B * c.state_dim, d_e2, G(&p, p.i_enc_w[3]), G(&p, p.i_enc_b[3]), G(&p, p.i_cs_w),
                      G(&p, p.i_cs_b), t > 0 ? ws + g.dstate + (size_t)(t - 1) * B * c.state_dim : ws + g.dstate + (size_t)(c.seq_len - 1) * B * c.state_dim,
                      B, p.H8 * p.W8, c.use_state, s, 1, p.det ? ws + g.det_enc3 : nullptr, c.action_dim, c.state_dim));      // d e2 comes out masked by enc2's ReLU
    // d action[t]: the other half of the smeared-input gradient, from the tensors enc3_state_bwd has just read (it wrote d e2 and gradients only)
    if (p.in_dact)
        RC(action_grad(ws + S->e3, DIN(4, true), 192, P(&p, p.i_enc_w[3]), P(&p, p.i_cs_w), ws + g.dstate + (size_t)t * B * c.state_dim,
                       p.in_dact + (size_t)t * B * c.action_dim, B, p.H8 * p.W8, c.use_state, s, c.action_dim, c.state_dim));
    // d states[0]: the state chain ends in slot T-1 of g.dstate (this launch's d state_prev at t = 0; behind its det_rows_reduce in deterministic plans)
    if (t == 0 && p.in_dstate0 &&
        hipMemcpyAsync(p.in_dstate0, ws + g.dstate + (size_t)(c.seq_len - 1) * B * c.state_dim, (size_t)B * c.state_dim * 4, hipMemcpyDeviceToDevice, s) != hipSuccess)
        return PIVP_ERR_LAUNCH;
    // group 2 (TM:597): enc2 conv (ReLU) <- hidden4 <- lstm4 <- hidden3 <- lstm3 <- enc1
    RC(encb(3, ws + S->n4, d_e2, nullptr, ws + g.n4, 0));
    RC(lnb_cell(3, ws + g.n4, 64, n4, 64));
    RC(lstmb(3, ws + S->n3, 64));      // its data gradient's x columns = the dy of hidden3
    RC(lnb_cell(2, DIN(3, true), 128, n4, 64));
    RC(lstmb(2, ws + S->cat6 + 64, 96));
    RC(done(4));
    // group 1 (TM:596): enc1 conv (ReLU) <- hidden2 <- lstm2 <- hidden1 <- lstm1 <- enc0
    RC(encb(4, ws + S->n2, d_cat6 + 64, ws + S->cat6 + 64, ws + g.n2, 0, DIN(2, true), 96));      // d enc1 = enc5's concat part (in d cat6) + lstm3's x gradient, summed in the ReLU-mask pass
    RC(lnb_cell(1, ws + g.n2, 32, n2, 32));
    RC(lstmb(1, ws + S->n1, 32));      // ... of hidden1
    RC(lnb_cell(0, DIN(1, true), 64, n2, 32));
    RC(lstmb(0, ws + S->cat7 + 32, 64, &ep0));
    if (!ep_ok0) RC(add_strided(ws + g.cat7 + 32, 64, DIN(0, true), 64, 32, px2, s));          // d enc0: from enc6's concat + from lstm1
    if (want_dstate) {      // every cell's gate backward and data gradient of t = 0 is enqueued: d c_{-1} sits in g.dc, d h_{-1} in the h columns of this step's d_in
        const float* dcs[7]; const float* dins[7];
        for (int i = 0; i < 7; ++i) { dcs[i] = ws + g.dc[i]; dins[i] = DIN(i, true); }
        RC(state_grad_gather(c, dcs, dins, p.sg_dstate_in, s));
    }
    // group 0 (TM:595): norm_enc0 (+relu) <- enc0 conv <- frame
    RC(join(SLOT_ENC0_W));          // d e0raw
    if (!params) {      // enc0's weight gradient is a launch of its own: only the frame gradient of a feed-self step is left, and norm_enc0's dx feeds nothing else
        if (!prev_has_grad) return PIVP_OK;
        RC(lnb(0, ep_ok0 ? DIN(0, true) : ws + g.cat7 + 32, 64, ws + S->cat7 + 32, 64, ws + S->e0raw, ws + g.e0raw[par], n2, 32, 1));
        return enc0_bwd_data(P(&p, p.i_enc_w[0]), ws + g.e0raw[par], go_prev, 1, B, H, W, s);
    }
    RC(lnb(0, ep_ok0 ? DIN(0, true) : ws + g.cat7 + 32, 64, ws + S->cat7 + 32, 64, ws + S->e0raw, ws + g.e0raw[par], n2, 32, 1));
    RC(enc0_bwd(prev, P(&p, p.i_enc_w[0]), ws + g.e0raw[par], G(&p, p.i_enc_w[0]), G(&p, p.i_enc_b[0]), prev_has_grad ? go_prev : nullptr, 1,
                B, H, W, s, fork_of(SLOT_ENC0_W, fe), p.det ? ws + g.det_enc0 : nullptr));
    RC(done(5));
    return PIVP_OK;
}

}  // namespace

static int rollout_backward_sweep(pivp_plan_t* plan, const float* images, const float* actions, const float* states,
                                  const unsigned char* gt_select, const float* gen_images, const float* gen_states, void* stream);
extern "C" int pivp_rollout_backward(pivp_plan_t* plan, const float* images, const float* actions, const float* states,
                                     const unsigned char* gt_select, const float* gen_images, const float* gen_states, void* stream) {
    if (!plan) return PIVP_ERR_BADARG;
    const int rc = rollout_backward_sweep(plan, images, actions, states, gt_select, gen_images, gen_states, stream);
    // A sweep without parameter gradients forked nothing (rollout_backward_sweep): nothing is joined, and no event of an earlier sweep is waited for
    // (those sweeps joined their own work into the caller's stream before they returned)
    if (!(plan->sweep_mode & PIVP_SWEEP_PARAMS) || !plan->lane.live()) return rc;
    // The side stream's weight gradients are joined whatever the sweep returned: on success the caller's stream is made to wait for
    // them (what it enqueues next -- the all-reduce, Adam -- sees every gradient); after a failure half-way the host waits for both
    // streams, so nothing is still reading the workspace or writing gradients when the caller clears, reuses or frees them.
    hipStream_t s = (hipStream_t)stream;
    if (rc == PIVP_OK && plan->lane.join_all(s) == PIVP_OK) return PIVP_OK;
    plan->lane.sync();
    (void)hipStreamSynchronize(s);
    return rc != PIVP_OK ? rc : PIVP_ERR_LAUNCH;
}
static int rollout_backward_sweep(pivp_plan_t* plan, const float* images, const float* actions, const float* states,
                                  const unsigned char* gt_select, const float* gen_images, const float* gen_states, void* stream) {
    if (!plan || !images || !actions || !states || !gen_images || !gen_states) return PIVP_ERR_BADARG;
    const LastRollout& last = plan->last;
    if (!plan->ws || !plan->has_grads || last.steps != plan->cfg.seq_len - 1) return PIVP_ERR_STATE;
    if (last.predict) return PIVP_ERR_STATE;      // pivp_rollout_predict keeps no loss to differentiate
    // the rollout started from a registered state: served only when enabled (include/pivp_state_grad.h), and only while that state still exists
    if (last.carried && (!plan->sg_enable || last.state_lost)) return PIVP_ERR_STATE;
    if (plan->sg_dstate_in && !(plan->sg_enable && last.carried)) return PIVP_ERR_STATE;      // d loss / d (a state the rollout did not start from)
    if (last.carried && ranges_overlap(plan->sg_dstate_in, last.state_in, state_bytes(plan->cfg))) return PIVP_ERR_STATE;
    if ((gt_select != nullptr) != last.sched) return PIVP_ERR_STATE;
    for (const ParamInfo& pi : plan->params) if (!pi.ptr || !pi.grad) return PIVP_ERR_STATE;
    const bool params = (plan->sweep_mode & PIVP_SWEEP_PARAMS) != 0, own_loss = (plan->sweep_mode & PIVP_SWEEP_BUILTIN_LOSS) != 0;
    if (!own_loss && !plan->frame_seed && !plan->sg_seed) return PIVP_ERR_STATE;      // nothing to differentiate
    // a configuration the forward serves and a backward kernel does not (include/pivp_hip.h): refused in front of the first launch, gradients and workspace untouched
    if (!plan_serves_backward(plan->cfg, plan->det != 0)) return PIVP_ERR_BADARG;
    hipStream_t s = (hipStream_t)stream;
    const pivp_config_t& c = plan->cfg;
    const int B = c.batch, T = c.seq_len, ctx = c.context_frames;
    const size_t fr = (size_t)B * 3 * c.height * c.width;
    float* ws = plan->ws;
    const Grads& g = plan->g;
    const float fscale = 2.0f / ((float)fr * (float)(T - ctx));              // d/d gen of mean-squared error / (T - ctx)
    const float sscale = 2.0f * 1e-4f / ((float)(B * c.state_dim) * (float)(T - ctx));
    const Modes& md = plan->mode;
    // the lane this sweep forks its weight gradients to, decided once: none when the sweep forms no parameter gradients, the option is off or creation failed
    if (params && plan->opt[PIVP_OPT_SIDE_STREAM]) plan->lane.create();
    const SideLane* const lane = params && plan->lane.live() ? &plan->lane : nullptr;
    RC(apply_main_prio(plan, s));
    int gb;
    {   // Timesteps per ConvLSTM weight-gradient launch (PIVP_OPT_WGRAD_BATCH overrides, 1..wg_cap).  fp32: 1 (batches arrive in bursts and
        // overlap the sweep worse: 29.9 / 30.3 ms for 1 / 2, profiles/r02).  bf16 mode: as many as the rings hold -- its 25-tap kernel
        // fetches every operand tile once per 32 x 64 output slice, and what a block pays per launch (205 KB of atomics, the first tile's
        // latency) is amortised over the batch (csrc/wgrad_bf16.hip).
        const int e = plan->opt[PIVP_OPT_WGRAD_BATCH];
        gb = e ? e : (md.wgrad_batches() ? plan->wg_cap : 1);
        if (gb < 1) gb = 1;
        if (gb > plan->wg_cap) gb = plan->wg_cap;
    }
    // from here on the plan is read only: what the sweep mutates is the Sweep's (a fresh one per call: no batch of an earlier sweep is open in it)
    const long long slab_bytes = plan->nslabs > 1 ? ((long long)plan->slabs[1].cat7 - (long long)plan->slabs[0].cat7) * 4 : 0;
    Sweep sweep{*plan, s, lane, params, gb, slab_bytes, md};
    // the norms' partial parameter gradients start from zero every sweep; the enc convs' partial planes are STORED by each layer's first launch of the
    // sweep (WgradDesc::part_overwrite; 240 MB of planes at B = 32: a memset of them would cost what the weight gradients do)
    if (params && hipMemsetAsync(ws + g.ln_ppart[0], 0, g.ln_ppart_floats * 4, s) != hipSuccess) return PIVP_ERR_LAUNCH;
    if (plan->det && g.det_stp_acc &&      // STP's integer d prev accumulator starts at zero (each launch's finish clears what it used)
        hipMemsetAsync(ws + g.det_stp_acc, 0, (size_t)B * 3 * c.height * c.width * 8, s) != hipSuccess) return PIVP_ERR_LAUNCH;
    // d loss / d gen_states[t] for every t (zero before ctx-1), later accumulated with the state recurrence
    if (hipMemsetAsync(ws + g.dstate, 0, (size_t)T * B * c.state_dim * 4, s) != hipSuccess) return PIVP_ERR_LAUNCH;
    // (gen_states[t] against states[t + 1], t = ctx-1 .. T-2: contiguous in t, one launch; likewise the frames' loss terms below -- 16 launches per sweep before)
    // (without the plan's own loss, pivp_plan_set_sweep_mode: the memset above is the state seed, a zero fill the frames')
    if (own_loss)
        RC(scaled_diff(gen_states + (size_t)(ctx - 1) * B * c.state_dim, states + (size_t)ctx * B * c.state_dim, ws + g.dstate + (size_t)(ctx - 1) * B * c.state_dim,
                       (long)(T - ctx) * B * c.state_dim, sscale, 0, s));
    // d loss / d gen[t], t = ctx-1 .. T-2 (gen[t] is compared with images[t + 1]); the sweep adds the feed-back terms of step t + 1 into frame t in place
    if (own_loss)
        RC(scaled_diff(gen_images + (size_t)(ctx - 1) * fr, images + (size_t)ctx * fr, ws + g.go + (size_t)(ctx - 1) * fr, (long)(T - ctx) * (long)fr, fscale, 0, s));
    else if (hipMemsetAsync(ws + g.go + (size_t)(ctx - 1) * fr, 0, (size_t)(T - ctx) * fr * 4, s) != hipSuccess) return PIVP_ERR_LAUNCH;
    // ... plus the caller's own d loss / d gen (pivp_plan_set_frame_grad): everything downstream of g.go is indifferent to where the seed came from
    if (plan->frame_seed) RC(frame_seed_add(ws + g.go + (size_t)(ctx - 1) * fr, plan->frame_seed, (long)(T - ctx) * (long)fr, s));
    // weights are constant during the sweep: the transposed packs for the data gradients, all twelve in one launch (7 + 5 launches before round 5)
    {
        WeightPrepJob jobs[12];
        int n = 0;
        for (int i = 0; i < 7; ++i)
            jobs[n++] = WeightPrepJob{0, P(plan, plan->i_lstm_w[i]), ws + g.wt_lstm[i], 25, kLstm[i].cx + kLstm[i].C, 4 * kLstm[i].C, 1};
        for (int k = 4; k >= 0; --k)      // (enc1, enc2, enc4, enc5, enc6)
            jobs[n++] = WeightPrepJob{0, P(plan, plan->i_enc_w[kEnc[k].layer]), ws + g.wt_enc[kEnc[k].layer], 9, kEnc[k].c, kEnc[k].c, 0};
        RC(weight_prep_batch(jobs, n, s));
    }
    if (md.precision == Operand::BF16) {      // bf16 mode: the ConvLSTM data gradients run on one-plane bf16 packs of those: one launch
        WeightPrepJob jobs[7];
        for (int i = 0; i < 7; ++i) {
            const int cin = kLstm[i].cx + kLstm[i].C;
            jobs[i] = WeightPrepJob{1, ws + g.wt_lstm[i], ws + g.wtb_lstm[i], 4 * kLstm[i].C, cin, conv5x5_bf16_rows(cin), 0};
        }
        RC(weight_prep_batch(jobs, 7, s));
    } else if (md.packs())        // split modes: the hi / lo pair, the three pieces or the fp16 pieces (their own pack kernels, per layer)
        for (int i = 0; i < 7; ++i) {
            const int cin = kLstm[i].cx + kLstm[i].C;
            RC(pack_lstm_bf16(ws + g.wt_lstm[i], reinterpret_cast<unsigned short*>(ws + g.wtb_lstm[i]), 4 * kLstm[i].C, cin, s, md.precision,
                              conv5x5_bf16_rows(cin), 1));
        }
    if (plan->sg_seed) {      // the seed's c segments start every cell's d c (its h segments are read in place by the first visited step's gate backward)
        float* dcs[7];
        for (int i = 0; i < 7; ++i) dcs[i] = ws + g.dc[i];
        RC(state_grad_scatter(c, plan->sg_seed, dcs, s));
    }
    bool has_go = false;
    int eq_next = 0;      // the enc dY ring slot of step t + 1 (unused at t = T - 2)
    for (int t = T - 2; t >= 0; --t) {
        float* go = ws + g.go + (size_t)t * fr;
        float* go_prev = t >= 1 ? ws + g.go + (size_t)(t - 1) * fr : nullptr;
        const bool last_step = t == T - 2;
        if (last_step) has_go = true;                                            // d gen[T-2] comes from the loss only
        const bool prev_has_grad = (t >= ctx) && !gt_select;                // feed-self: prev = gen[t-1] is differentiable (TM:664-666)
        // d gen[t-1] holds its loss term (if it has one: t - 1 >= ctx - 1, which prev_has_grad implies); this step's composite / enc0 backward add the feed-back term
        const bool next_loss = (t - 1) >= ctx - 1 && t >= 1;
        const float* prev = step_input(plan, t, images, gt_select, gen_images, fr);
        const float* st_prev = t == 0 ? states : gen_states + (size_t)(t - 1) * B * c.state_dim;
        // the ConvLSTM weight gradients: batches of wg_batch timesteps (sweep_schedule.h)
        const BatchSlot wg = batch_slot(T, t, sweep.wg_batch);
        // (1 / 2 / 4 timesteps per launch instead of the rings' 8, r05_c23: config 3 11.63 / 11.24 / 11.22 ms against 11.10, fp32 train 28.08 / 27.90 / 27.67 against 27.41)
        const BatchSlot eg = batch_slot(T, t, plan->eg_cap);      // the stride-2 3x3 layers' weight gradients: as many timesteps per launch as their rings hold, every mode
        const StepSlots ss{wg.batch & 1, wg.slot, wg.flush, eg.batch & 1, eg.slot, eg.flush, eq_next};
        RC(sweep.step(StepIn{t, prev, prev_has_grad && has_go, actions + (size_t)t * B * c.action_dim, st_prev, has_go, go, go_prev, last_step, ss}));
        eq_next = ss.eg_ring * plan->eg_cap + ss.eg_slot;
        has_go = next_loss || (prev_has_grad && has_go);
    }
    return PIVP_OK;      // the side stream is joined by the caller, pivp_rollout_backward, on every path
}

// d loss / d state_in <- the cells' d c (contiguous) and the h columns of their input gradients (rows of C floats at stride cx + C, cx floats in): ONE launch
int pivp::state_grad_gather(const pivp_config_t& c, const float* const dc[7], const float* const din[7], float* d_state_in, hipStream_t s) {
    StateRowSeg seg[STATE_SEGMENTS];
    for (int i = 0; i < 7; ++i) {
        const MapSize m = lstm_map(c, i);
        const long long rows = (long long)c.batch * m.H * m.W;
        const int C = kLstm[i].C, cx = kLstm[i].cx;
        seg[2 * i] = StateRowSeg{dc[i], d_state_in + state_seg_offset(c, 2 * i), rows, C, C, C};
        seg[2 * i + 1] = StateRowSeg{din[i] + cx, d_state_in + state_seg_offset(c, 2 * i + 1), rows, C, cx + C, C};
    }
    return state_rows_copy(seg, STATE_SEGMENTS, s);
}
// the seed's seven c segments -> the cells' d c buffers: the same kernel the other way, ONE launch
int pivp::state_grad_scatter(const pivp_config_t& c, const float* d_state_out, float* const dc[7], hipStream_t s) {
    StateRowSeg seg[7];
    for (int i = 0; i < 7; ++i) {
        const MapSize m = lstm_map(c, i);
        seg[i] = StateRowSeg{d_state_out + state_seg_offset(c, 2 * i), dc[i], (long long)c.batch * m.H * m.W, kLstm[i].C, kLstm[i].C, kLstm[i].C};
    }
    return state_rows_copy(seg, 7, s);
}
static bool state_grad_cfg_ok(const pivp_config_t* cfg) { return cfg && cfg->batch >= 1 && frame_size_ok(*cfg); }
extern "C" int pivp_state_grad_gather(const pivp_config_t* cfg, const float* const dc[7], const float* const din[7], float* d_state_in, void* stream) {
    if (!state_grad_cfg_ok(cfg) || !dc || !din || !d_state_in || (reinterpret_cast<uintptr_t>(d_state_in) & 3)) return PIVP_ERR_BADARG;
    for (int i = 0; i < 7; ++i)
        if (!dc[i] || !din[i] || ((reinterpret_cast<uintptr_t>(dc[i]) | reinterpret_cast<uintptr_t>(din[i])) & 3)) return PIVP_ERR_BADARG;
    return state_grad_gather(*cfg, dc, din, d_state_in, (hipStream_t)stream);
}
extern "C" int pivp_state_grad_scatter(const pivp_config_t* cfg, const float* d_state_out, float* const dc[7], void* stream) {
    if (!state_grad_cfg_ok(cfg) || !dc || !d_state_out || (reinterpret_cast<uintptr_t>(d_state_out) & 3)) return PIVP_ERR_BADARG;
    for (int i = 0; i < 7; ++i)
        if (!dc[i] || (reinterpret_cast<uintptr_t>(dc[i]) & 3)) return PIVP_ERR_BADARG;
    return state_grad_scatter(*cfg, d_state_out, dc, (hipStream_t)stream);
}
