// The plan's set-up side (plan.h): create / destroy, the parameter table, every setter and getter, the workspace layout, the state entries, profiling
// and taps.  Nothing here launches a timestep.
#include "plan.h"

using namespace pivp;

// group of a parameter = position of its layer in the backward sweep of one timestep (include/pivp_hip.h, PIVP_GRAD_GROUPS)
static int grad_group_of(const std::string& n) {
    auto starts = [&](const char* p) { return n.rfind(p, 0) == 0; };
    if (starts("masks/") || starts("model/") || starts("norm_enc6/") || starts("enc6/")) return 0;
    if (starts("hidden7/") || starts("lstm7/")) return 1;
    if (starts("enc5/") || starts("hidden6/") || starts("lstm6/")) return 2;
    if (starts("enc4/") || starts("hidden5/") || starts("lstm5/")) return 3;
    if (starts("enc3/") || starts("current_state/") || starts("enc2/") || starts("hidden4/") || starts("lstm4/") ||
        starts("hidden3/") || starts("lstm3/")) return 4;
    return 5;   // enc1, hidden2, lstm2, hidden1, lstm1, norm_enc0, enc0
}

// ConvLSTM weight gradients can be taken over a batch of up to this many timesteps in ONE launch (the reduction runs over pixels and
// timesteps alike; WgradDesc::tcount): a quarter of the block epilogues and grid ramps.  Measured at B = 32 it does not pay: alone
// it is worth 0.4 ms of a 35.6 ms train step, and next to the side stream it LOSES 0.7 ms (34.1 vs 33.4 ms) because the weight
// gradients then arrive in bursts instead of filling the gaps of every step.  So the default is one timestep per launch
// (PIVP_OPT_WGRAD_BATCH 0 in fp32 = 1), the dG rings then simply double-buffer; the batched path stays for larger per-GPU batches and is tested
// (tests/test_gpu_train.py).  Timestep 0 is always its own batch (its h_{-1} = 0 half is skipped).
constexpr size_t ENC_RING_BYTES_MAX = (size_t)2 << 30;   // the five stride-2 3x3 layers' dY rings together (pivp_plan::eg_cap is cut to fit)
constexpr int WG_BATCH_MAX = 8;   // most timesteps one ConvLSTM weight-gradient launch can take (dG ring slots per ring: pivp_plan::wg_cap <= this)

// ---- workspace carve (offsets in floats, 256-B aligned).  Runs at pivp_plan_create and again from pivp_plan_set_precision while no
// workspace is bound, and from pivp_plan_set_option(PIVP_OPT_WGRAD_BATCH): the ConvLSTM dG rings hold wg_cap timesteps per ring, and only the bf16 mode
// (or that option) batches its weight gradients -- an fp32 plan double-buffers with ONE slot per ring instead of 8 (2.5 GB less at 128 x 128, B = 32, T = 20). ----
// dG ring slots per ring: timesteps t = T-2 .. 1 batch (t = 0, no h input, goes alone), as many slots as a launch may take timesteps.
// (fp16-piece / three-piece weight gradients: TWO timesteps per launch on half the CUs -- measured grid, profiles/r04/fp16x3_train_wgrad_batch_slots.txt:
// 8 per launch on every CU, what the bf16 mode does, leaves all of that work to the end of the sweep: 16.85 ms against 16.34)
static int wg_cap_of(int T, const Modes& m, int e /* PIVP_OPT_WGRAD_BATCH */) {
    const int want = e ? e : m.precision == Operand::BF16 ? WG_BATCH_MAX : m.wgrad_batches() ? 2 : 1;
    int cap = T - 2 < 1 ? 1 : (T - 2 > WG_BATCH_MAX ? WG_BATCH_MAX : T - 2);
    if (want < cap) cap = want < 1 ? 1 : want;
    return cap;
}
void pivp::plan_layout(pivp_plan* p) {
    const pivp_config_t* cfg = &p->cfg;
    const int H = cfg->height, W = cfg->width, B = cfg->batch, T = cfg->seq_len;
    size_t off = 0;
    auto carve = [&](size_t n) { size_t o = off; off += (n + 63) / 64 * 64; return o; };
    const size_t HW = (size_t)H * W, HW2 = (size_t)p->H2 * p->W2, HW4 = (size_t)p->H4 * p->W4, HW8 = (size_t)p->H8 * p->W8;
    size_t hsz[7];      // floats per sample of a cell's h / c
    for (int i = 0; i < 7; ++i) { const MapSize m = lstm_map(*cfg, i); hsz[i] = (size_t)m.H * m.W * kLstm[i].C; }
    const bool train = cfg->keep_activations != 0;
    p->o_zero = carve((size_t)B * HW2 * 32);
    p->o_lnpart = carve((size_t)B * ln_partial_cap((int)HW) * 4);
    p->o_lnpart2 = carve((size_t)B * ln_partial_cap((int)HW) * 4);
    p->o_linpart = carve((size_t)motion_partials_floats(B, p->K5));      // [B][K slices][256] + the tail frame_head_kernel's finisher may read
    p->o_masks = carve((size_t)B * p->NP * HW);
    p->loss_nparts = loss_partials_count((int)(B * 3 * HW));
    p->o_losspart = carve((size_t)T * p->loss_nparts);
    p->o_wabs[0] = carve(128); p->o_wabs[1] = carve(128);
    for (int i = 0; i < 7; ++i)       // 2-byte elements in a float-counted workspace
        p->o_wbf16[i] = carve(lstm_bf16_weight_elems(kLstm[i].cx + kLstm[i].C, 4 * kLstm[i].C) * 3 / 2 + 64);   // room for the three planes of PIVP_PRECISION_BF16X6
    p->nslabs = train ? T - 1 : 2;
    p->wg_cap = wg_cap_of(T, p->mode, p->opt[PIVP_OPT_WGRAD_BATCH]);
    p->eg_cap = T - 2 < 1 ? 1 : (T - 2 > WG_BATCH_MAX ? WG_BATCH_MAX : T - 2);      // whatever the precision mode: every mode batches these
    if (train) {
        // ... bounded by bytes: a ring slot holds the dY of all five layers (60 MB at B = 32 on 64 x 64 frames, 240 MB on 128 x 128), and there are
        // 2 x eg_cap of them.  ENC_RING_BYTES_MAX keeps config 2 at 8 timesteps per launch (0.97 GB) and gives config 5 four (1.9 GB instead of
        // 3.9 GB; 4 against 8 per launch measured 11.22 against 11.10 ms on config 3, profiles/r05/NOTES.md).  include/pivp_hip.h documents the growth.
        const size_t r64 = 63;
        const size_t slot_floats = (((size_t)B * HW4 * 96 + r64) & ~r64) + (((size_t)B * HW8 * 64 + r64) & ~r64) + (((size_t)B * HW * 64 + r64) & ~r64) +
                                   (((size_t)B * HW4 * (kLstm[5].cx + kLstm[5].C) + r64) & ~r64) + (((size_t)B * HW2 * (kLstm[6].cx + kLstm[6].C) + r64) & ~r64);
        while (p->eg_cap > 1 && (size_t)2 * p->eg_cap * slot_floats * 4 > ENC_RING_BYTES_MAX) --p->eg_cap;
    }
    p->slabs.resize(p->nslabs);
    for (int s = 0; s < p->nslabs; ++s) {
        Slab& S = p->slabs[s];
        S.cat7 = carve(B * HW2 * 64); S.n1 = carve(B * HW2 * 32); S.n2 = carve(B * HW2 * 32);
        S.cat6 = carve(B * HW4 * 96); S.n3 = carve(B * HW4 * 64); S.n4 = carve(B * HW4 * 64);
        S.e2 = carve(B * HW8 * 64); S.e3 = carve(B * HW8 * 64); S.n5 = carve(B * HW8 * 128);
        S.e4 = carve(B * HW4 * 128); S.e5 = carve(B * HW2 * 96); S.e6 = carve(B * HW * 64);
        for (int i = 0; i < 7; ++i) { S.h[i] = carve(B * hsz[i]); S.c[i] = carve(B * hsz[i]); }
        S.e0raw = carve(B * HW2 * 32); S.e6raw = carve(B * HW * 64);
        for (int i = 0; i < 7; ++i) S.gates[i] = train ? carve(B * hsz[i] * 4) : 0;
        S.lnstat = carve((size_t)9 * B * 2);
        S.logits = carve((size_t)B * p->NP * HW); S.enc7 = carve((size_t)B * p->NE * HW); S.layer0 = carve((size_t)B * 3 * HW);
        S.kerns = carve((size_t)B * 25 * cfg->num_masks); S.vpre = carve((size_t)B * 256); S.theta = carve((size_t)B * 6);
        S.prevsel = carve((size_t)B * 3 * HW);
    }
    p->has_grads = train;
    if (p->has_grads) {
        Grads& g = p->g;
        g.cat7 = carve(B * HW2 * 64); g.n2 = carve(B * HW2 * 32); g.n4 = carve(B * HW4 * 64);
        g.n5 = carve(B * HW8 * 128); g.e6 = carve(B * HW * 64);
        for (int r = 0; r < 2; ++r) { g.e0raw[r] = carve(B * HW2 * 32); g.dv[r] = carve((size_t)B * 256); }
        const size_t nq = (size_t)2 * p->eg_cap;      // slots per enc dY ring pair
        auto slots = [&](size_t n, size_t count, size_t& sz) { sz = (n + 63) / 64 * 64; return carve(sz * count); };
        g.cat6 = slots(B * HW4 * 96, nq, g.cat6_sz); g.e2 = slots(B * HW8 * 64, nq, g.e2_sz); g.e6raw = slots(B * HW * 64, nq, g.e6raw_sz);
        for (int i = 0; i < 7; ++i) {
            const size_t M = hsz[i] / kLstm[i].C * B;
            g.dc[i] = carve(B * hsz[i]);   // (d h of a cell is never materialised: the LayerNorm backward is folded into the gate backward)
            g.din[i] = slots(M * (kLstm[i].cx + kLstm[i].C), i >= 5 ? nq : 2, g.din_sz[i]);
            g.dG[i] = carve(M * 4 * kLstm[i].C * 2 * p->wg_cap);
            g.wt_lstm[i] = carve((size_t)25 * (kLstm[i].cx + kLstm[i].C) * 4 * kLstm[i].C);
            g.wtb_lstm[i] = carve(lstm_bf16_weight_elems(4 * kLstm[i].C, conv5x5_bf16_rows(kLstm[i].cx + kLstm[i].C)) * 3 / 2 + 64);   // up to three planes
            g.wt_enc[i] = (i == 0 || i == 3) ? 0 : carve((size_t)enc_w_numel(*cfg, i));
        }
        g.dg_absmax = carve((size_t)7 * 2 * p->wg_cap * 72);     // dG's partial maxima per (cell, ring, slot): the fp16-piece gradients' scales
        for (int i = 0; i < 7; ++i) g.lstm_part[i] = 0;
        g.det_heads = g.det_dv = g.det_enc3 = g.det_enc0 = g.det_stp = g.det_stp_acc = 0;
        if (p->det) {      // (pivp_plan_set_deterministic has checked that every cell's shape is served)
            for (int i = 0; i < 7; ++i) {
                const MapSize m = lstm_map(*cfg, i);
                g.lstm_part[i] = carve((size_t)lstm_wgrad_part_floats(kLstm[i].cx, kLstm[i].C, B, m.H, m.W, 0, DET_SLOT_J));
            }
            g.det_heads = carve((size_t)heads_bwd_det_floats(B, (int)HW, p->NP, p->NE));
            g.det_dv = carve((size_t)B * 256);
            g.det_enc3 = carve((size_t)enc3_state_bwd_det_floats(B, (int)HW8, cfg->use_state, cfg->action_dim, cfg->state_dim));
            g.det_enc0 = carve((size_t)enc0_bwd_det_floats(B, H, W));
            if (cfg->model_type == PIVP_MODEL_STP) { g.det_stp = carve((size_t)B * 706); g.det_stp_acc = carve((size_t)B * 3 * HW * 2); }   // (64-bit integers)
        }
        g.go = carve((size_t)(T - 1) * B * 3 * HW);
        g.dmk = carve((size_t)B * p->NP * HW); g.dz = carve((size_t)B * p->NE * HW);
        g.dkpart = carve((size_t)B * composite_bwd_tiles(H, W) * 256);
        g.dstate = carve((size_t)T * B * cfg->state_dim);
        g.lnpart = carve((size_t)B * ln_bwd_slices((int)(64 * HW)) * 2);
        g.ln_ppart_floats = 0;
        for (int j = 0; j < 9; ++j) {
            const size_t n = (size_t)ln_bwd_param_part_floats((int)ln_numel(*cfg, j));
            g.ln_ppart[j] = carve(n);
            g.ln_ppart_floats = g.ln_ppart[j] + n - g.ln_ppart[0];
        }
        g.wg_part_floats = 0;
        for (int k = 0; k < 5; ++k) {
            const MapSize m = level_map(*cfg, kEnc[k].level);
            const size_t n = (size_t)conv_backward_part_floats(kEnc[k].mode, kEnc[k].c, kEnc[k].c, B, m.H, m.W);
            g.wg_part[k] = carve(n);
            g.wg_part_floats = g.wg_part[k] + n - g.wg_part[0];      // carve() aligns: measure the region, not the sum
        }
    }
    p->ws_floats = (long long)off;
    p->form = step_form(*p);
}

extern "C" int pivp_plan_create(const pivp_config_t* cfg, pivp_plan_t** out) {
    if (!cfg || !out) return PIVP_ERR_BADARG;
    if (cfg->batch <= 0 || cfg->seq_len < 2 || !frame_size_ok(*cfg)) return PIVP_ERR_BADARG;
    if (cfg->model_type < 0 || cfg->model_type > 2) return PIVP_ERR_BADARG;
    if (cfg->num_masks < 1 || cfg->num_masks > 11) return PIVP_ERR_BADARG;
    if (cfg->model_type == PIVP_MODEL_DNA && cfg->num_masks != 1) return PIVP_ERR_BADARG;  // TM:389-390
    if (cfg->context_frames < 1 || cfg->context_frames >= cfg->seq_len) return PIVP_ERR_BADARG;
    if (!plan_serves_forward(*cfg)) return PIVP_ERR_BADARG;      // a frame or mask count a kernel of the rollout would refuse: refused here, not at that launch
    // the widths of an action and of a robot state: 0 = the reference data's 5; the enc3 / state-predictor kernels hold both in 32 floats of LDS
    if (cfg->action_dim < 0 || cfg->action_dim > 16 || cfg->state_dim < 0 || cfg->state_dim > 16) return PIVP_ERR_BADARG;
    pivp_plan* p = new pivp_plan();
    p->cfg = *cfg;
    if (!p->cfg.action_dim) p->cfg.action_dim = 5;
    if (!p->cfg.state_dim) p->cfg.state_dim = 5;
    cfg = &p->cfg;      // (from here on the resolved widths)
    const int H = cfg->height, W = cfg->width;
    p->H2 = H / 2; p->W2 = W / 2; p->H4 = H / 4; p->W4 = W / 4; p->H8 = H / 8; p->W8 = W / 8;
    p->NP = cfg->num_masks + 1;
    p->NE = cfg->model_type == PIVP_MODEL_DNA ? 25 : 3;
    p->K5 = 128 * p->H8 * p->W8;
    p->ws = nullptr; p->ws_floats = 0;

    auto add = [&](const std::string& name, long long n) { p->params.push_back({name, n, nullptr, nullptr, grad_group_of(name)}); return (int)p->params.size() - 1; };
    for (int i = 0; i < 7; ++i) {
        p->i_enc_w[i] = add("enc" + std::to_string(i) + "/W", enc_w_numel(*cfg, i));
        p->i_enc_b[i] = add("enc" + std::to_string(i) + "/b", kEncB[i]);
    }
    for (int i = 0; i < 7; ++i) {
        const LstmSpec& L = kLstm[i];
        p->i_lstm_w[i] = add(std::string(L.name) + "/conv/W", 25LL * (L.cx + L.C) * 4 * L.C);
        p->i_lstm_b[i] = add(std::string(L.name) + "/conv/b", 4 * L.C);
    }
    const char* lnn[9] = {"norm_enc0", "hidden1", "hidden2", "hidden3", "hidden4", "hidden5", "hidden6", "hidden7", "norm_enc6"};
    for (int i = 0; i < 9; ++i) {
        p->i_ln_g[i] = add(std::string(lnn[i]) + "/norm/gamma", ln_numel(*cfg, i));
        p->i_ln_b[i] = add(std::string(lnn[i]) + "/norm/beta", ln_numel(*cfg, i));
    }
    p->i_masks_w = add("masks/W", 64LL * p->NP);
    p->i_masks_b = add("masks/b", p->NP);
    p->i_cs_w = add("current_state/W", (long long)cfg->state_dim * smear_width(*cfg));
    p->i_cs_b = add("current_state/b", cfg->state_dim);
    p->i_enc7_w = add("model/enc7/W", 64LL * p->NE);
    p->i_enc7_b = add("model/enc7/b", p->NE);
    p->i_head_w = p->i_head_b = p->i_head2_w = p->i_head2_b = -1;
    if (cfg->model_type == PIVP_MODEL_CDNA) {
        p->i_head_w = add("model/cdna_kerns/W", (long long)p->K5 * 256);
        p->i_head_b = add("model/cdna_kerns/b", 25LL * cfg->num_masks);
    } else if (cfg->model_type == PIVP_MODEL_STP) {
        p->i_head_w = add("model/stp_input/W", (long long)p->K5 * 256);
        p->i_head_b = add("model/stp_input/b", 100);
        p->i_head2_w = add("model/identity_params/W", 600);
        p->i_head2_b = add("model/identity_params/b", 6);
    }

    plan_layout(p);
    *out = p;
    return PIVP_OK;
}

extern "C" void pivp_plan_destroy(pivp_plan_t* plan) { delete plan; }
extern "C" int pivp_param_count(const pivp_plan_t* plan) { return plan ? (int)plan->params.size() : PIVP_ERR_BADARG; }
extern "C" const char* pivp_param_name(const pivp_plan_t* plan, int idx) {
    if (!plan || idx < 0 || idx >= (int)plan->params.size()) return nullptr;
    return plan->params[idx].name.c_str();
}
extern "C" long long pivp_param_numel(const pivp_plan_t* plan, int idx) {
    if (!plan || idx < 0 || idx >= (int)plan->params.size()) return PIVP_ERR_BADARG;
    return plan->params[idx].numel;
}
extern "C" int pivp_plan_set_param(pivp_plan_t* plan, int idx, const float* dptr) {
    if (!plan || idx < 0 || idx >= (int)plan->params.size() || !dptr) return PIVP_ERR_BADARG;
    plan->params[idx].ptr = dptr;
    plan->packs_valid = 0;
    return PIVP_OK;
}
extern "C" int pivp_param_group(const pivp_plan_t* plan, int idx) {
    if (!plan || idx < 0 || idx >= (int)plan->params.size()) return PIVP_ERR_BADARG;
    return plan->params[idx].group;
}
extern "C" int pivp_param_group_by_name(const char* name) { return name ? grad_group_of(name) : PIVP_ERR_BADARG; }
extern "C" int pivp_plan_set_grad_callback(pivp_plan_t* plan, pivp_grad_group_cb cb, void* user) {
    if (!plan) return PIVP_ERR_BADARG;
    plan->grad_cb = cb; plan->grad_cb_user = user;
    return PIVP_OK;
}
extern "C" int pivp_plan_set_grad(pivp_plan_t* plan, int idx, float* dptr) {
    if (!plan || idx < 0 || idx >= (int)plan->params.size() || !dptr) return PIVP_ERR_BADARG;
    plan->params[idx].grad = dptr;
    return PIVP_OK;
}
// Precision of the ConvLSTM gate convolutions (95 % of the FLOPs): PIVP_PRECISION_F32 (default), PIVP_PRECISION_BF16X3 = every fp32 operand of the
// FORWARD gate convolutions as two bf16 pieces and three MFMAs per product (fp32-grade results, everything else and the backward in fp32), or
// PIVP_PRECISION_BF16 = operands
// rounded to bf16, fp32 accumulation / gates / state (csrc/convlstm_bf16.hip), and in the backward sweep their data and weight gradients
// (csrc/convlstm_bf16.hip <NCH, false>, csrc/wgrad_bf16.hip).  Everything else stays fp32, as do the parameters, the gradients and Adam.  Refused when a layer's map does not fit the bf16 kernel's tiles (8-wide maps need an even batch).
static bool det_supported(const pivp_plan* p, Operand precision);
extern "C" int pivp_plan_set_precision(pivp_plan_t* plan, int precision_code) {
    if (!plan || precision_code < PIVP_PRECISION_F32 || precision_code > PIVP_PRECISION_FP16X3) return PIVP_ERR_BADARG;
    const Operand precision = (Operand)precision_code;
    if (plan->det && !det_supported(plan, precision)) return PIVP_ERR_BADARG;      // a deterministic plan keeps to the modes its sweep serves
    if (precision == Operand::BF16 || precision == Operand::BF16X3) {   // (the L2-direct forms: a layer their tile does not serve runs the fp32 kernel)
        for (int i = 0; i < 7; ++i) {
            const MapSize m = lstm_map(plan->cfg, i);
            IgemmDesc d;
            memset(&d, 0, sizeof(d));
            d.ksize = 5; d.pad = 2; d.in_step = 1; d.C = kLstm[i].C; d.c0 = kLstm[i].cx; d.c1 = kLstm[i].C;
            d.ld0 = 4; d.ld1 = 4; d.B = plan->cfg.batch; d.Hin = m.H; d.Win = m.W;
            if (!convlstm_bf16_ok(d)) return PIVP_ERR_BADARG;
        }
    }
    // The dG rings' depth follows the precision, so the order is set_precision -> workspace_bytes -> set_workspace (include/pivp_hip.h).  With a
    // workspace already bound the layout it was sized for stays; a mode that needs deeper rings than it has is refused, not run short.
    const Modes cand{precision};
    if (plan->ws && plan->has_grads && wg_cap_of(plan->cfg.seq_len, cand, plan->opt[PIVP_OPT_WGRAD_BATCH]) > plan->wg_cap) return PIVP_ERR_STATE;
    plan->mode = cand;
    plan->packs_valid = 0;
    if (!plan->ws) plan_layout(plan);
    else plan->form = step_form(*plan);
    return PIVP_OK;
}
// Deterministic training (include/pivp_hip.h): every sum of the forward and the backward sweep in an order fixed by the problem shape.  Served:
// precision F32, BF16 and BF16X3 (the ConvLSTM weight gradients then take the fp32 slot form, wgrad5x5p), models CDNA, STP and DNA, and shapes whose
// cells fit wgrad5x5p and whose stride-2 3x3 layers fit wgrad3x3s2 (both with their column sums: no bias_grad launch is needed) -- wgrad_fixed_order of the
// form wgrad_launch (wgrad_form.h) names, the question run_wgrad asks again in front of each of the sweep's launches.
static bool det_supported(const pivp_plan* p, Operand precision) {
    if (operand_l2_direct(precision)) return false;
    const int B = p->cfg.batch;
    for (int i = 0; i < 7; ++i) {
        const MapSize m = lstm_map(p->cfg, i);
        if (lstm_wgrad_part_floats(kLstm[i].cx, kLstm[i].C, B, m.H, m.W, 0, DET_SLOT_J) <= 0) return false;
    }
    for (const EncSpec& E : kEnc) {
        const MapSize m = level_map(p->cfg, E.level);
        if (!conv_backward_fixed_order(E.mode, E.c, E.c, B, m.H, m.W)) return false;
    }
    return true;
}
extern "C" int pivp_plan_set_deterministic(pivp_plan_t* plan, int on) {
    if (!plan) return PIVP_ERR_BADARG;
    const int want = on ? 1 : 0;
    if (want == plan->det) return PIVP_OK;
    if (want && !det_supported(plan, plan->mode.precision)) return PIVP_ERR_BADARG;
    if (plan->ws) {      // a bound workspace keeps its layout: switching on needs the slots it was sized with
        if (want && plan->has_grads && plan->g.det_heads == 0) return PIVP_ERR_STATE;
        plan->det = want;
        return PIVP_OK;
    }
    plan->det = want;
    plan_layout(plan);
    return PIVP_OK;
}
extern "C" int pivp_plan_get_deterministic(const pivp_plan_t* plan) { return plan ? plan->det : PIVP_ERR_BADARG; }
// include/pivp_hip.h: the four switches 0 / 1, the weight-gradient batch 0 .. WG_BATCH_MAX; before a workspace is bound (the batch sets the dG rings' depth)
extern "C" int pivp_plan_set_option(pivp_plan_t* plan, int option, int value) {
    if (!plan || option < 0 || option >= PIVP_OPT_COUNT) return PIVP_ERR_BADARG;
    if (value < 0 || value > (option == PIVP_OPT_WGRAD_BATCH ? WG_BATCH_MAX : 1)) return PIVP_ERR_BADARG;
    if (plan->ws) return PIVP_ERR_STATE;
    plan->opt[option] = value;
    plan_layout(plan);      // the batch sets the dG rings' depth, the switches the step's form
    return PIVP_OK;
}
extern "C" int pivp_plan_get_option(const pivp_plan_t* plan, int option) {
    return plan && option >= 0 && option < PIVP_OPT_COUNT ? plan->opt[option] : PIVP_ERR_BADARG;
}

// include/pivp_loss.h: an additional d loss / d gen_images for every later sweep (null: none -- the sweep's launches are then exactly its own)
extern "C" int pivp_plan_set_frame_grad(pivp_plan_t* plan, const float* seed) {
    if (!plan || (reinterpret_cast<uintptr_t>(seed) & 3)) return PIVP_ERR_BADARG;
    plan->frame_seed = seed;
    return PIVP_OK;
}
// include/pivp_input_grad.h: where the sweep leaves d loss / d actions and d loss / d states[0] (null: nowhere -- no launch is added), and what it computes
extern "C" int pivp_plan_set_input_grad(pivp_plan_t* plan, float* dactions, float* dstate0) {
    if (!plan || ((reinterpret_cast<uintptr_t>(dactions) | reinterpret_cast<uintptr_t>(dstate0)) & 3)) return PIVP_ERR_BADARG;
    plan->in_dact = dactions; plan->in_dstate0 = dstate0;
    return PIVP_OK;
}
// include/pivp_state.h: the recurrent state across rollouts
extern "C" int pivp_state_layout(const pivp_config_t* cfg, long long seg_floats_per_sample[PIVP_STATE_SEGMENTS], long long* floats_per_sample) {
    if (!cfg || !frame_size_ok(*cfg)) return PIVP_ERR_BADARG;
    long long total = 0;
    for (int g = 0; g < PIVP_STATE_SEGMENTS; ++g) {
        const long long n = state_seg_floats(*cfg, g);
        if (seg_floats_per_sample) seg_floats_per_sample[g] = n;
        total += n;
    }
    if (floats_per_sample) *floats_per_sample = total;
    return PIVP_OK;
}
extern "C" int pivp_plan_set_rollout_state(pivp_plan_t* plan, const float* state_in, float* state_out, int observed) {
    if (!plan || ((reinterpret_cast<uintptr_t>(state_in) | reinterpret_cast<uintptr_t>(state_out)) & 15)) return PIVP_ERR_BADARG;
    if (observed < 0 || observed > plan->cfg.seq_len - 1) return PIVP_ERR_BADARG;
    plan->state_in = state_in; plan->state_out = state_out; plan->observed = observed;
    return PIVP_OK;
}
extern "C" int pivp_plan_get_rollout_state(const pivp_plan_t* plan, const float** state_in, float** state_out, int* observed) {
    if (!plan) return PIVP_ERR_BADARG;
    if (state_in) *state_in = plan->state_in;
    if (state_out) *state_out = plan->state_out;
    if (observed) *observed = plan->observed;
    return PIVP_OK;
}
extern "C" int pivp_state_copy(const pivp_config_t* cfg, const float* src, int B_src, float* dst, int B_dst, const int* index, void* stream) {
    if (!cfg || !src || !dst || B_src < 1 || B_dst < 1 || (!index && B_src != B_dst)) return PIVP_ERR_BADARG;
    if (!frame_size_ok(*cfg)) return PIVP_ERR_BADARG;
    if ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(index)) & 3) return PIVP_ERR_BADARG;
    StateSeg seg[STATE_SEGMENTS];
    long long at = 0;      // floats per sample in front of the segment: it starts at B * at on either side
    for (int g = 0; g < STATE_SEGMENTS; ++g) {
        const long long n = state_seg_floats(*cfg, g);
        seg[g] = StateSeg{src + at * B_src, dst + at * B_dst, n};
        at += n;
    }
    return state_copy(seg, index, B_dst, (hipStream_t)stream);
}
// include/pivp_state_grad.h: gradients through the recurrent state
size_t pivp::state_bytes(const pivp_config_t& c) { return (state_seg_offset(c, STATE_SEGMENTS - 1) + (size_t)state_seg_floats(c, STATE_SEGMENTS - 1) * c.batch) * 4; }
bool pivp::ranges_overlap(const void* a, const void* b, size_t bytes) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return a && b && x < y + bytes && y < x + bytes;
}
extern "C" int pivp_plan_set_state_grad(pivp_plan_t* plan, int enable, const float* d_state_out, float* d_state_in) {
    if (!plan || (enable != 0 && enable != 1)) return PIVP_ERR_BADARG;
    if ((reinterpret_cast<uintptr_t>(d_state_out) | reinterpret_cast<uintptr_t>(d_state_in)) & 15) return PIVP_ERR_BADARG;
    if (d_state_in && !enable) return PIVP_ERR_BADARG;
    const size_t bytes = state_bytes(plan->cfg);
    if (ranges_overlap(d_state_out, d_state_in, bytes)) return PIVP_ERR_BADARG;
    if (plan->last.carried && ranges_overlap(d_state_in, plan->last.state_in, bytes)) return PIVP_ERR_BADARG;
    plan->sg_enable = enable; plan->sg_seed = d_state_out; plan->sg_dstate_in = d_state_in;
    return PIVP_OK;
}
extern "C" int pivp_plan_get_state_grad(const pivp_plan_t* plan, int* enable, const float** d_state_out, float** d_state_in) {
    if (!plan) return PIVP_ERR_BADARG;
    if (enable) *enable = plan->sg_enable;
    if (d_state_out) *d_state_out = plan->sg_seed;
    if (d_state_in) *d_state_in = plan->sg_dstate_in;
    return PIVP_OK;
}
extern "C" int pivp_plan_set_sweep_mode(pivp_plan_t* plan, int flags) {
    if (!plan || flags < 0 || flags > (PIVP_SWEEP_PARAMS | PIVP_SWEEP_BUILTIN_LOSS)) return PIVP_ERR_BADARG;
    plan->sweep_mode = flags;
    return PIVP_OK;
}
extern "C" int pivp_plan_get_sweep_mode(const pivp_plan_t* plan) { return plan ? plan->sweep_mode : PIVP_ERR_BADARG; }
// Inference with constant weights: keep the bf16 / fp16 weight packs across rollouts (on = 1) instead of rebuilding them at the start of each.  The
// caller then owes pivp_plan_params_changed after EVERY modification of a parameter tensor (optimizer step, checkpoint load, host write); set_param,
// set_precision and set_workspace invalidate by themselves.  Default off.
extern "C" int pivp_plan_set_pack_cache(pivp_plan_t* plan, int on) {
    if (!plan) return PIVP_ERR_BADARG;
    plan->pack_cache = on ? 1 : 0; plan->packs_valid = 0;
    return PIVP_OK;
}
extern "C" int pivp_plan_params_changed(pivp_plan_t* plan) {
    if (!plan) return PIVP_ERR_BADARG;
    plan->packs_valid = 0;
    return PIVP_OK;
}
extern "C" int pivp_plan_get_precision(const pivp_plan_t* plan) { return plan ? (int)plan->mode.precision : PIVP_ERR_BADARG; }
extern "C" long long pivp_plan_workspace_bytes(const pivp_plan_t* plan) { return plan ? plan->ws_floats * 4 : PIVP_ERR_BADARG; }
extern "C" int pivp_plan_set_workspace(pivp_plan_t* plan, void* dptr, long long bytes) {
    if (!plan || !dptr || bytes < plan->ws_floats * 4 || ((uintptr_t)dptr & 255)) return PIVP_ERR_BADARG;
    plan->ws = (float*)dptr;
    plan->packs_valid = 0;
    return PIVP_OK;
}
extern "C" int pivp_reset_state(pivp_plan_t* plan, void* stream) {
    if (!plan || !plan->ws) return PIVP_ERR_STATE;
    const size_t n = (size_t)plan->cfg.batch * plan->H2 * plan->W2 * 32;
    if (hipMemsetAsync(plan->ws + plan->o_zero, 0, n * 4, (hipStream_t)stream) != hipSuccess) return PIVP_ERR_LAUNCH;
    return PIVP_OK;
}

// ------------------------------------------------------------------------------------------------------------
// measurement hooks and taps
// ------------------------------------------------------------------------------------------------------------
extern "C" int pivp_plan_set_profiling(pivp_plan_t* plan, int enable) {
    if (!plan) return PIVP_ERR_BADARG;
    StepProfile& pr = plan->prof;
    if (enable && pr.ev.empty()) {
        const size_t n = (size_t)2 * 7 * (plan->cfg.seq_len - 1);
        pr.ev.resize(n);
        pr.layer.assign(n / 2, 0);
        for (size_t i = 0; i < n; ++i)
            if (hipEventCreate(&pr.ev[i]) != hipSuccess) { pr.ev.resize(i); return PIVP_ERR_LAUNCH; }
    }
    pr.on = enable != 0;
    pr.used = 0;
    return PIVP_OK;
}

extern "C" int pivp_plan_profile_read(pivp_plan_t* plan, double* ms_per_layer, int* launches_per_layer, double* flops_per_layer) {
    if (!plan || !ms_per_layer || !launches_per_layer || !flops_per_layer) return PIVP_ERR_BADARG;
    const pivp_config_t& c = plan->cfg;
    double fl_full[7], fl_first[7];
    for (int i = 0; i < 7; ++i) {
        ms_per_layer[i] = 0.0; launches_per_layer[i] = 0; flops_per_layer[i] = 0.0;
        const int lv = kLstm[i].level;
        const double M = (double)c.batch * (c.height / lv) * (c.width / lv);
        fl_full[i] = 2.0 * M * 4.0 * kLstm[i].C * 25.0 * (kLstm[i].cx + kLstm[i].C);
        fl_first[i] = 2.0 * M * 4.0 * kLstm[i].C * 25.0 * kLstm[i].cx;     // executed flops when h == 0 is skipped
    }
    StepProfile& pr = plan->prof;
    for (size_t k = 0; k + 1 < pr.used; k += 2) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, pr.ev[k], pr.ev[k + 1]) != hipSuccess) return PIVP_ERR_STATE;
        const int tag = pr.layer[k / 2];
        const int L = tag & 7;
        ms_per_layer[L] += ms; launches_per_layer[L] += 1;
        flops_per_layer[L] += (tag & 8) ? fl_first[L] : fl_full[L];   // SUM of executed flops over the launches
    }
    pr.used = 0;
    return PIVP_OK;
}

extern "C" long long pivp_get_tap(pivp_plan_t* plan, const char* name, int step, float* out, void* stream) {
    if (!plan || !name || !out || !plan->ws) return PIVP_ERR_BADARG;
    if (step < 0 || step >= plan->last.steps) return PIVP_ERR_BADARG;
    if (!plan->cfg.keep_activations && step < plan->last.steps - 2) return PIVP_ERR_STATE;
    hipStream_t s = (hipStream_t)stream;
    const pivp_config_t& c = plan->cfg;
    const int B = c.batch;
    const Slab& S = plan->slabs[step % plan->nslabs];
    float* ws = plan->ws;
    const int HW = c.height * c.width, HW2 = plan->H2 * plan->W2, HW4 = plan->H4 * plan->W4, HW8 = plan->H8 * plan->W8;
    struct T { const char* n; size_t off; int C, hw, ld; int norm = 0; };      // norm j: the tensor is hidden<j>, norm j of cell j - 1's h
    const T taps[] = {
        {"enc0", S.cat7 + 32, 32, HW2, 64}, {"enc1", S.cat6 + 64, 32, HW4, 96}, {"enc2", S.e2, 64, HW8, 64},
        {"enc3", S.e3, 64, HW8, 64}, {"enc4", S.e4, 128, HW4, 128}, {"enc5", S.e5, 96, HW2, 96}, {"enc6", S.e6, 64, HW, 64},
        {"hidden1", S.n1, 32, HW2, 32, 1}, {"hidden2", S.n2, 32, HW2, 32, 2}, {"hidden3", S.n3, 64, HW4, 64, 3},
        {"hidden4", S.n4, 64, HW4, 64, 4}, {"hidden5", S.n5, 128, HW8, 128, 5}, {"hidden6", S.cat6, 64, HW4, 96, 6},
        {"hidden7", S.cat7, 32, HW2, 64, 7},
        {"lstm1_h", S.h[0], 32, HW2, 32}, {"lstm2_h", S.h[1], 32, HW2, 32}, {"lstm3_h", S.h[2], 64, HW4, 64},
        {"lstm4_h", S.h[3], 64, HW4, 64}, {"lstm5_h", S.h[4], 128, HW8, 128}, {"lstm6_h", S.h[5], 64, HW4, 64},
        {"lstm7_h", S.h[6], 32, HW2, 32},
        {"lstm1_c", S.c[0], 32, HW2, 32}, {"lstm2_c", S.c[1], 32, HW2, 32}, {"lstm3_c", S.c[2], 64, HW4, 64},
        {"lstm4_c", S.c[3], 64, HW4, 64}, {"lstm5_c", S.c[4], 128, HW8, 128}, {"lstm6_c", S.c[5], 64, HW4, 64},
        {"lstm7_c", S.c[6], 32, HW2, 32}};
    if (strcmp(name, "enc6") == 0 && !c.keep_activations) {
        // inference does not materialise relu(norm_enc6(.)) (fused into the heads kernel): rebuild it from the raw map
        // and the saved (mean, rstd)
        int rc = ln_apply(ws + S.e6raw, ws + S.lnstat + (size_t)8 * B * 2, P(plan, plan->i_ln_g[8]), P(plan, plan->i_ln_b[8]),
                          ws + S.e6, B, 64 * HW, 64, 64, c.ln_eps, 1, s, nullptr, -1);
        if (rc != PIVP_OK) return rc;
    }
    for (const T& t : taps) {
        if (strcmp(t.n, name) == 0) {
            int rc = PIVP_OK;
            // Where the step's form (StepForm) applies a norm inside its consumer, an inference plan never wrote the tensor: rebuild it on request from the
            // raw ConvLSTM output (statistics recomputed by ln_stats: equal to the fused ones up to fp32 summation order).  Everywhere else the step wrote it.
            if (t.norm && plan->form.norm_inside[t.norm] && !plan->form.keep)
                rc = run_layernorm(ws + S.h[t.norm - 1], P(plan, plan->i_ln_g[t.norm]), P(plan, plan->i_ln_b[t.norm]), ws + t.off,
                                   ws + plan->o_lnpart, B, t.C * t.hw, t.C, t.ld, c.ln_eps, 0, s);
            if (rc != PIVP_OK) return rc;
            rc = nhwc_to_nchw(ws + t.off, out, B, t.C, t.hw, t.ld, s);
            return rc == PIVP_OK ? (long long)B * t.C * t.hw : rc;
        }
    }
    size_t off = 0, n = 0;
    if (strcmp(name, "enc7") == 0) { off = S.enc7; n = (size_t)B * plan->NE * HW; }
    else if (strcmp(name, "cdna_kerns") == 0 && c.model_type == PIVP_MODEL_CDNA) { off = S.kerns; n = (size_t)B * 25 * c.num_masks; }
    else if (strcmp(name, "stp_theta") == 0 && c.model_type == PIVP_MODEL_STP) { off = S.theta; n = (size_t)B * 6; }
    else if (strcmp(name, "masks") == 0) {
        if (step != plan->last.steps - 1) return PIVP_ERR_STATE;      // softmaxed masks exist only for the most recent step
        off = plan->o_masks; n = (size_t)B * plan->NP * HW;
    } else return PIVP_ERR_BADARG;
    if (hipMemcpyAsync(out, ws + off, n * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) return PIVP_ERR_LAUNCH;
    return (long long)n;
}
