// The plan (Model.__init__ / reset_state / __call__ of the reference, TM:484-764, and the backward pass that Chainer's autograd performs under
// optimizer.update, TM:950, sequenced in native code on one HIP stream): its layer tables and types, shared by plan_setup.hip (create, setters, layout,
// taps), plan_forward.hip (the rollouts) and plan_backward.hip (the sweep).  Internal: nothing here is part of the C ABI but the name `pivp_plan`.
#pragma once
#include <string.h>
#include <string>
#include <vector>

#include "../../include/pivp_hip.h"
#include "../../include/pivp_loss.h"
#include "../../include/pivp_input_grad.h"
#include "../../include/pivp_state.h"
#include "../../include/pivp_state_grad.h"
#include "pivp_host.h"

#pragma GCC visibility push(hidden)      // internal names: none of them joins the library's exports
namespace pivp {

// ---- the layer tables: every per-layer size of the plan comes from here ----
struct MapSize { int H, W; };
inline MapSize level_map(const pivp_config_t& c, int level) { return {c.height / level, c.width / level}; }   // pyramid level: 1 = the frame, 2 -> H/2, 4 -> H/4, 8 -> H/8
struct LstmSpec { const char* name; int cx; int C; int level; };
inline const LstmSpec kLstm[7] = {
    {"lstm1", 32, 32, 2}, {"lstm2", 32, 32, 2}, {"lstm3", 32, 64, 4}, {"lstm4", 64, 64, 4},
    {"lstm5", 64, 128, 8}, {"lstm6", 128, 64, 4}, {"lstm7", 96, 32, 2}};
inline MapSize lstm_map(const pivp_config_t& c, int i) { return level_map(c, kLstm[i].level); }   // cell i's (H, W)
// The recurrent state as one buffer (include/pivp_state.h): segment g = 2 i is cell i's c, 2 i + 1 its h; floats per sample, and where the segment
// starts in the state of a batch c.batch
static_assert(STATE_SEGMENTS == PIVP_STATE_SEGMENTS && STATE_SEGMENTS == 2 * 7, "c and h of the seven cells");
inline long long state_seg_floats(const pivp_config_t& c, int g) { const MapSize m = lstm_map(c, g / 2); return (long long)m.H * m.W * kLstm[g / 2].C; }
inline size_t state_seg_offset(const pivp_config_t& c, int g) {
    long long at = 0;
    for (int k = 0; k < g; ++k) at += state_seg_floats(c, k);
    return (size_t)at * c.batch;
}
// The five stride-2 3x3 layers in the order of their side-stream slots 7..11 and of Grads::wg_part: enc6, enc5, enc4 (transposed: anchors = their INPUT maps),
// enc2, enc1 (convs).  c: channels in = out; ldx / ldo: pixel strides of the forward input / output (enc1 writes into cat6); ldy: of dY in the backward sweep
// (a ring slot of its own, or the x columns of the next cell's input gradient); level: of the input map.
struct EncSpec { int mode, layer, c, ldx, ldo, ldy, level; };
inline const EncSpec kEnc[5] = {{1, 6, 64, 64, 64, 64, 2}, {1, 5, 96, 96, 96, 128, 4}, {1, 4, 128, 128, 128, 192, 8}, {0, 2, 64, 64, 64, 64, 4}, {0, 1, 32, 32, 96, 96, 2}};
// parameter sizes: enc0 5x5 on 3 channels, enc3 1x1 on e2 (+ the smeared action / state), the others 3x3 with as many channels in as out
inline const int kEncB[7] = {32, 32, 64, 64, 128, 96, 64};
// (c: a plan's cfg, whose action_dim / state_dim pivp_plan_create has resolved to 1 .. 16)
inline int smear_width(const pivp_config_t& c) { return c.action_dim + c.state_dim; }      // the [action, state] vector of TM:556-567
inline long long enc_w_numel(const pivp_config_t& c, int i) {
    return i == 0 ? 75 * 32 : i == 3 ? (64 + (c.use_state ? smear_width(c) : 0)) * 64LL : 9LL * kEncB[i] * kEncB[i];
}
// elements per sample of the nine LayerNorms: norm_enc0, hidden1..hidden7 (behind cell j - 1), norm_enc6
inline long long ln_numel(const pivp_config_t& c, int j) {
    if (j == 0) return 32LL * (c.height / 2) * (c.width / 2);
    if (j == 8) return 64LL * c.height * c.width;
    const MapSize m = lstm_map(c, j - 1);
    return (long long)kLstm[j - 1].C * m.H * m.W;
}

// ---- the precision mode: everything the plan derives from it ----
static_assert((int)Operand::F32 == PIVP_PRECISION_F32 && (int)Operand::BF16 == PIVP_PRECISION_BF16 && (int)Operand::BF16X3 == PIVP_PRECISION_BF16X3 &&
              (int)Operand::BF16X6 == PIVP_PRECISION_BF16X6 && (int)Operand::FP16X3 == PIVP_PRECISION_FP16X3, "Operand is the PIVP_PRECISION_* code");
struct Modes {
    Operand precision;      // the mode = the form of the ConvLSTM forward's operands
    // the ConvLSTM forward runs on weight packs (of the form `precision`)
    bool packs() const { return precision != Operand::F32; }
    // The ConvLSTM data gradient on an H x W map at batch B: the forward's form where its tiles serve the map -- packed_tiles_serve (pivp_kernels.h), the
    // predicate by which run_convlstm sends a cell of the L2-direct modes to the fp32 kernel, so the forward and the sweep agree cell by cell (an 8-wide map with
    // an odd batch, a height that is no multiple of 8: the fp32 kernels take the cell).  The other modes are refused at pivp_plan_set_precision on such a map.
    Operand dgrad(int H, int W, int B) const { return operand_l2_direct(precision) && !packed_tiles_serve(H, W, B) ? Operand::F32 : precision; }
    // ... and the weight gradient of a batch of timesteps: the split mode has no form of its own and stays fp32
    Operand wgrad(int H, int W, int B) const { return precision == Operand::BF16X3 ? Operand::F32 : dgrad(H, W, B); }
    // ... which those forms batch: BF16 as many timesteps per launch as the rings hold, the L2-direct forms two; fp32 none
    bool wgrad_batches() const { return precision == Operand::BF16 || operand_l2_direct(precision); }
    // a transposed conv.  has_wabs: the layer keeps its weights' absmax partials (enc5 / enc6: pivp_plan::o_wabs), which the fp16-piece form needs -- a layer
    // without them (enc4) stays fp32 in that mode, as every layer does in the three-piece mode (the tile kernel has no such form)
    Operand deconv(bool has_wabs) const { return precision == Operand::BF16X6 || (operand_needs_scale(precision) && !has_wabs) ? Operand::F32 : precision; }
    // the stride-2 convs' data gradient (enc1's is a transposed conv the tile kernel takes): bf16 operands in that mode only
    Operand enc_dgrad() const { return precision == Operand::BF16 ? Operand::BF16 : Operand::F32; }
};

struct ParamInfo { std::string name; long long numel; const float* ptr; float* grad; int group; };

// LayerNorm partial slots per sample: the ln_stats slices of the largest map (64 channels at full resolution) or the tiles
// of the producers that write partials themselves (enc6 through igemm_small: HW/4 anchors / 32 x 2 column blocks x 4 parities)
inline int ln_partial_cap(int HW) {
    const int a = ln_stats_slices(64 * HW), b = (HW / 4 / 32 + 1) * 2 * 4;
    return a > b ? a : b;
}

// Deterministic sweeps: the fp32 slot form of the ConvLSTM weight gradients with this many blocks per XCD whatever the device reports (WgradDesc::slot_j;
// two per CU on a 256-CU MI355X), so that the order of its sums follows the problem shape alone -- not the CU count of a partition mode
constexpr int DET_SLOT_J = 64;

// Per-timestep activations (offsets in floats from the workspace base).  Two rolling slabs for inference, T-1 slabs
// when keep_activations (BPTT needs every step).
struct Slab {
    size_t cat7, n1, n2, cat6, n3, n4, e2, e3, n5, e4, e5, e6;   // NHWC feature maps (cat7 = [hidden7|enc0], cat6 = [hidden6|enc1])
    size_t h[7], c[7];                                           // ConvLSTM states
    size_t e0raw, e6raw;                                         // LayerNorm inputs of norm_enc0 / norm_enc6
    size_t gates[7];                                             // gate activations [M][4C] (training)
    size_t lnstat;                                               // [9][B][2] mean, rstd (training)
    size_t logits, enc7, layer0, kerns, vpre, theta;             // head tensors of the step
    size_t prevsel;                                              // scheduled-sampling input frame of the step
};

struct Grads {   // gradient workspace (single copy, reused by every timestep of the backward sweep)
    size_t cat7, n2, n4, n5, e6;
    size_t e0raw[2], dv[2];   // dY tensors the side stream's weight gradients read, by timestep parity: a step rewrites the buffer the weight gradients of
                              // TWO steps ago read, so the main stream never waits for the previous step's (round 5)
    // The dY tensors of the five stride-2 3x3 layers live in RINGS like the ConvLSTMs' dG: 2 rings x eg_cap timesteps, one weight-gradient launch per
    // batch (wgrad3x3s2.hip).  enc6: d e6raw; enc2: d e2; enc1: columns 64.. of d cat6; enc5 / enc4: the x columns of lstm7's / lstm6's input gradient,
    // din[6] / din[5] -- so those two hold ring slots as well (the other cells' din: two buffers by timestep parity).  *_sz: floats per slot.
    size_t cat6, e2, e6raw, cat6_sz, e2_sz, e6raw_sz;
    size_t din[7], din_sz[7], dc[7];
    size_t dG[7], go, dmk, dz, dkpart, dstate, lnpart;   // dG: gate pre-activation gradients per ConvLSTM: 2 rings x wg_cap timesteps (batched weight gradients)
                                                             // go: d loss / d gen[t] for every t ([T-1] frames: the loss terms of all of them come from ONE launch)
    size_t wt_lstm[7], wt_enc[7];   // re-packed (transposed) weights for the data gradients, rebuilt once per backward
    size_t ln_ppart[9], ln_ppart_floats;   // per-norm partial parameter gradients (ln_backward's param_part), one contiguous region
    size_t wg_part[5], wg_part_floats;   // per-block partial weight gradients of enc6, enc5, enc4, enc2, enc1 (WgradDesc::part), one contiguous region
    size_t wtb_lstm[7];             // ... and their bf16 packs (bf16 precision mode)
    size_t dg_absmax;               // fp16-piece data gradients: the partial maxima of the dG in front of the launch (absmax_partials; stream-ordered, one buffer)
    // deterministic sweeps only (pivp_plan_set_deterministic; 0 otherwise): the ConvLSTM weight gradients' segment slots (wgrad5x5p, one region per cell,
    // summed once per sweep), and the per-block rows of the output side's small gradients (heads_bwd, the CDNA generator's bias, enc3 + state
    // predictor, enc0, the STP regressor), summed in order behind each launch; STP's d prev as exact 64-bit integer sums (det_stp_acc)
    size_t lstm_part[7], det_heads, det_dv, det_enc3, det_enc0, det_stp, det_stp_acc;
};

// What the last rollout of a plan was: what pivp_rollout_backward, pivp_get_tap and pivp_plan_set_state_grad may assume about the slabs.  A rollout resets it
// to {} in front of its first launch and assigns it whole behind its last, so one that failed half-way leaves "no rollout".
struct LastRollout {
    int steps;                  // timesteps whose slabs are whole (0: none)
    bool sched;                 // scheduled sampling was on (frames detached, TM:669-670)
    bool predict;               // it was pivp_rollout_predict: nothing to back-propagate
    bool carried;               // it started from a registered state: the sweep's t = 0 forms without h do not describe it
    const float* state_in;      // pivp_rollout_forward: the state it read (null: zeros) -- the sweep's t = 0 reads it again
    bool state_lost;            // ... which that rollout overwrote with its own final state (state_in == state_out)
};

// The forms a timestep's launches take as far as cfg, the precision mode and the options decide them: computed once (step_form, below) where any of the
// three is assigned, read by Rollout::step (plan_forward.hip) and pivp_get_tap.  The other half of each choice is made per launch: a norm is applied
// inside its consumer only if the producer's launcher reported LayerNorm partials (LnPartOut::nparts > 0), and frame_head runs only if enc6's did.
enum class MotionHead { None, Rider, InHead, Separate };   // DNA has none; the finisher rides behind enc5's tiles; inside frame_head; cdna_kernels / stp_params
enum class Output { FrameHead, Separate };                 // one launch (frame_head.hip) / heads_1x1 + the motion head + composite
struct StepForm {
    bool keep;               // a launch that applies a norm also writes the tensor and its (mean, rstd): training plans
    bool norm_inside[9];     // norm j (hidden1..hidden7; 8 = norm_enc6) is applied by its consumer -- 1, 3: lstm2 / lstm4; 2, 4: enc1 / enc2; 6, 7: enc5 / enc6;
                             // 8: heads_1x1, where Output::Separate runs.  (norm_enc0 and hidden5 keep their launches.)
    bool enc3_in_enc2;       // enc3 + the state predictor in enc2's epilogue (its fmaf chains are written for 5 / 5: other widths take the separate launch)
    bool enc4_partials;      // enc4 shares its grid with the partial sums of the motion head's Linear
    MotionHead motion;
    Output output;
};

// pivp_plan_set_profiling: an event pair around every ConvLSTM launch of a rollout, which reaches it through Rollout::prof.  tag: cell + 8 for a
// first-step launch without the h half of K
struct StepProfile {
    bool on = false; std::vector<hipEvent_t> ev; std::vector<int> layer; size_t used = 0;
    bool room() const { return used + 2 <= ev.size(); }
    void begin(hipStream_t s) { if (room()) (void)hipEventRecord(ev[used], s); }
    void end(int tag, hipStream_t s) { if (room()) { (void)hipEventRecord(ev[used + 1], s); layer[used / 2] = tag; used += 2; } }
};

}  // namespace pivp
#pragma GCC visibility pop

struct pivp_plan {
    // ---- fixed at pivp_plan_create ----
    pivp_config_t cfg;
    std::vector<pivp::ParamInfo> params;      // (ptr / grad: pivp_plan_set_param / pivp_plan_set_grad)
    int i_enc_w[7], i_enc_b[7], i_lstm_w[7], i_lstm_b[7];
    int i_ln_g[9], i_ln_b[9];   // order: norm_enc0, hidden1..hidden7, norm_enc6
    int i_masks_w, i_masks_b, i_cs_w, i_cs_b, i_enc7_w, i_enc7_b;
    int i_head_w, i_head_b, i_head2_w, i_head2_b;
    int H2, W2, H4, W4, H8, W8, NP, NE, K5;
    // ---- fixed before the workspace is bound: the switches the layout follows, and the layout (plan_layout) ----
    pivp::Modes mode{pivp::Operand::F32};   // pivp_plan_set_precision
    int det = 0;                      // pivp_plan_set_deterministic: fixed-order forms of every sum of the sweep (no float atomics)
    // pivp_plan_set_option (include/pivp_hip.h), by PIVP_OPT_*: SIDE_STREAM; FINISH_RIDER: the motion head's finisher rides behind enc5's tiles (0: inside
    // frame_head, as rounds 4-5); FUSE_ENC3, inference: enc3 + state predictor in enc2's epilogue (0: their own launch); LN_FOLD_TRAIN, training: the norms of
    // hidden2 / hidden4 applied (and written) by enc1 / enc2's launches (0: ln_apply launches); WGRAD_BATCH: timesteps per ConvLSTM weight-gradient launch
    // (tests, measurements), whatever the precision mode; 0 = the mode's own choice
    int opt[PIVP_OPT_COUNT] = {1, 1, 1, 1, 0};
    pivp::StepForm form = {};         // step_form(*this): recomputed wherever mode or opt is assigned
    int wg_cap = 1;                  // dG ring slots per ring = min(T - 2, WG_BATCH_MAX), fixed when the workspace is laid out
    int eg_cap = 1;                   // slots per enc dY ring (Grads::cat6): min(T - 2, WG_BATCH_MAX), cut to ENC_RING_BYTES_MAX
    float* ws; long long ws_floats;
    int nslabs;
    std::vector<pivp::Slab> slabs;
    pivp::Grads g;
    bool has_grads;
    size_t o_zero, o_lnpart, o_lnpart2, o_linpart, o_masks, o_losspart;   // o_lnpart2: enc6 reads hidden7's partials while writing its own
    size_t o_wabs[2];                 // precision mode FP16X3: absmax_partials of the enc5 / enc6 weights (rebuilt at the start of a rollout)
    size_t o_wbf16[7];                // bf16 packs of the ConvLSTM weights (pivp_plan_set_precision), rebuilt at the start of a rollout
    int loss_nparts;
    // ---- registered for the next calls ----
    int pack_cache = 0, packs_valid = 0;   // pivp_plan_set_pack_cache: keep the precision modes' weight packs across rollouts until pivp_plan_params_changed
    int main_prio = -1;               // pivp_plan_set_main_priority: -1 = on unless a gradient listener is registered (data parallelism), 0 / 1 = as said
    pivp_grad_group_cb grad_cb = nullptr; void* grad_cb_user = nullptr;   // gradient-group-final notifications (t = 0 sweep)
    bool group_join = true;           // pivp_plan_set_group_join
    const float* frame_seed = nullptr;   // pivp_plan_set_frame_grad: an additional d loss / d gen_images[ctx-1 .. T-2] for the sweep (null: the plan's own seed alone)
    float* in_dact = nullptr; float* in_dstate0 = nullptr;   // pivp_plan_set_input_grad: d loss / d actions [T-1][B][A] and d loss / d states[0] [B][S] (null: not wanted)
    int sweep_mode = 3;               // pivp_plan_set_sweep_mode: PIVP_SWEEP_PARAMS | PIVP_SWEEP_BUILTIN_LOSS (include/pivp_input_grad.h)
    // pivp_plan_set_rollout_state (include/pivp_state.h): where the next rollouts read their initial (c, h) of the seven cells and leave their final ones
    // (null: zeros / nowhere), and how many leading steps pivp_rollout_predict feeds from context_images (0: cfg.context_frames)
    const float* state_in = nullptr; float* state_out = nullptr; int observed = 0;
    // pivp_plan_set_state_grad (include/pivp_state_grad.h): the sweep serves a rollout that started from a state (sg_enable), is seeded with d / d (its final
    // state) (sg_seed) and leaves d loss / d (its initial state) (sg_dstate_in); null / 0: none of it
    int sg_enable = 0; const float* sg_seed = nullptr; float* sg_dstate_in = nullptr;
    // ---- written by the rollouts: packs_valid and last by their shared prologue / epilogue, prof through Rollout::prof.  (What a rollout passes to its
    // own steps is the Rollout's, plan_forward.hip) ----
    pivp::LastRollout last = {};
    pivp::StepProfile prof;
    // ---- the weight gradients' stream and its events (side_lane.h): a sweep reads it, only create / the destructor change it.  (What a sweep mutates
    // is its own: Sweep, plan_backward.hip) ----
    pivp::SideLane lane;
    ~pivp_plan() {
        lane.sync();
        for (hipEvent_t e : prof.ev) (void)hipEventDestroy(e);
        lane.destroy();
    }
};

#pragma GCC visibility push(hidden)
namespace pivp {

inline const float* P(const pivp_plan* p, int idx) { return p->params[idx].ptr; }
inline float* G(const pivp_plan* p, int idx) { return p->params[idx].grad; }

// the frame sizes every entry point takes: three stride-2 levels under 5x5 ConvLSTMs.  (Each caller adds its own condition on batch and seq_len.)
inline bool frame_size_ok(const pivp_config_t& c) { return c.height >= 16 && c.width >= 16 && c.height % 8 == 0 && c.width % 8 == 0; }
// The accepted domain (include/pivp_hip.h, pivp_plan_create), from the kernels' own limits, so that nothing is refused half-way through a rollout or a sweep:
// ... of the forward: the compositing kernels stage a padded frame row per 256 threads (W + 4 <= 256) within their LDS budget, and the CDNA motion head's
// finishers give each of the 25 * num_masks kernel taps a thread of one 256-thread block (num_masks <= 10).  Asked by pivp_plan_create.
inline bool plan_serves_forward(const pivp_config_t& c) {
    return frame_size_ok(c) && composite_serves(c.height, c.width, c.num_masks, c.model_type) &&
           (c.model_type != PIVP_MODEL_CDNA || cdna_kernels_serves(c.num_masks));
}
// ... of the backward sweep, narrower than the forward's: the composite backward takes 1 .. 10 masks for CDNA and 2 .. 10 for STP (its mask loop has no
// one-mask form, and eleven masks pass the forward alone), and its tile's staging must fit in LDS -- every mask count up to 128-wide frames, fewer masks on
// wider ones; det: a deterministic sweep's integer d prev window (STP) is twice as large.  Asked at the entry of pivp_rollout_backward, in front of its
// first launch.
inline bool plan_serves_backward(const pivp_config_t& c, bool det) {
    return plan_serves_forward(c) && composite_bwd_serves(c.model_type, c.height, c.width, c.num_masks, det);
}

// The static half of a timestep's choices (StepForm), each predicate with the arguments and thresholds its launch site had.
inline StepForm step_form(const pivp_plan& p) {
    const pivp_config_t& c = p.cfg;
    const int B = c.batch, H = c.height, W = c.width;
    const bool train = c.keep_activations != 0, fold_opt = p.opt[PIVP_OPT_LN_FOLD_TRAIN] || !train;
    const Modes& md = p.mode;
    StepForm f = {};
    f.keep = train;
    // lstm2 / lstm4: inference rollouts in the L2-direct modes, with enough tiles
    f.norm_inside[1] = !train && convlstm_ln_in_ok(md.precision, 32, 32, 32, B, p.H2, p.W2) && (long)B * (p.H2 / 8) * (p.W2 / 16) >= 128;
    f.norm_inside[3] = !train && convlstm_ln_in_ok(md.precision, 64, 64, 64, B, p.H4, p.W4) && (long)B * (p.H4 / 8) * (p.W4 / 16) >= 64;
    f.norm_inside[2] = fold_opt && conv3x3s2_ln_ok(32, 32, B, p.H2, p.W2);      // enc1 / enc2: training plans by PIVP_OPT_LN_FOLD_TRAIN
    f.norm_inside[4] = fold_opt && conv3x3s2_ln_ok(64, 64, B, p.H4, p.W4);
    f.enc3_in_enc2 = !train && f.norm_inside[4] && p.opt[PIVP_OPT_FUSE_ENC3] && (p.H8 * p.W8) % 32 == 0 &&
                     c.action_dim == 5 && c.state_dim == 5;
    // enc5 / enc6: only while the norm is a launch-bound 5-us kernel (<= 6 MB of hidden tensor: 64 x 64 frames at B = 32): the consumer's column blocks
    // each stage the patch and its gamma / beta again, which at config 5's 128 x 128 costs more than one bandwidth-bound ln_apply pass
    // (B = 32, T = 20: rollout 65.5 -> 65.9 ms with the fold, so it is not taken there).
    auto fold_small = [](long long floats) { return floats * 4 <= 6LL << 20; };
    f.norm_inside[6] = fold_small((long long)B * 64 * p.H4 * p.W4) && deconv3x3s2_ln_ok(64, 32, 96, B, p.H4, p.W4);
    f.norm_inside[7] = fold_small((long long)B * 32 * p.H2 * p.W2) && deconv3x3s2_ln_ok(32, 32, 64, B, p.H2, p.W2);
    f.norm_inside[8] = (H * W) % 64 == 0;
    // the output side: frame_head where it beats the separate kernels, finishing the Linear's partial sums itself where it can -- which an fp32 enc4 then forms
    const bool fh = frame_head_pays(c.model_type, B, H, W, c.num_masks);
    const bool fh_fin = fh && c.model_type != PIVP_MODEL_DNA && frame_head_finishes(p.K5);
    f.output = fh ? Output::FrameHead : Output::Separate;
    f.enc4_partials = fh_fin && md.deconv(false) == Operand::F32;
    f.motion = c.model_type == PIVP_MODEL_DNA ? MotionHead::None
             : !fh_fin ? MotionHead::Separate
             : f.norm_inside[6] && p.opt[PIVP_OPT_FINISH_RIDER] ? MotionHead::Rider : MotionHead::InHead;
    return f;
}

// ---- what crosses the units ----
void plan_layout(pivp_plan* p);                              // plan_setup.hip: the workspace carve
size_t state_bytes(const pivp_config_t& c);                  // ... bytes of the recurrent state at batch c.batch
bool ranges_overlap(const void* a, const void* b, size_t bytes);
// plan_forward.hip: the frame fed to step t; ctx: the leading steps fed from `images` (0: cfg.context_frames)
const float* step_input(const pivp_plan* plan, int t, const float* images, const unsigned char* gt_select, const float* gen_images, size_t fr, int ctx = 0);
int state_grad_gather(const pivp_config_t& c, const float* const dc[7], const float* const din[7], float* d_state_in, hipStream_t s);             // plan_backward.hip
int state_grad_scatter(const pivp_config_t& c, const float* d_state_out, float* const dc[7], hipStream_t s);

#define RC(call) do { int rc_ = (call); if (rc_ != PIVP_OK) return rc_; } while (0)

}  // namespace pivp
#pragma GCC visibility pop
