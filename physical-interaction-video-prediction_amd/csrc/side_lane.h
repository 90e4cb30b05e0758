// The backward sweep's second stream and every fork / join event on it.
// Weight gradients feed nothing but the optimizer: they run on a lower-priority stream next to the sweep's critical path (SideFork, pivp_kernels.h),
// one slot per layer whose weight gradient runs there.  A plan owns one lane, created by its first sweep that forms parameter gradients;
// PIVP_OPT_SIDE_STREAM = 0 keeps everything on the caller's stream.
// (A second side stream for the odd slots, round 3: fp32 no change, bf16 12.25 -> 12.05 ms, but with two processes on one GPU the step went from
// 65 ms to 78 SECONDS -- the hardware queues oversubscribe.  One stream.)
#pragma once
#include "pivp_kernels.h"

namespace pivp {

// The numbering is part of the interface: the gradient groups (kGroupSlots, pivp_plan_group_wait) are written in it.
enum : int {
    SLOT_LSTM = 0,        // + i: ConvLSTM cell i, seven of them
    SLOT_ENC = 7,         // + k: the stride-2 3x3 layers in kEnc order (enc6, enc5, enc4, enc2, enc1)
    SLOT_ENC0_W = 12,     // enc0's weight gradient
    SLOT_HEAD = 13,       // the motion head's Linear (cdna_kernels / stp_input)
    NSLOT = 14
};
// A slot has two events of each kind.  Ring slots pick by the ring their dY lives in (the cells: the dG ring, the stride-2 layers: the dY ring of
// Grads::cat6), the other two by timestep parity (their dY buffers e0raw / dv are double-buffered by it).
constexpr bool slot_is_ring(int slot) { return slot < SLOT_ENC0_W; }
// the stride-2 layer (kEnc index) a slot stands for, -1 for every other slot
constexpr int slot_enc_layer(int slot) { return slot >= SLOT_ENC && slot < SLOT_ENC0_W ? slot - SLOT_ENC : -1; }

struct SideLane {
    hipStream_t stream = nullptr;
    bool failed = false;      // the stream or an event could not be created: this plan's sweeps run on one stream
    hipEvent_t ready[NSLOT][2] = {}, done[NSLOT][2] = {};

    bool live() const { return stream != nullptr; }
    // the stream (lowest priority: the critical path wins the CUs it asks for) and its events, once; a failure is remembered, not reported
    void create() {
        if (failed || stream) return;
        int least = 0, greatest = 0;
        if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) least = 0;
        bool ok = hipStreamCreateWithPriority(&stream, hipStreamNonBlocking, least) == hipSuccess;
        if (!ok) stream = nullptr;
        for (int i = 0; i < NSLOT && ok; ++i)
            for (int r = 0; r < 2 && ok; ++r)
                ok = hipEventCreateWithFlags(&ready[i][r], hipEventDisableTiming) == hipSuccess &&
                     hipEventCreateWithFlags(&done[i][r], hipEventDisableTiming) == hipSuccess;
        if (!ok) {      // never leave `stream` set beside null events: back to "no side stream"
            destroy();
            failed = true;
            (void)hipGetLastError();
        }
    }
    // back to "never created"
    void destroy() {
        for (int i = 0; i < NSLOT; ++i)
            for (int r = 0; r < 2; ++r) {
                if (ready[i][r]) { (void)hipEventDestroy(ready[i][r]); ready[i][r] = nullptr; }
                if (done[i][r]) { (void)hipEventDestroy(done[i][r]); done[i][r] = nullptr; }
            }
        if (stream) { (void)hipStreamDestroy(stream); stream = nullptr; }
    }
    // the host waits for the lane (a sweep that failed half-way may have left weight-gradient kernels in flight)
    void sync() const { if (stream) (void)hipStreamSynchronize(stream); }

    SideFork fork(int slot, int r) const { return SideFork{stream, ready[slot][r], done[slot][r]}; }
    int record_done(int slot, int r) const { return hipEventRecord(done[slot][r], stream) == hipSuccess ? PIVP_OK : PIVP_ERR_LAUNCH; }
    // `s` waits for what the lane last recorded there (never recorded: returns at once).  NB: a null hipStream_t is the legacy default stream, a
    // perfectly good stream to wait on -- never a "no stream" marker.
    int wait_done(int slot, int r, hipStream_t s) const { return hipStreamWaitEvent(s, done[slot][r], 0) == hipSuccess ? PIVP_OK : PIVP_ERR_LAUNCH; }
    int wait_slot(int slot, hipStream_t s) const {
        const int rc = wait_done(slot, 0, s);
        return rc != PIVP_OK ? rc : wait_done(slot, 1, s);
    }
    int join_all(hipStream_t s) const {
        for (int i = 0; i < NSLOT; ++i) { const int rc = wait_slot(i, s); if (rc != PIVP_OK) return rc; }
        return PIVP_OK;
    }
};

}  // namespace pivp
