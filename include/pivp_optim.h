/* Guarded optimizer step: entry points of libpivp_hip.so that look at the flat gradient buffer before Adam consumes it, beside the model's C ABI
 * of pivp_hip.h (same conventions: int status PIVP_OK / PIVP_ERR_*, PIVP_ERR_BADARG with nothing launched, caller-owned device memory,
 * stream-ordered, no synchronisation, no allocation).  Bound by `_lib.OPTIM_SIGNATURES`; the ABI version of pivp_hip.h covers this header too.
 *
 * The flat gradient g[n] (Model._flat_grads) is a row of SEGMENTS, one per parameter tensor, padding included: segment s is
 * g[seg_end[s-1] .. seg_end[s]) with seg_end[-1] = 0.  Ends ascend; every end but the last is a multiple of 64 elements, the last equals n (any
 * n >= 1).  Each segment belongs to one of `ngroups` gradient groups (PIVP_GRAD_GROUPS of pivp_hip.h), seg_group[s] in [0, ngroups).
 * Both tables live in DEVICE memory and are trusted: validating them would take a copy and a synchronisation.  Whoever builds them (optimizer.py)
 * answers for them; a table that breaks the rules above makes the kernels read outside g or the workspace. */
#ifndef PIVP_OPTIM_H
#define PIVP_OPTIM_H

#ifdef __cplusplus
extern "C" {
#endif

#define PIVP_OPTIM_MAX_SEGMENTS 1024      /* nseg cap of pivp_grad_stats */
#define PIVP_OPTIM_STATS_HEAD 3           /* floats in front of the group norms: norm, rate, nonfinite */

/* Bytes of the workspace pivp_grad_stats needs for a buffer of n floats in nseg segments: one double per 64-element granule and one per
 * segment.  PIVP_ERR_BADARG (-1) for n < 1 or nseg outside 1 .. PIVP_OPTIM_MAX_SEGMENTS. */
long long pivp_grad_stats_ws_bytes(long long n, int nseg);

/* L2 norms of gscale * g per segment, per group and over the whole buffer, the clipping rate and the non-finite flag, reading g ONCE.
 *   g [n] fp32, 16-byte aligned.  seg_end [nseg] (long long), seg_group [nseg] (int): device memory, see above.
 *   ws: pivp_grad_stats_ws_bytes(n, nseg) bytes of device memory, 8-byte aligned; scratch, overwritten by every call.
 *   stats [3 + ngroups + nseg] fp32, every element written:
 *     stats[0] norm = sqrt(sum_i (gscale * g_i)^2) over the whole buffer,
 *     stats[1] rate = (float)(threshold / norm) where that quotient is < 1, else 1.0f  (Chainer's GradientClipping: rate = threshold / norm;
 *              if rate < 1: grad *= rate).  A zero norm, a NaN norm and threshold <= 0 (no clipping) give 1; an infinite norm gives 0, as the rule does,
 *     stats[2] nonfinite = 1.0f if the sum of squares is not finite (some g_i is NaN or +-inf), else 0.0f,
 *     stats[3 + k] the norm of group k (0 for a group without segments),  stats[3 + ngroups + s] the norm of segment s.
 * Products, squares and sums are fp64 and each result is rounded once to fp32 (a norm above FLT_MAX becomes +inf there; rate and nonfinite are
 * formed from the fp64 value, so finite gradients of any magnitude never raise the flag).  No atomics.  The order of every sum is a function of
 * (n, seg_end, seg_group) alone -- not of the grid, the timing or the device: 64-element granules by a fixed 16-lane tree, a segment's granules by a
 * fixed strided sum and tree, segments into groups and groups into the total in ascending order -- so the same bytes give the same bits.  A
 * non-finite element makes exactly its segment's, its group's and the total norm non-finite.
 * Three launches.  PIVP_ERR_BADARG: a null pointer, g not 16-byte or ws not 8-byte aligned, n < 1, nseg outside 1 .. PIVP_OPTIM_MAX_SEGMENTS,
 * ngroups outside 1 .. PIVP_GRAD_GROUPS, gscale not finite. */
int pivp_grad_stats(const float* g, long long n, const long long* seg_end, const int* seg_group, int nseg, int ngroups, double gscale,
                    double threshold, void* ws, float* stats, void* stream);

/* pivp_adam_step with the gradient read as gk = (g * gscale) * rate, rate = stats[1] of a pivp_grad_stats call earlier on the same stream
 * (rate == 1.0f gives pivp_adam_step's bits).  lr_t, the betas and eps are the host's, as there.
 * skip_nonfinite = 1 and stats[2] != 0: no thread writes p, m or v, and ONE thread adds 1 to *skipped (a device int the caller zeroes once; a
 * plain load / add / store, no atomic -- calls on one stream are ordered).  skip_nonfinite = 0: the step is applied whatever g holds (Chainer's
 * behaviour: a NaN reaches every parameter it touches); `skipped` is not read and may be null.
 * One launch.  PIVP_ERR_BADARG: a null p / g / m / v / stats, a null `skipped` with skip_nonfinite = 1, n < 1, skip_nonfinite not 0 or 1. */
int pivp_adam_step_guarded(float* p, const float* g, float* m, float* v, long long n, double lr_t, double beta1, double beta2, double eps,
                           double gscale, const float* stats, int skip_nonfinite, int* skipped, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PIVP_OPTIM_H */
