/* Data feed of the training loop: entry points of libpivp_hip.so that move data sets and batches, beside the model's C ABI of pivp_hip.h (same
 * conventions: int status PIVP_OK / PIVP_ERR_*, caller-owned device memory, stream-ordered, no synchronisation).  Bound by `_lib.DATA_SIGNATURES`;
 * the ABI version of pivp_hip.h covers this header too. */
#ifndef PIVP_DATA_H
#define PIVP_DATA_H

#ifdef __cplusplus
extern "C" {
#endif

/* One training batch out of a data set that lives on the device, in ONE launch (the host feed of train_model.py:51-71, `concat_examples`, as a
 * gather).
 *   frames  [N][T][H][W][3], as the per-sequence .npy files lie: float32 (frames_u8 = 0) or uint8 levels (frames_u8 = 1), level k standing for k / 255.
 *   actions, states [N][T][5] fp32.   index [B]: sequence numbers in DEVICE memory, each in [0, N); repeats and any order are fine.  The kernel
 *   trusts them: the caller validates.
 *   out_images [T][B][3][H][W], out_actions / out_states [T][B][5] fp32: out[t][b] = in[index[b]][t], the frames turned from HWC to planar.
 * Bit-exact: float32 storage is a permuted copy; a uint8 level k becomes the correctly rounded fp32 quotient (float)k / 255.0f, i.e.
 * np.float32(k) / np.float32(255).  Every offset into `frames` is 64-bit.  Any H, W >= 1: sizes that leave a frame or plane base off 16 bytes
 * (H*W % 16 for uint8, H*W % 4 for float32) or unaligned pointers take element-wise accesses, the others 16-B loads and stores.
 * frames_u8 0 or 1; B, N, T, H, W >= 1; H*W*3 < 2^31; every pointer non-null; anything else: PIVP_ERR_BADARG, nothing launched.  One launch,
 * stream-ordered, no synchronisation, no allocation, no atomics. */
int pivp_gather_batch(const void* frames, int frames_u8, const float* actions, const float* states, const int* index, int B,
                      long long N, int T, int H, int W, float* out_images, float* out_actions, float* out_states, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PIVP_DATA_H */
