// Training batch from a device-resident data set in ONE launch (pivp_gather_batch): B sequences picked by index out of frames stored as the .npy
// files hold them, [N][T][H][W][3] (float32, or uint8 levels k standing for k / 255), become the time-major planar batch Model.__call__ takes,
// images [T][B][3][H][W], with actions / states [N][T][5] -> [T][B][5] riding in the same grid.
//   A block owns a band of BG_PX pixels of one (timestep, sequence) frame.  The band's source is ONE contiguous run of 3 * BG_PX elements: it is read
//   with 16-B loads, lane after lane, and laid into LDS as it comes.  Thread l then takes pixels 4l .. 4l+3 back out -- 12 consecutive elements: three
//   ds_read_b128 at a 48-B lane stride (float32; every 16-lane group of that instruction covers the 64 banks once) or three dwords at a 3-dword lane
//   stride (uint8; conflict-free) -- and stores one float4 per colour plane.  Plain stores: the line stays in the XCD's L2 for the model's first kernels.
//   Frames whose size does not keep every frame and plane base on 16 bytes (H*W % 16 for uint8, H*W % 4 for float32, or an unaligned pointer) take
//   the element-wise form of the same band: same LDS image, 1-, 4-byte accesses.
//   Bits: float32 storage is copied; uint8 level k becomes (float)k / 255.0f, the correctly rounded IEEE quotient (hipcc's default for fp32 division;
//   k / 255 is never subnormal) = np.float32(k) / np.float32(255).  No atomics, every output element written once.
//   The last blocks of the grid copy the actions and states, one element of each per thread.
//   Every offset into `frames` is 64-bit (the stored set may exceed 4 GiB); index[] is trusted (the host layer validates it).
#include <type_traits>

#include "pivp_kernels.h"

namespace pivp {

constexpr int BG_NT = 256;
constexpr int BG_PX = 4 * BG_NT;                  // pixels per band: four per thread, 12 KB (float32) / 3 KB (uint8) of LDS

typedef unsigned bg_u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float bg_value(float v) { return v; }
__device__ __forceinline__ float bg_value(unsigned char k) { return (float)k / 255.0f; }

template <bool U8, bool VEC>
__global__ __launch_bounds__(BG_NT) void gather_batch_kernel(const void* __restrict__ frames, const float* __restrict__ actions,
                                                             const float* __restrict__ states, const int* __restrict__ index, int B, int T, int HW,
                                                             int bands, int frame_blocks, float* __restrict__ out_images,
                                                             float* __restrict__ out_actions, float* __restrict__ out_states) {
    using S = typename std::conditional<U8, unsigned char, float>::type;
    __shared__ __attribute__((aligned(16))) S lds[3 * BG_PX];
    const int tid = threadIdx.x;
    if ((int)blockIdx.x >= frame_blocks) {        // the riders: out[t][b][d] = in[index[b]][t][d]
        const int i = ((int)blockIdx.x - frame_blocks) * BG_NT + tid;
        if (i < T * B * 5) {
            const int tb = i / 5, d = i - tb * 5, t = tb / B, b = tb - t * B;
            const size_t src = ((size_t)index[b] * T + t) * 5 + d;
            out_actions[i] = actions[src];
            out_states[i] = states[src];
        }
        return;
    }
    const int f = (int)blockIdx.x / bands, k = (int)blockIdx.x - f * bands;      // f = t * B + b
    const int t = f / B, b = f - t * B;
    const int p0 = k * BG_PX, np = HW - p0 < BG_PX ? HW - p0 : BG_PX;
    const S* __restrict__ src = static_cast<const S*>(frames) + ((size_t)index[b] * T + t) * ((size_t)HW * 3) + (size_t)p0 * 3;
    float* __restrict__ dst = out_images + (size_t)f * 3 * HW + p0;

    if constexpr (VEC) {
        float e[12];                              // pixels 4 tid .. 4 tid + 3 as they are stored: e[3 j + c]
        if constexpr (U8) {                       // np % 16 == 0: the band is np * 3 / 16 whole 16-B pieces (at most 192)
            if (tid < np * 3 / 16) reinterpret_cast<bg_u32x4*>(lds)[tid] = reinterpret_cast<const bg_u32x4*>(src)[tid];
            __syncthreads();
            if (4 * tid >= np) return;
            const unsigned* w = reinterpret_cast<const unsigned*>(lds) + 3 * tid;
            const unsigned w0 = w[0], w1 = w[1], w2 = w[2];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                e[i] = bg_value((unsigned char)(w0 >> (8 * i)));
                e[4 + i] = bg_value((unsigned char)(w1 >> (8 * i)));
                e[8 + i] = bg_value((unsigned char)(w2 >> (8 * i)));
            }
        } else {                                  // np % 4 == 0: np * 3 / 4 float4 (at most 768, three per thread), all loads in flight before the LDS stores
            const int nq = np * 3 / 4;
            f32x4 r[3];
#pragma unroll
            for (int u = 0; u < 3; ++u)
                if (tid + u * BG_NT < nq) r[u] = reinterpret_cast<const f32x4*>(src)[tid + u * BG_NT];
#pragma unroll
            for (int u = 0; u < 3; ++u)
                if (tid + u * BG_NT < nq) reinterpret_cast<f32x4*>(lds)[tid + u * BG_NT] = r[u];
            __syncthreads();
            if (4 * tid >= np) return;
#pragma unroll
            for (int u = 0; u < 3; ++u) {
                const f32x4 q = reinterpret_cast<const f32x4*>(lds)[3 * tid + u];
#pragma unroll
                for (int i = 0; i < 4; ++i) e[4 * u + i] = q[i];
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const f32x4 q = {e[c], e[3 + c], e[6 + c], e[9 + c]};
            *reinterpret_cast<f32x4*>(dst + (size_t)c * HW + 4 * tid) = q;
        }
    } else {
        for (int i = tid; i < np * 3; i += BG_NT) lds[i] = src[i];
        __syncthreads();
        for (int p = tid; p < np; p += BG_NT) {
#pragma unroll
            for (int c = 0; c < 3; ++c) dst[(size_t)c * HW + p] = bg_value(lds[3 * p + c]);
        }
    }
}

int gather_batch(const void* frames, int frames_u8, const float* actions, const float* states, const int* index, int B, long long N, int T, int H,
                 int W, float* out_images, float* out_actions, float* out_states, hipStream_t s) {
    PIVP_CHECK_ARG(frames && actions && states && index && out_images && out_actions && out_states);
    PIVP_CHECK_ARG(B >= 1 && N >= 1 && T >= 1 && H >= 1 && W >= 1 && (frames_u8 == 0 || frames_u8 == 1));
    const long long HW = (long long)H * W;
    PIVP_CHECK_ARG(HW * 3 < (1ll << 31));
    const long long bands = (HW + BG_PX - 1) / BG_PX, frame_blocks = (long long)T * B * bands, riders = ((long long)T * B * 5 + BG_NT - 1) / BG_NT;
    PIVP_CHECK_ARG(frame_blocks + riders < (1ll << 31) && (long long)T * B * 5 < (1ll << 31));
    // 16-B accesses need every frame, band and plane to start on 16 bytes: bands start at multiples of 1,024 pixels, so the frame size decides
    const bool aligned = ((reinterpret_cast<uintptr_t>(frames) | reinterpret_cast<uintptr_t>(out_images)) & 15) == 0;
    const bool vec = aligned && HW % (frames_u8 ? 16 : 4) == 0;
    const dim3 grid((unsigned)(frame_blocks + riders)), block(BG_NT);
#define PIVP_BG_LAUNCH(U8_, VEC_)                                                                                                            \
    hipLaunchKernelGGL((gather_batch_kernel<U8_, VEC_>), grid, block, 0, s, frames, actions, states, index, B, T, (int)HW, (int)bands,       \
                       (int)frame_blocks, out_images, out_actions, out_states)
    if (frames_u8) { if (vec) PIVP_BG_LAUNCH(true, true); else PIVP_BG_LAUNCH(true, false); }
    else { if (vec) PIVP_BG_LAUNCH(false, true); else PIVP_BG_LAUNCH(false, false); }
#undef PIVP_BG_LAUNCH
    return PIVP_LAUNCH_STATUS();
}

}  // namespace pivp
