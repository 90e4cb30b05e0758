// Which launch form a plain convolution takes: the decisions of igemm_conv (igemm_f32.hip), igemm_small (igemm_small.hip) and conv_enc0
// (small_kernels.hip) as pure functions of integers.  The launchers switch on the result, pivp_conv_form / pivp_conv_enc0_form
// (include/pivp_conv_forms.h) export it, and tests/test_conv_forms_host.py compiles this header alone: it includes nothing, HIP least of all.
#pragma once

namespace pivp {

// (the values are the PIVP_CONV_FORM_* codes of include/pivp_conv_forms.h: pivp_c_api.hip asserts it)
enum class ConvForm : int {
    DeconvTile = 1,     // all four output parities per block (deconv_tile.hip)
    LongKDgrad = 2,     // a long-K data gradient: tile and K split by dgrad_choice's cost model (igemm_f32.hip)
    Small1 = 11, Small2 = 12, Small3 = 13,      // igemm_small_kernel<1 | 2 | 3>: 32-anchor tiles, that many 32-column tiles per block
    // igemm_f32_kernel<WM, WN, NTB, false>: block tile 32 WM rows x 32 NTB columns
    F32_128x32 = 21, F32_128x64 = 22, F32_128x96 = 23, F32_128x128 = 24, F32_64x64 = 25, F32_64x128 = 26, F32_32x128 = 27,
};
enum class Enc0Form : int { Rows = 1, Generic = 2 };      // conv_enc0_rows_kernel / conv_enc0_kernel (PIVP_ENC0_FORM_*)

// igemm_small's column tiles per block: the widest column block that still leaves >= 4 blocks per CU (enc4: 1 tile 14.2 us vs 2 tiles 15.3;
// enc5: 3 tiles 23.8 vs 1 tile 25.7; enc6: 2 tiles 39.5 vs 1 tile 44.9).  M anchors, nt = N / 32 column tiles, nphase 1 or 4 (transposed).
inline int small_ntb(int M, int nt, int nphase) {
    const int mblk = (M + 31) / 32;
    if (nt % 3 == 0 && (long)mblk * (nt / 3) * nphase >= 1024) return 3;
    if (nt % 2 == 0 && (long)mblk * (nt / 2) * nphase >= 1024) return 2;
    return 1;
}

// The all-parities tile kernel's maps: 8 x 16 input patches, unless the grid would be tiny.
inline bool deconv_tile_map(int cout, int B, int Hin, int Win) {
    return Hin % 8 == 0 && Win % 16 == 0 && (long)B * (Hin / 8) * (Win / 16) * (cout / 32) >= 16;
}

// Plain conv / transposed conv: pick the block tile that fills the 256 CUs.  Blocks = (M/BM) * (N/BN) * phases.
// deconv: the transposed 3x3 stride-2 conv (four phases over the M = B * Hin * Win input anchors); else a ksize x ksize conv with M anchors (M < 0: the
// 3x3 stride-2 conv's, B * Hin/2 * Win/2).  cin = c0 + c1 input channels, cout output columns, both multiples of 32.
// aligned: ldo % 4 == 0 and 16-byte aligned output and bias rows (what igemm_small needs).  long_k_dgrad: dgrad_choice took the descriptor.
inline ConvForm conv_form(int deconv, int cin, int cout, int B, int Hin, int Win, int aligned, int long_k_dgrad, int ksize = 3, int M = -1) {
    const int nt = cout / 32, nphase = deconv ? 4 : 1;
    if (deconv && deconv_tile_map(cout, B, Hin, Win)) return ConvForm::DeconvTile;
    if (M < 0) M = deconv ? B * Hin * Win : B * (Hin / 2) * (Win / 2);
    const long full = (long)((M + 127) / 128) * nphase;   // blocks with BM = 128 and the whole N in one block
    if (long_k_dgrad) return ConvForm::LongKDgrad;
    // Short K (the 3x3 stride-2 convs and the transposed convs: 2..18 chunks) or too few big tiles to fill the chip:
    // 32-row tiles with K split over the waves (igemm_small.hip).  Measured at B = 32 (scripts/bench_tail_ops.py):
    // enc1 15.0 -> 6.6 us, enc2 21.4 -> 9.7, enc4 19.3 -> 14.2, enc5 33.7 -> 23.8, enc6 47.6 -> 39.5.
    const long big = full * ((nt + 3) / 4);
    const int chunks = (deconv ? 4 : ksize * ksize) * (cin / 32);
    if (aligned && (big < 128 || chunks <= 40)) {
        const int ntb = small_ntb(M, nt, nphase);
        return ntb == 3 ? ConvForm::Small3 : ntb == 2 ? ConvForm::Small2 : ConvForm::Small1;
    }
    if (nt > 4) {                                             // wide outputs: several column blocks
        if (nt % 4 == 0) return full * (nt / 4) >= 256 ? ConvForm::F32_128x128 : ConvForm::F32_64x128;
        if (nt % 3 == 0) return ConvForm::F32_128x96;
        if (nt % 2 == 0) return full * (nt / 2) >= 256 ? ConvForm::F32_128x64 : ConvForm::F32_64x64;
        return ConvForm::F32_128x32;
    }
    if (full >= 256) return nt == 1 ? ConvForm::F32_128x32 : nt == 2 ? ConvForm::F32_128x64 : nt == 3 ? ConvForm::F32_128x96 : ConvForm::F32_128x128;
    if (nt == 4 && full * 2 < 256) return ConvForm::F32_32x128;   // BM 32
    if (nt == 4) return ConvForm::F32_64x128;                      // BM 64
    if (nt == 2 && full * 2 >= 128) return ConvForm::F32_64x64;    // BM 64
    return ConvForm::F32_128x32;                                   // BN 32: N/32 column blocks
}

// enc0 (5x5 stride 2 on the 3-channel frame): the row kernel owns 64 output pixels = whole output rows of a W/2 in {8, 16, 32, 64} map and stages its
// (2 rows + 3) x (W + 3) x 3 patch with E0_PR patch rows per thread and channel; every other frame takes the element-per-thread kernel.
constexpr int E0_PR = 4;
inline Enc0Form enc0_form(int B, int H, int W, int weights_aligned) {
    (void)B;
    const int H2 = H / 2, W2 = W / 2;
    if ((W2 == 8 || W2 == 16 || W2 == 32 || W2 == 64) && H2 % (64 / W2) == 0 && weights_aligned) {
        const int rows = 64 / W2, R = 2 * rows + 3;
        if (W + 3 <= 256 && R <= E0_PR * (256 / (W + 3))) return Enc0Form::Rows;
    }
    return Enc0Form::Generic;
}

}  // namespace pivp
