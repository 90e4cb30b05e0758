// Which launch form a weight gradient takes, and on what grid: the decisions of igemm_wgrad (igemm_wgrad.hip), wgrad5x5p (wgrad5x5p.hip), wgrad3x3s2
// (wgrad3x3s2.hip) and wgrad5x5_bf16 (wgrad_bf16.hip) as ONE pure function of integers.  A launch, the size of its partial buffer, its reduction, the
// bias_grad launches behind it (run_wgrad) and the plan's question "is this shape served in a fixed order" all read the same WgradLaunch, so they cannot
// disagree -- a launch and a reduction on different grids give a silent wrong sum, not a refusal.  The launchers switch on the result and
// tests/test_wgrad_forms_host.py compiles this header alone: it includes nothing, HIP least of all.
#pragma once

#ifdef __HIP__
#define PIVP_WF_HD __attribute__((host)) __attribute__((device))      // (wp_range is also the slot kernel's)
#else
#define PIVP_WF_HD
#endif

namespace pivp {

enum class WgradForm : int {
    None = 0,                                  // refused: no kernel serves the shape in the operand form asked for
    // igemm_wgrad_kernel<1 | 2>: a tap, 64 input channels and 64 | 128 columns per block; atomics into dw, or the block's own plane of `part`
    Generic64 = 1, Generic128 = 2, Generic64Part = 3, Generic128Part = 4,
    Row5x5_8 = 11, Row5x5_16 = 12, Row5x5_32 = 13,                                     // wgrad5x5_kernel<SW>: the fp32 ConvLSTM kernel-row form, atomics
    Slot5x5_8x1 = 21, Slot5x5_8x2 = 22, Slot5x5_16x1 = 23, Slot5x5_16x2 = 24,         // wgrad5x5p_kernel<SW, NTW>: segment slots, no atomics
    Tile3x3s2_D2x2 = 31, Tile3x3s2_D3x3 = 32, Tile3x3s2_C1x1 = 33,                    // wgrad3x3s2_kernel: instance 1, 2 (transposed), 3 (conv); slots, no atomics
    PackedRow_8 = 41, PackedRow_16 = 42,                                               // wgrad5x5_bf16_kernel<TW>: bf16 operands, one timestep
    Packed25x4_8 = 51, Packed25x4_16 = 52,                                             // wgrad25_bf16_kernel<TW, 1, 4>: bf16, a batch of timesteps, four waves
    // wgrad25_bf16_kernel<TW, PCS>: eight waves; 1 piece (bf16), 2 (fp16 pieces), 3 (bf16 pieces)
    Packed25x8_1_8 = 61, Packed25x8_1_16 = 62, Packed25x8_2_8 = 63, Packed25x8_2_16 = 64, Packed25x8_3_8 = 65, Packed25x8_3_16 = 66,
};
constexpr bool wgrad_is_slot(WgradForm f) { return (int)f >= 21 && (int)f <= 24; }
constexpr bool wgrad_is_tile(WgradForm f) { return (int)f >= 31 && (int)f <= 33; }
// no atomics anywhere, the column sums of dy included: the launches add into partial slots and the reduction sums them in an order fixed by the shape.
// What a deterministic sweep needs of every weight gradient (pivp_plan_set_deterministic asks this of every layer; run_wgrad refuses anything else there).
constexpr bool wgrad_fixed_order(WgradForm f) { return wgrad_is_slot(f) || wgrad_is_tile(f); }

// WgradDesc's ONE-timestep geometry (pivp_kernels.h documents the fields; wgrad_shape() there fills this from a descriptor)
struct WgradShape {
    int c0, ld0, c1, ld1, cin, wcin, ldy, N;
    int B, Hx, Wx, Hy, Wy, Hg, Wg, M;
    int deconv, ksize, pad, stride;
    int ts_aligned;      // the byte strides between the timesteps of a batch are multiples of 16
};

// ---- the generic kernel ----------------------------------------------------------------------------------------------------------------------
constexpr int WG_PIX = 32;     // pixels (GEMM K) per chunk
constexpr int WG_CI = 64;      // input channels per block
// grid of the generic kernel: a function of the shape alone, so a launch, its partial buffer and its reduction agree
inline void generic_grid(const WgradShape& d, int& wg_n, int& tiles, int& nsplit) {
    wg_n = d.N <= 64 ? 64 : 128;
    const int ncb = (d.cin + WG_CI - 1) / WG_CI, nnb = (d.N + wg_n - 1) / wg_n;
    tiles = d.ksize * d.ksize * ncb * nnb;
    const int chunks = (d.M + WG_PIX - 1) / WG_PIX;      // of ONE timestep: a batched launch, a single one and the reduction must agree on the planes
    // direct path: every block ends with a tile of atomics (64 x 128), so no more pixel splits than fill the chip twice (3 blocks fit a
    // CU) and >= 8 chunks (256 pixels) per block (enc4 with 4: 63 -> 94 us, atomics); kept for the partial-sum path, where a split
    // costs 16-32 KB of traffic instead
    // (round 5, call 15: a target of 256 / 384 / 1024 blocks instead of 512 gives config 3 11.50 / 11.27 / 11.27 ms against 11.18-11.22,
    // fp32 train 28.02 against 27.85 with 256: 512 stays)
    nsplit = tiles < 1 ? 1 : (512 + tiles - 1) / tiles;      // (no tiles: a width of zero or less, which igemm_wgrad_check refuses)
    if (nsplit > chunks / 8) nsplit = chunks / 8;
    if (nsplit < 1) nsplit = 1;
}
// the generic kernel sums dy's columns on the side when the tap set qualifies: a 3x3 conv, or the transposed 3x3 s2 conv (see the kernel)
inline bool generic_bias_rides(const WgradShape& d) { return d.ksize == 3 && (!d.deconv || (d.Hy == 2 * d.Hx && d.Wy == 2 * d.Wx)); }

// ---- the fp32 kernel-row form ----------------------------------------------------------------------------------------------------------------
// wgrad5x5_kernel<SW> walks chunks of 32 consecutive pixels = 32 / SW whole image rows and takes the sample and the rows' bounds from a chunk's first pixel:
// a map narrower than a chunk must be whole chunks deep (Hg % (32 / Wg) == 0), or a chunk would run over the end of a sample and pair the next sample's dY
// rows with this one's X rows (6 x 8, 9 x 8, 9 x 16 maps: the generic kernel takes them).  The model's power-of-two maps all pass.
inline bool takes_fast_path(const WgradShape& d) {
    return !d.deconv && d.ksize == 5 && d.pad == 2 && d.stride == 1 && d.M % 32 == 0 && d.N % 64 == 0 &&
           (d.Wg == 8 || d.Wg == 16 || d.Wg % 32 == 0) && (d.Wg >= 32 || d.Hg % (32 / d.Wg) == 0) && d.Hx == d.Hy && d.Wx == d.Wy;
}
constexpr int row5x5_lds_bytes(int SW) {      // four waves x two buffers of (X strip + dY tile), or the block reduction's two images
    const int SP = (32 / SW) * (SW + 4), WBUF = SP * 32 + 32 * 32, IMG = 5 * 32 * 33;
    return (4 * 2 * WBUF > 2 * IMG ? 4 * 2 * WBUF : 2 * IMG) * 4;
}
inline int row5x5_nsplit(const WgradShape& d, int tcount, int cus) {
    constexpr int OCC = 2;      // resident blocks per CU (the kernel's launch bounds)
    const int tiles = 5 * (d.cin / 32) * (d.N / 32);
    const int chunks = d.M / 32 * (tcount > 1 ? tcount : 1);
    if (tiles < 1) return 1;      // (fewer than 32 channels: igemm_wgrad refuses the descriptor)
    // One block per CU is resident (~100 KB of LDS), so the grid is sized to whole rounds of the chip's CUs: the first
    // version asked for "about 512" blocks and got 520-600, i.e. a third round that ran 8-88 blocks on 256 CUs (lstm7: 264 us
    // for 171 us of MFMA work).  Take the fewest rounds (1..3) whose last round is at least 90 % full.
    const int res = cus * OCC;   // resident blocks
    int nsplit = 1;
    double best = 0.0;
    for (int r = 1; r <= 3; ++r) {
        int ns = (res * r) / tiles;
        if (ns > chunks / 16) ns = chunks / 16;          // >= 4 chunks per wave
        if (ns < 1) ns = 1;
        const long blocks = (long)tiles * ns;
        const double fill = (double)blocks / (double)(((blocks + res - 1) / res) * res);
        if (fill > best + 0.02) { best = fill; nsplit = ns; }
        if (best >= 0.9) break;
    }
    return nsplit;
}

// ---- the fp32 slot form (wgrad5x5p.hip) ------------------------------------------------------------------------------------------------------
constexpr int WP_CH = 16;                  // pixels per chunk
constexpr int wp_nbuf(int ntw) { return ntw == 1 ? 3 : 2; }                       // LDS buffers per wave
constexpr int wp_buf(int ntw) { return (2 * ntw + 3) * 256; }                      // floats per buffer: the dG tile's 2 NTW pieces, then the strip's three
constexpr int wp_lds_floats(int ntw) { return 4 * wp_nbuf(ntw) * wp_buf(ntw); }   // 60 KiB / 56 KiB: two blocks per CU
constexpr int wp_slot(int ntw) { return 5 * ntw * 1024 + 64; }                    // floats per segment slot: [t][kx][n][ci] + the bias tail (32 NTW used)
// The partition: shared by the kernel, the reduction and the host (slot count).  All quantities describe ONE timestep.
struct WpPartition {
    int J;              // blocks per XCD (grid = 8 J)
    int PP, TP;         // pixel parts x tile parts = 8 (one pair per XCD)
    int NTW;            // 32-column MFMA tiles per wave
    int T;              // tiles = 5 * (cin / 32) * (N / (32 NTW)), ordered (nb, cb, ky)
    int cpt;            // 16-pixel chunks per timestep
    int maxseg;         // slots per block
    int logW, logHW;    // the map is a power of two wide and high
};
struct WpRange { int t_lo, nt, c_lo, len; long long i0, i1; };
PIVP_WF_HD inline WpRange wp_range(const WpPartition& g, int x, int j) {
    WpRange r;
    const int px = x % g.PP, tx = x / g.PP;
    r.t_lo = (int)((long long)g.T * tx / g.TP);
    r.nt = (int)((long long)g.T * (tx + 1) / g.TP) - r.t_lo;
    r.c_lo = (int)((long long)g.cpt * px / g.PP);
    r.len = (int)((long long)g.cpt * (px + 1) / g.PP) - r.c_lo;
    const long long tot = (long long)r.nt * r.len;
    r.i0 = tot * j / g.J; r.i1 = tot * (j + 1) / g.J;
    return r;
}
inline bool wp_ok_shape(const WgradShape& d) {
    if (d.deconv || d.ksize != 5 || d.pad != 2 || d.stride != 1 || d.Hx != d.Hy || d.Wx != d.Wy) return false;
    if (d.Wg < 8 || (d.Wg & (d.Wg - 1)) || (d.Hg & (d.Hg - 1)) || d.Hg < 2) return false;
    if (d.M % WP_CH || d.N % 32 || d.cin % 32 || d.c0 % 32 || d.c1 % 32 || d.ld0 % 4 || d.ldy % 4 || (d.c1 && d.ld1 % 4)) return false;
    return true;
}
inline int ilog2(int v) { int l = 0; while ((1 << l) < v) ++l; return l; }
// slot_ntw: 0 = by shape, 1 / 2 = 32 / 64 columns per wave (64 needs N % 64 == 0)
inline int wp_ntw(const WgradShape& d, int slot_ntw) {
    if (d.N % 64) return 1;
    if (slot_ntw == 1 || slot_ntw == 2) return slot_ntw;
    return 1;
}
// slot_j: blocks per XCD, 0 = two per CU of a device with `cus` CUs (the CU count then decides the order of the sums)
inline WpPartition wp_geom(const WgradShape& d, int slot_ntw, int slot_j, int cus) {
    WpPartition g;
    g.J = slot_j > 0 ? slot_j : (2 * cus) / 8;
    if (g.J < 1) g.J = 1;
    g.NTW = wp_ntw(d, slot_ntw);
    g.T = 5 * (d.cin / 32) * (d.N / (32 * g.NTW));
    g.cpt = d.M / WP_CH;
    // pixel parts: as many as keep the segment count near the block count (every tile of a part is cut once more per part) and a part's chunk
    // range long enough for four waves
    int pp = 8;
    while (pp > 1 && ((long long)g.T * pp > 8LL * g.J || g.cpt / pp < 16)) pp >>= 1;
    // (r06_c05, all six shapes at B = 32: one part against this rule within +-2 % -- lstm7 222.5 against 218.1 us --, eight parts on the small maps
    // 5-25 % slower: lstm5 112.4 against 90.1)
    while (8 / pp > g.T) pp <<= 1;               // (fewer tiles than tile parts: never with this model's layers)
    g.PP = pp; g.TP = 8 / pp;
    g.logW = ilog2(d.Wg); g.logHW = ilog2(d.Hg * d.Wg);
    int ms = 1;
    for (int x = 0; x < 8; ++x)
        for (int j = 0; j < g.J; ++j) {
            const WpRange r = wp_range(g, x, j);
            if (r.i1 <= r.i0) continue;
            const int segs = (int)((r.i1 - 1) / r.len - r.i0 / r.len) + 1;
            if (segs > ms) ms = segs;
        }
    g.maxseg = ms;
    return g;
}

// ---- the stride-2 3x3 tile form (wgrad3x3s2.hip) ---------------------------------------------------------------------------------------------
constexpr int W3_PW = 17, W3_PH = 9, W3_PPIX = W3_PW * W3_PH;     // patch of a 4 x 8 anchor chunk
constexpr int W3_TARGET_BLOCKS = 256;
constexpr int W3_BIAS_TAIL = 128;      // floats behind a block's [unit][16][64] accumulators: its column sums of dY (bias gradient), <= 96 used
struct W3Shape { int deconv, TI, TJ, NW; };
// which instance takes a layer (0 = none): transposed 96 -> 96 (enc5) as one 3 x 3-tile block of twelve waves (seven units each, six for the last three),
// transposed convs on multiples of 64 channels (enc6, enc4) as 2 x 2-tile blocks of twelve waves (one kernel row of one tile each), convs (enc1, enc2) as
// one-tile blocks of three waves (tiny layers: parallelism first).  Waves per block at B = 32, nine timesteps per launch (r05_c17 .. r05_c19): enc6 4 / 8 / 12
// waves 265 / 244 / 235 us, enc4 76 / 69 / 67, enc5 8 / 12 waves 159 / 152, enc1 and enc2 3 / 9 waves 30 / 29.
inline int w3_instance(const WgradShape& d) {
    if (d.ksize != 3 || d.stride != 2 || d.pad != 1 || d.c1 != 0 || d.cin != d.c0 || d.wcin != d.cin) return 0;
    if (d.Hg % 4 || d.Wg % 8 || d.cin % 32 || d.N % 32 || d.ld0 % 4 || d.ldy % 4) return 0;
    if (d.deconv) {
        if (d.Hy != 2 * d.Hx || d.Wy != 2 * d.Wx || d.Hg != d.Hx || d.Wg != d.Wx) return 0;
        if (d.cin == 96 && d.N == 96) return 2;
        if (d.cin % 64 == 0 && d.N % 64 == 0) return 1;
        return 0;
    }
    if (d.Hx != 2 * d.Hy || d.Wx != 2 * d.Wy || d.Hg != d.Hy || d.Wg != d.Wy) return 0;
    return 3;
}
constexpr W3Shape w3_shape(int inst) {
    return inst == 1 ? W3Shape{1, 2, 2, 12} : inst == 2 ? W3Shape{1, 3, 3, 12} : W3Shape{0, 1, 1, 3};
}
constexpr W3Shape w3_shape(WgradForm f) { return w3_shape((int)f - 30); }
constexpr int w3_slot(const W3Shape& sh) { return sh.TI * sh.TJ * 9 * 1024 + W3_BIAS_TAIL; }      // floats of a block's slot
constexpr int w3_lds_bytes(const W3Shape& sh) {      // two chunk images (patch | small tile), whole DMA instructions per thread
    const int CS = (sh.deconv ? sh.TI : sh.TJ) * 32, CB = (sh.deconv ? sh.TJ : sh.TI) * 32;
    const int TOT4 = W3_PPIX * CB / 4 + 32 * CS / 4, KL = (TOT4 + sh.NW * 64 - 1) / (sh.NW * 64);
    return 2 * KL * sh.NW * 64 * 16;
}
// grid: a function of the ONE-timestep geometry alone, so every launch of a sweep, the partial buffer and the reduction agree
inline void w3_grid(const WgradShape& d, const W3Shape& sh, int& nblk, int& nsplit) {
    nblk = (d.cin / (32 * sh.TI)) * (d.N / (32 * sh.TJ));
    const int cpt = d.B * (d.Hg / 4) * (d.Wg / 8);
    nsplit = W3_TARGET_BLOCKS / nblk;
    if (nsplit > cpt) nsplit = cpt;
    if (nsplit < 1) nsplit = 1;
}

// ---- the packed-operand forms (wgrad_bf16.hip) -----------------------------------------------------------------------------------------------
// The maps the packed-operand kernels' tiles serve (convlstm_bf16.hip, conv5x5_bf16.hip, wgrad_bf16.hip): 8 rows deep, and 16 wide or 8 wide with two images
// to a tile (an even batch).  The one predicate of the kernels' own checks (bf16_geometry_ok, the packed forms here), of the forward's per-layer fall-back to fp32,
// of the sweep's choice of a cell's data- and weight-gradient form (Modes, plan.h) and of the op entries' refusals: they must agree on every map.
constexpr bool packed_tiles_serve(int H, int W, int B) { return H % 8 == 0 && (W % 16 == 0 || (W % 8 == 0 && B % 2 == 0)); }
inline bool wgrad5x5_packed_ok(const WgradShape& d, int tcount) {
    if (d.deconv || d.ksize != 5 || d.pad != 2 || d.stride != 1 || d.Hx != d.Hy || d.Wx != d.Wy) return false;
    if (d.N % 128 || d.cin % 32 || d.c0 % 32 || d.c1 % 32 || d.ld0 % 4 || d.ld1 % 4 || d.ldy % 4) return false;
    if (tcount > 1 && !d.ts_aligned) return false;
    return packed_tiles_serve(d.Hx, d.Wx, d.B);
}
constexpr int PACKED_ROW_LDS = 128 * 320 + 192 * 64;                  // dG image [128 px] at a 320-byte pitch | X strip of 192 pixels x 32 bf16
constexpr int PACKED25_GH = 128 * 64 + 64, PACKED25_X = 320 * 64;     // one 32-column half of the dG tile | the X patch of 320 pixels (one plane each)
// Pixel splits of the packed forms: about `target` blocks over the gx output slices, at least 2 tiles per block, the tiles dealt evenly
struct PixelSplit { int ns, tps; };      // splits (grid y), tiles per split
inline PixelSplit packed_split(int n_tiles, int gx, int target) {
    int ns = (target + gx - 1) / gx;
    if (ns > n_tiles / 2) ns = n_tiles / 2;
    if (ns < 1) ns = 1;
    const int tps = (n_tiles + ns - 1) / ns;
    return {(n_tiles + tps - 1) / tps, tps};
}
// The sweep's hint for a batch of timesteps with plain bf16 operands (`form` of wgrad_launch): the eight-wave form on every layer of frames above
// 64 x 64 x 32 -- config 5, whose main-stream kernels fill the chip by themselves: 68.2 ms with the four-wave form everywhere against 66.3
inline int packed_form_hint(int B, int frame_h, int frame_w) { return (long)B * frame_h * frame_w > 32L * 64 * 64 ? 2 : 0; }

// ---- the answer ------------------------------------------------------------------------------------------------------------------------------
struct WgradLaunch {
    WgradForm form;
    int gx, gy, threads, lds_bytes;      // the kernel's grid, block and dynamic LDS
    int tiles_per_split;                 // the packed forms' second kernel argument (0 elsewhere)
    long long part_floats;               // floats of the partial buffer the form adds into (0: it has none)
    int rgx, rgy;                        // the reduce kernel's grid (256 threads; 0: the form has no reduction)
    bool bias_rides;                     // the kernel sums dy's columns itself (into db, or into the slots its reduction adds to db): no bias_grad launch
    WpPartition wp;                      // slot forms only: the kernel's and the reduction's second argument
};

// operand: 0 = fp32, 1 = bf16, 2 = two bf16 pieces (no weight-gradient form), 3 = three bf16 pieces, 4 = two fp16 pieces (Operand, pivp_kernels.h).
// tcount: timesteps in the launch.  form: the packed bf16 batch's block form, 0 = by size, 1 = four-wave, 2 = eight-wave.  slot_ntw / slot_j: see wp_ntw /
// wp_geom.  has_part: a partial buffer is given -- or asked about: the buffer's size and the reduction are those of the launch WITH the buffer.
// cus: the device's compute units.
inline WgradLaunch wgrad_launch(const WgradShape& d, int operand, int tcount, int form, int slot_ntw, int slot_j, int has_part, int cus) {
    WgradLaunch L{};
    L.threads = 256;
    if (operand != 0) {      // 5x5 ConvLSTM case only: operands as bf16 or as pieces, fp32 accumulation; db summed on the side in fp32
        if (operand < 1 || operand > 4 || operand == 2 || !wgrad5x5_packed_ok(d, tcount) || d.wcin < d.cin || d.wcin % 32) return L;
        const int tw = d.Wx % 16 == 0 ? 16 : 8, ti_n = tw == 16 ? 1 : 2, w16 = tw == 16;
        const int tiles1 = (d.B / ti_n) * (d.Hx / 8) * (d.Wx / tw), n_tiles = tiles1 * (tcount > 1 ? tcount : 1);
        L.bias_rides = true;
        PixelSplit sp;
        // A batch of timesteps goes to the 25-tap kernel (per timestep at B = 32, all seven layers: 168 us at 8 per launch, 225 us at 4); ONE
        // timestep to the kernel-row kernel, whose 5 x cin/32 blocks per tile are then the better use of the chip (389 us against 580:
        // the sweep's t = 0 launches, sequences too short to batch).  Pieces (fp16x3, bf16x6): the 25-tap kernel, whatever the batch.
        if (operand == 1 && tcount <= 1) {
            // Pixel splits: about one block per TWO CUs, at least 2 tiles per block.  Two blocks per CU could be resident, but the kernel is not
            // short of parallelism: it is short of tiles per block -- every block ends with 20,480 atomic adds into the same 80 KB of dW as the
            // other splits of its tile (timing-only build without them: 72 -> 43 us on lstm1 at 52 splits) -- and it runs on the side stream, where
            // a grid that fills every CU's registers starves the main stream's small kernels (a 5 us add_strided took 34 us beside it).
            // Train step in the bf16 mode against the block target: 512: 13.93 ms, 256: 13.00, 192: 12.73, 128: 12.54, 96: 13.08, 64: 14.57.
            L.form = w16 ? WgradForm::PackedRow_16 : WgradForm::PackedRow_8;
            L.gx = 5 * (d.cin / 32) * (d.N / 128);
            L.lds_bytes = PACKED_ROW_LDS;
            sp = packed_split(tiles1, L.gx, cus / 2);
        } else if (operand == 1 && (form == 1 || (form == 0 && (long)d.B * d.Hx * d.Wx <= 32L * 32 * 32))) {
            // A batch of timesteps: the four-wave form (co-resident with the main stream's small kernels) on maps of up to 32 x 32 x 32 pixels per
            // timestep, the eight-wave form (half the patch traffic per multiply-add) on larger ones; see packed_form_hint for the plan's say.
            // (One timestep on the four-wave form: config 3 11.36 against 11.29 ms: the kernel-row kernel stays.)
            // about one block per CU (config 3's step against the block target: 128: 11.84 ms, 256: 11.28, 384: 11.25, 512: 11.60)
            L.form = w16 ? WgradForm::Packed25x4_16 : WgradForm::Packed25x4_8;
            L.gx = (d.cin / 32) * (d.N / 32);
            L.lds_bytes = PACKED25_GH + PACKED25_X;
            sp = packed_split(n_tiles, L.gx, cus);
        } else {
            // the 25-tap kernel: grid = (cin / 32) x (N / 64) output slices x pixel splits over the tiles of ALL timesteps of the batch
            // Pixel splits: one block per CU (8 waves, ~70 KB of LDS), at least 2 tiles per block; every split ends with 25 x 32 x 64 atomic adds
            // (205 KB: the batch of timesteps is what amortises them).
            // (fp16 pieces: its 8-wave blocks hold a CU's whole register file, and the sweep's small kernels need CUs without one: half the CUs)
            // bf16: three quarters (train step 11.86 -> 11.66 ms, profiles/r04/bf16_train_wgrad_batch_slots.txt)
            const int pcs = operand == 1 ? 1 : operand == 4 ? 2 : 3;
            L.form = (WgradForm)((int)WgradForm::Packed25x8_1_8 + 2 * (pcs - 1) + w16);
            L.gx = (d.cin / 32) * (d.N / 64);
            L.threads = 512;
            L.lds_bytes = pcs * (2 * PACKED25_GH + PACKED25_X);
            sp = packed_split(n_tiles, L.gx, pcs >= 2 ? cus / 2 : cus * 3 / 4);
        }
        L.gy = sp.ns; L.tiles_per_split = sp.tps;
        return L;
    }
    if (has_part && wp_ok_shape(d)) {        // ConvLSTM 5x5, partial-slot form (round 6): no atomics; the column sums ride along
        L.wp = wp_geom(d, slot_ntw, slot_j, cus);
        L.form = d.Wg >= 16 ? (L.wp.NTW == 2 ? WgradForm::Slot5x5_16x2 : WgradForm::Slot5x5_16x1) : (L.wp.NTW == 2 ? WgradForm::Slot5x5_8x2 : WgradForm::Slot5x5_8x1);
        L.gx = 8 * L.wp.J; L.gy = 1;
        L.lds_bytes = wp_lds_floats(L.wp.NTW) * 4;
        L.part_floats = (long long)8 * L.wp.J * L.wp.maxseg * wp_slot(L.wp.NTW);
        L.rgx = L.wp.T * 5 * L.wp.NTW; L.rgy = 1;
        L.bias_rides = true;
        return L;
    }
    if (takes_fast_path(d)) {
        const int SW = d.Wg == 8 ? 8 : d.Wg == 16 ? 16 : 32;
        L.form = SW == 8 ? WgradForm::Row5x5_8 : SW == 16 ? WgradForm::Row5x5_16 : WgradForm::Row5x5_32;
        L.gx = 5 * (d.cin / 32) * (d.N / 32); L.gy = row5x5_nsplit(d, tcount, cus);
        L.lds_bytes = row5x5_lds_bytes(SW);
        L.bias_rides = true;
        return L;
    }
    if (has_part && w3_instance(d)) {      // stride-2 3x3: all nine taps from one staging (wgrad3x3s2.hip); the column sums ride along
        const int inst = w3_instance(d);
        const W3Shape sh = w3_shape(inst);
        L.form = (WgradForm)(30 + inst);
        w3_grid(d, sh, L.gx, L.gy);
        L.threads = sh.NW * 64;
        L.lds_bytes = w3_lds_bytes(sh);
        L.part_floats = (long long)L.gx * L.gy * w3_slot(sh);
        L.rgx = sh.TI * sh.TJ * 9 * 32 + sh.TJ; L.rgy = L.gx;
        L.bias_rides = true;
        return L;
    }
    int wg_n;
    generic_grid(d, wg_n, L.gx, L.gy);
    L.form = has_part ? (wg_n == 64 ? WgradForm::Generic64Part : WgradForm::Generic128Part) : (wg_n == 64 ? WgradForm::Generic64 : WgradForm::Generic128);
    if (has_part) {
        L.part_floats = (long long)L.gx * L.gy * 64 * wg_n;
        L.rgx = (64 * wg_n + 255) / 256; L.rgy = L.gx;
    }
    L.bias_rides = generic_bias_rides(d);
    return L;
}

}  // namespace pivp
