"""The weight gradients' launch forms (csrc/wgrad_form.h) on the host: a stand-alone program that includes nothing but that header is compiled for the host
(-Wall -Werror) and prints the WgradLaunch -- form, grid, block, dynamic LDS, tiles per split, floats of the partial buffer, the reduction's grid, whether the
bias rides -- of every product layer over the whole domain the plan accepts (B 1..64, frames in multiples of 8 from 16 x 16 to 256 x 248) in the forms the sweeps
launch, and of every layer on a grid of frames in every operand form, single and batched, with and without a partial buffer, under the hints 0 / 1 / 2, at 256
compute units and at 304.  Every field is compared with `ref_launch`, a restatement of the dispatch and grid rules as they stood inside igemm_wgrad /
igemm_wgrad_part_floats / igemm_wgrad_reduce (igemm_wgrad.hip), wgrad5x5p.hip, wgrad3x3s2.hip and wgrad5x5_bf16 (wgrad_bf16.hip) before the header existed, so
the refactor moved no launch.  Then: no form without a product layer or a GPU case that reaches it, and the restatement against the built library's own sizes."""
import os
import re
import struct
import subprocess
import sys
from functools import lru_cache
from types import SimpleNamespace

import pytest

from pivp_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
CSRC = os.path.join(os.path.dirname(_lib.LIB_PATH), 'csrc')
F32, BF16, BF16X3, BF16X6, FP16X3 = 0, 1, 2, 3, 4
FORM = {m.group(1): int(m.group(2)) for m in re.finditer(r'\b(None|[A-Z][A-Za-z0-9]+(?:_\w+)?) = (\d+)', open(os.path.join(CSRC, 'wgrad_form.h')).read().split('enum class WgradForm')[1].split('};')[0])}
NAME = {v: k for k, v in FORM.items()}
FRAMES = [(H, W) for H in range(16, 257, 8) for W in range(16, 249, 8)]      # what plan_serves_forward accepts
# the grid of frames every combination runs on: power-of-two frames (the slot form's maps), 8-wide and odd maps, the largest frame
GRID_256 = GRID = [(16, 16), (32, 32), (64, 64), (64, 128), (128, 128), (24, 16), (32, 16), (72, 40), (64, 48), (136, 104), (256, 128), (256, 248)]
# the layers (csrc/plan.h): the seven cells as (cx, C, level) -- lstm1 and lstm2 are one shape --, with and without the h operand (the sweep's t = 0); the five
# stride-2 3x3 layers enc6, enc5, enc4, enc2, enc1 as (mode, channels, ldx, ldy, level of the input map)
CELLS = [(32, 32, 2), (32, 64, 4), (64, 64, 4), (64, 128, 8), (128, 64, 4), (96, 32, 2)]
ENCS = [(1, 64, 64, 64, 2), (1, 96, 96, 128, 4), (1, 128, 128, 192, 8), (0, 64, 64, 64, 4), (0, 32, 32, 96, 2)]
DET_SLOT_J = 64

PROGRAM = r'''
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "wgrad_form.h"
using namespace pivp;
// cus operand tcount hint slot_j has_part kind a b c ld0 ldy level Blo Bhi ts_aligned frames     (frames: all | H:W,H:W,...; one row of ten int32 per frame and B)
int main(int argc, char** argv) {
    if (argc != 18) return 2;
    int v[17];
    for (int i = 1; i < 17; ++i) v[i] = atoi(argv[i]);
    const int cus = v[1], operand = v[2], tcount = v[3], hint = v[4], slot_j = v[5], has_part = v[6], kind = v[7], a = v[8], b = v[9], c = v[10], ld0 = v[11],
              ldy = v[12], level = v[13], Blo = v[14], Bhi = v[15], ts_aligned = v[16];
    static int fr[2048][2];
    int nf = 0;
    if (!strcmp(argv[17], "all")) { for (int H = 16; H <= 256; H += 8) for (int W = 16; W <= 248; W += 8) { fr[nf][0] = H; fr[nf][1] = W; ++nf; } }
    else for (char* p = argv[17]; p && *p && nf < 2048; ) { fr[nf][0] = atoi(p); p = strchr(p, ':') + 1; fr[nf][1] = atoi(p); ++nf; p = strchr(p, ','); if (p) ++p; }
    for (int f = 0; f < nf; ++f)
        for (int B = Blo; B <= Bhi; ++B) {
            const int H = fr[f][0] / level, W = fr[f][1] / level;
            WgradShape d{};
            if (kind == 0) {      // a cell (lstm_wgrad_geom, run_wgrad): a = cx, b = C, c = has_h
                d.c0 = a; d.ld0 = ld0; d.c1 = c ? b : 0; d.ld1 = b; d.cin = d.c0 + d.c1; d.wcin = a + b; d.N = 4 * b; d.ldy = ldy;
                d.B = B; d.Hx = H; d.Wx = W; d.Hy = H; d.Wy = W; d.Hg = H; d.Wg = W; d.M = B * H * W; d.ksize = 5; d.pad = 2; d.stride = 1;
            } else {              // a stride-2 3x3 layer (conv3x3s2_wgrad_geom): a = mode, b = channels in, c = channels out
                const int Ho = a ? 2 * H : H / 2, Wo = a ? 2 * W : W / 2;
                d.c0 = b; d.ld0 = ld0; d.cin = b; d.wcin = b; d.N = c; d.ldy = ldy; d.B = B; d.Hx = H; d.Wx = W; d.Hy = Ho; d.Wy = Wo;
                d.deconv = a; d.ksize = 3; d.pad = 1; d.stride = 2; d.Hg = a ? H : Ho; d.Wg = a ? W : Wo; d.M = B * d.Hg * d.Wg;
            }
            d.ts_aligned = ts_aligned;
            const WgradLaunch L = wgrad_launch(d, operand, tcount, hint, hint, slot_j, has_part, cus);
            if (L.part_floats >= (1LL << 31)) return 3;
            const int row[10] = {(int)L.form, L.gx, L.gy, L.threads, L.lds_bytes, L.tiles_per_split, (int)L.part_floats, L.rgx, L.rgy, (int)L.bias_rides};
            fwrite(row, sizeof(int), 10, stdout);
        }
    return 0;
}
'''


# ---- the restatement: the parent's launchers, line by line -------------------------------------------------------------------------------------------------
def cell_shape(cx, C, has_h, B, H, W, ld0=None, ldy=None):
    """lstm_wgrad_geom, then run_wgrad's `if (!d.x1) d.c1 = 0; d.cin = d.c0 + d.c1`"""
    c1 = C if has_h else 0
    return SimpleNamespace(c0=cx, ld0=ld0 or cx, c1=c1, ld1=C, cin=cx + c1, wcin=cx + C, N=4 * C, ldy=ldy or 4 * C, B=B, Hx=H, Wx=W, Hy=H, Wy=W, Hg=H, Wg=W,
                           M=B * H * W, deconv=0, ksize=5, pad=2, stride=1)


def enc_shape(mode, c, ld0, ldy, B, Hin, Win, cout=None):
    """conv3x3s2_wgrad_geom"""
    Hout, Wout = (2 * Hin, 2 * Win) if mode else (Hin // 2, Win // 2)
    Hg, Wg = (Hin, Win) if mode else (Hout, Wout)
    return SimpleNamespace(c0=c, ld0=ld0, c1=0, ld1=0, cin=c, wcin=c, N=cout or c, ldy=ldy, B=B, Hx=Hin, Wx=Win, Hy=Hout, Wy=Wout, Hg=Hg, Wg=Wg, M=B * Hg * Wg,
                           deconv=mode, ksize=3, pad=1, stride=2)


def wp_ok_shape(d):
    if d.deconv or d.ksize != 5 or d.pad != 2 or d.stride != 1 or d.Hx != d.Hy or d.Wx != d.Wy:
        return False
    if d.Wg < 8 or (d.Wg & (d.Wg - 1)) or (d.Hg & (d.Hg - 1)) or d.Hg < 2:
        return False
    return not (d.M % 16 or d.N % 32 or d.cin % 32 or d.c0 % 32 or d.c1 % 32 or d.ld0 % 4 or d.ldy % 4 or (d.c1 and d.ld1 % 4))


@lru_cache(maxsize=None)
def wp_geom(cin, N, M, slot_ntw, slot_j, cus):
    """wgrad5x5p.hip's wp_ntw + wp_geom with wp_range -> (J, NTW, T, maxseg)"""
    J = slot_j if slot_j > 0 else (2 * cus) // 8
    J = max(J, 1)
    NTW = 1 if N % 64 else slot_ntw if slot_ntw in (1, 2) else 1
    T = 5 * (cin // 32) * (N // (32 * NTW))
    cpt = M // 16
    pp = 8
    while pp > 1 and (T * pp > 8 * J or cpt // pp < 16):
        pp >>= 1
    while 8 // pp > T:
        pp <<= 1
    PP, TP = pp, 8 // pp
    ms = 1
    for x in range(8):
        px, tx = x % PP, x // PP
        t_lo = T * tx // TP
        nt = T * (tx + 1) // TP - t_lo
        c_lo = cpt * px // PP
        ln = cpt * (px + 1) // PP - c_lo
        tot = nt * ln
        for j in range(J):
            i0, i1 = tot * j // J, tot * (j + 1) // J
            if i1 <= i0:
                continue
            ms = max(ms, (i1 - 1) // ln - i0 // ln + 1)
    return J, NTW, T, ms


def takes_fast_path(d):
    return (not d.deconv and d.ksize == 5 and d.pad == 2 and d.stride == 1 and d.M % 32 == 0 and d.N % 64 == 0 and (d.Wg == 8 or d.Wg == 16 or d.Wg % 32 == 0) and
            (d.Wg >= 32 or d.Hg % (32 // d.Wg) == 0) and d.Hx == d.Hy and d.Wx == d.Wy)


def w3_instance(d):
    if d.ksize != 3 or d.stride != 2 or d.pad != 1 or d.c1 != 0 or d.cin != d.c0 or d.wcin != d.cin:
        return 0
    if d.Hg % 4 or d.Wg % 8 or d.cin % 32 or d.N % 32 or d.ld0 % 4 or d.ldy % 4:
        return 0
    if d.deconv:
        if d.Hy != 2 * d.Hx or d.Wy != 2 * d.Wx or d.Hg != d.Hx or d.Wg != d.Wx:
            return 0
        if d.cin == 96 and d.N == 96:
            return 2
        return 1 if d.cin % 64 == 0 and d.N % 64 == 0 else 0
    if d.Hx != 2 * d.Hy or d.Wx != 2 * d.Wy or d.Hg != d.Hy or d.Wg != d.Wy:
        return 0
    return 3


def packed_split(n_tiles, gx, target):
    ns = (target + gx - 1) // gx
    ns = max(min(ns, n_tiles // 2), 1)
    tps = (n_tiles + ns - 1) // ns
    return (n_tiles + tps - 1) // tps, tps


NONE = (0, 0, 0, 256, 0, 0, 0, 0, 0, 0)


def ref_launch(d, operand, tcount, form, slot_ntw, slot_j, has_part, cus, ts_aligned=1):
    """(form, grid x, grid y, threads, LDS bytes, tiles per split, floats of the partial buffer, the reduce kernel's grid x, y, the bias rides)"""
    tc = max(tcount, 1)
    if operand != F32:                                   # run_wgrad -> wgrad5x5_bf16
        if d.deconv or d.ksize != 5 or d.pad != 2 or d.stride != 1 or d.Hx != d.Hy or d.Wx != d.Wy:      # wgrad5x5_bf16_ok
            return NONE
        if d.N % 128 or d.cin % 32 or d.c0 % 32 or d.c1 % 32 or d.ld0 % 4 or d.ld1 % 4 or d.ldy % 4:
            return NONE
        if tcount > 1 and not ts_aligned:                # (d.ts_x0 % 16 || d.ts_x1 % 16 || d.ts_dy % 16)
            return NONE
        if not (d.Hx % 8 == 0 and (d.Wx % 16 == 0 or (d.Wx % 8 == 0 and d.B % 2 == 0))):                  # packed_tiles_serve
            return NONE
        if d.wcin < d.cin or d.wcin % 32 or operand == BF16X3:
            return NONE
        tw = 16 if d.Wx % 16 == 0 else 8
        ti_n = 1 if tw == 16 else 2
        n1 = (d.B // ti_n) * (d.Hx // 8) * (d.Wx // tw)

        def wgrad25(pcs):                                # launch_wgrad25<PCS>
            gx = (d.cin // 32) * (d.N // 64)
            ns, tps = packed_split(n1 * tc, gx, cus // 2 if pcs >= 2 else cus * 3 // 4)
            return (FORM['Packed25x8_%d_%d' % (pcs, tw)], gx, ns, 512, pcs * (2 * (128 * 64 + 64) + 320 * 64), tps, 0, 0, 0, 1)
        if operand == FP16X3:
            return wgrad25(2)
        if operand == BF16X6:
            return wgrad25(3)
        if tcount > 1:
            if form == 1 or (form == 0 and d.B * d.Hx * d.Wx <= 32 * 32 * 32):      # launch_wgrad25_nw4
                gx = (d.cin // 32) * (d.N // 32)
                ns, tps = packed_split(n1 * tc, gx, cus)
                return (FORM['Packed25x4_%d' % tw], gx, ns, 256, 128 * 64 + 64 + 320 * 64, tps, 0, 0, 0, 1)
            return wgrad25(1)
        gx = 5 * (d.cin // 32) * (d.N // 128)            # the kernel-row kernel
        ns, tps = packed_split(n1, gx, cus // 2)
        return (FORM['PackedRow_%d' % tw], gx, ns, 256, 128 * 320 + 192 * 64, tps, 0, 0, 0, 1)
    # igemm_wgrad / igemm_wgrad_part_floats / igemm_wgrad_reduce: wgrad5x5p_ok -> takes_fast_path -> wgrad3x3s2_ok -> generic
    if has_part and wp_ok_shape(d):
        J, NTW, T, ms = wp_geom(d.cin, d.N, d.M, slot_ntw, slot_j, cus)
        sw = 16 if d.Wg >= 16 else 8
        lds = 4 * (3 if NTW == 1 else 2) * (2 * NTW + 3) * 256 * 4
        return (FORM['Slot5x5_%dx%d' % (sw, NTW)], 8 * J, 1, 256, lds, 0, 8 * J * ms * (5 * NTW * 1024 + 64), T * 5 * NTW, 1, 1)
    if takes_fast_path(d):                               # launch_wgrad5x5<SW>
        SW = 8 if d.Wg == 8 else 16 if d.Wg == 16 else 32
        SP = (32 // SW) * (SW + 4)
        lds = max(4 * 2 * (SP * 32 + 32 * 32), 2 * 5 * 32 * 33) * 4
        tiles = 5 * (d.cin // 32) * (d.N // 32)
        chunks = d.M // 32 * tc
        res = cus * 2
        nsplit, best = 1, 0.0
        for r in (1, 2, 3):
            ns = max(min((res * r) // tiles, chunks // 16), 1)
            blocks = tiles * ns
            fill = float(blocks) / float(((blocks + res - 1) // res) * res)
            if fill > best + 0.02:
                best, nsplit = fill, ns
            if best >= 0.9:
                break
        return (FORM['Row5x5_%d' % SW], tiles, nsplit, 256, lds, 0, 0, 0, 0, 1)
    inst = w3_instance(d)
    if has_part and inst:
        deconv, TI, TJ, NW = {1: (1, 2, 2, 12), 2: (1, 3, 3, 12), 3: (0, 1, 1, 3)}[inst]
        nblk = (d.cin // (32 * TI)) * (d.N // (32 * TJ))
        nsplit = max(min(256 // nblk, d.B * (d.Hg // 4) * (d.Wg // 8)), 1)
        CS, CB = ((TI, TJ) if deconv else (TJ, TI))
        TOT4 = 17 * 9 * CB * 32 // 4 + 32 * CS * 32 // 4
        KL = (TOT4 + NW * 64 - 1) // (NW * 64)
        return (FORM[{1: 'Tile3x3s2_D2x2', 2: 'Tile3x3s2_D3x3', 3: 'Tile3x3s2_C1x1'}[inst]], nblk, nsplit, NW * 64, 2 * KL * NW * 64 * 16, 0,
                nblk * nsplit * (TI * TJ * 9 * 1024 + 128), TI * TJ * 9 * 32 + TJ, nblk, 1)
    wg_n = 64 if d.N <= 64 else 128                      # generic_grid
    tiles = d.ksize * d.ksize * ((d.cin + 63) // 64) * ((d.N + wg_n - 1) // wg_n)
    nsplit = max(min((512 + tiles - 1) // tiles, ((d.M + 31) // 32) // 8), 1)
    bias = int(d.ksize == 3 and (not d.deconv or (d.Hy == 2 * d.Hx and d.Wy == 2 * d.Wx)))
    if has_part:
        return (FORM['Generic%dPart' % wg_n], tiles, nsplit, 256, 0, 0, tiles * nsplit * 64 * wg_n, (64 * wg_n + 255) // 256, tiles, bias)
    return (FORM['Generic%d' % wg_n], tiles, nsplit, 256, 0, 0, 0, 0, 0, bias)


# ---- the program ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp('wgrad_form')
    src, out = str(d / 'wgrad_form.cpp'), str(d / 'wgrad_form')
    with open(src, 'w') as f:
        f.write(PROGRAM)
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')      # the compiler build.py uses; host only: plain C++, no device code, no library
    subprocess.check_call([hipcc, '-x', 'c++', '-std=c++17', '-O1', '-Wall', '-Werror', '-I', CSRC, src, '-o', out])
    return out


def ask(exe, cus, operand, tcount, hint, slot_j, has_part, spec, Bs, frames, ts_aligned=1):
    """spec: ('cell', cx, C, has_h, level[, ld0, ldy]) | ('enc', mode, c, ldx, ldy, level[, cout]) -> the program's rows and the shapes they belong to, in its order"""
    if spec[0] == 'cell':
        _, cx, C, has_h, level = spec[:5]
        ld0, ldy = (spec[5], spec[6]) if len(spec) > 5 else (cx, 4 * C)
        args = [0, cx, C, has_h, ld0, ldy, level]
    else:
        _, mode, c, ldx, ldy, level = spec[:6]
        args = [1, mode, c, spec[6] if len(spec) > 6 else c, ldx, ldy, level]
    fr = 'all' if frames is FRAMES else ','.join('%d:%d' % f for f in frames)
    raw = subprocess.check_output([exe] + [str(a) for a in [cus, operand, tcount, hint, slot_j, has_part] + args + [Bs[0], Bs[-1], ts_aligned, fr]])
    rows = list(struct.iter_unpack('<10i', raw))
    assert len(rows) == len(frames) * len(Bs)
    shapes = ((B, H // level, W // level) for H, W in frames for B in Bs)
    return rows, shapes, level


def check(exe, cus, operand, tcount, hint, slot_j, has_part, spec, Bs, frames, reached, ts_aligned=1):
    rows, shapes, level = ask(exe, cus, operand, tcount, hint, slot_j, has_part, spec, Bs, frames, ts_aligned)
    for got, (B, H, W) in zip(rows, shapes):
        if spec[0] == 'cell':
            d = cell_shape(spec[1], spec[2], spec[3], B, H, W)
        else:
            d = enc_shape(spec[1], spec[2], spec[3], spec[4], B, H, W)
        want = ref_launch(d, operand, tcount, hint, hint, slot_j, has_part, cus, ts_aligned)
        assert got == want, (spec, 'B %d map %d x %d' % (B, H, W), dict(cus=cus, operand=operand, tcount=tcount, hint=hint, slot_j=slot_j, has_part=has_part),
                             NAME.get(got[0]), got, NAME.get(want[0]), want)
        reached.add(got[0])


CELL_SPECS = [('cell', cx, C, has_h, level) for cx, C, level in CELLS for has_h in (1, 0)]
ENC_SPECS = [('enc',) + e for e in ENCS]
BS = list(range(1, 65))
LAYER_FORMS = set()      # what the two layer tests reach (the third test reads it, and runs the grid itself when selected alone)


def test_the_header_chooses_what_the_launchers_chose_on_every_frame(exe):
    """the whole domain, in the forms the sweeps launch: the fp32 sweep's cells (kernel-row form or generic, atomics), the bf16 sweep's batches of four
    timesteps, the deterministic sweep's cells (the slot form at slot_j = 64 where pivp_plan_set_deterministic admits the frame), and every sweep's 3x3 layers
    into their partial planes.  The other combinations of operand form, tcount, partial buffer and hint run on a grid of frames (next test): the full cross
    product over 59,520 frame-and-batch points is minutes of Python."""
    for spec in CELL_SPECS:
        check(exe, 256, F32, 1, 0, 0, 0, spec, BS, FRAMES, LAYER_FORMS)
        check(exe, 256, BF16, 4, 0, 0, 0, spec, BS, FRAMES, LAYER_FORMS)
        check(exe, 256, F32, 4, 0, DET_SLOT_J, 1, spec, BS, FRAMES, LAYER_FORMS)
    for spec in ENC_SPECS:
        check(exe, 256, F32, 4, 0, 0, 1, spec, BS, FRAMES, LAYER_FORMS)


def test_every_operand_form_batch_partial_buffer_and_hint_on_a_grid_of_frames(exe):
    for cus, GRID in ((256, GRID_256), (304, GRID_256[1:9:2])):      # (304: the dependence on the CU count travels in the argument)
        for spec in CELL_SPECS:
            for tcount in (1, 4):
                check(exe, cus, F32, tcount, 0, 0, 0, spec, BS, GRID, LAYER_FORMS)
                for hint in (0, 1, 2):
                    check(exe, cus, F32, tcount, hint, 0, 1, spec, BS, GRID, LAYER_FORMS)
                    check(exe, cus, BF16, tcount, hint, 0, 0, spec, BS, GRID, LAYER_FORMS)
                check(exe, cus, BF16X6, tcount, 0, 0, 0, spec, BS, GRID, LAYER_FORMS)
                check(exe, cus, FP16X3, tcount, 0, 0, 0, spec, BS, GRID, LAYER_FORMS)
            check(exe, cus, F32, 4, 0, DET_SLOT_J, 1, spec, BS, GRID, LAYER_FORMS)      # the deterministic sweep's launches
            check(exe, cus, BF16X3, 4, 0, 0, 0, spec, BS[:2], GRID, LAYER_FORMS)        # no weight-gradient form: refused
            for operand in (F32, BF16, BF16X6, FP16X3):      # timesteps that are no multiple of 16 bytes apart: the packed forms refuse a batch, and only a batch
                for tcount in (1, 4):
                    check(exe, cus, operand, tcount, 0, 0, 0, spec, BS[:4], GRID, LAYER_FORMS, ts_aligned=0)
        for spec in ENC_SPECS:
            for tcount in (1, 4):
                for has_part in (0, 1):
                    check(exe, cus, F32, tcount, 0, 0, has_part, spec, BS, GRID, LAYER_FORMS)
    # the dependence is real: lstm7's kernel-row split and lstm1's slot partition at 64 x 64, B = 32
    a = ask(exe, 256, F32, 1, 0, 0, 0, CELL_SPECS[10], [32], [(64, 64)])[0][0]
    b = ask(exe, 304, F32, 1, 0, 0, 0, CELL_SPECS[10], [32], [(64, 64)])[0][0]
    assert a[0] == b[0] == FORM['Row5x5_32'] and a[2] != b[2]
    a = ask(exe, 256, F32, 1, 0, 0, 1, CELL_SPECS[0], [32], [(64, 64)])[0][0]
    b = ask(exe, 304, F32, 1, 0, 0, 1, CELL_SPECS[0], [32], [(64, 64)])[0][0]
    assert a[0] == b[0] == FORM['Slot5x5_16x1'] and (a[1], b[1]) == (512, 608)
    assert ask(exe, 304, F32, 1, 0, DET_SLOT_J, 1, CELL_SPECS[0], [32], [(64, 64)])[0][0] == a      # ... and slot_j takes it away


def gpu_case_forms(exe):
    """the forms the GPU tests' own cases reach: tests/test_gpu_backward_ops.py and tests/test_gpu_backward_shapes.py (the checkers of tests/backward_cases.py),
    the SERVED table and the tests/test_gpu_bf16.py parametrisations, each through the entry its checker calls"""
    sys.path.insert(0, os.path.dirname(HERE))
    import test_gpu_backward_ops as O
    import test_gpu_backward_shapes as S
    import test_gpu_bf16 as T

    def params(fn, names):
        return [m.args[1] for m in fn.pytestmark if m.name == 'parametrize' and m.args[0] == names][0]
    forms = {}

    def one(what, spec, B, H, W, operand=F32, tcount=1, hint=0, has_part=0):
        forms.setdefault(ask(exe, 256, operand, tcount, hint, 0, has_part, spec, [B], [(H, W)])[0][0][0], what)
    for B, cx, C, H, first in params(O.test_convlstm_backward, 'B,cx,C,H,first'):
        one('ops::test_convlstm_backward', ('cell', cx, C, int(not first), 1), B, H, H)
    for B, cx, C, H, W, first in S.LSTM_CASES:
        one('shapes::test_convlstm_backward', ('cell', cx, C, int(not first), 1), B, H, W)
    for mode, B, cin, cout, H in params(O.test_conv_deconv_backward, 'mode,B,cin,cout,H'):
        one('ops::test_conv_deconv_backward', ('enc', mode, cin, cin, cout, 1, cout), B, H, H)
    for mode, B, cin, cout, H, T_ in params(O.test_conv_weight_gradient_batched_over_timesteps, 'mode,B,cin,cout,H,T'):
        one('ops::test_conv_weight_gradient_batched_over_timesteps', ('enc', mode, cin, cin, cout, 1, cout), B, H, H, tcount=T_, has_part=1)
    for mode, B, cin, cout, H, W in S.CONV_CASES:
        one('shapes::test_conv_deconv_backward', ('enc', mode, cin, cin, cout, 1, cout), B, H, W)
        one('shapes::test_conv_weight_gradient_in_partial_planes', ('enc', mode, cin, cin, cout, 1, cout), B, H, W, tcount=2, has_part=1)
    for hint in (1, 2):
        for B, cx, C, H, Ts in params(O.test_convlstm_weight_gradient_in_partial_slots, 'B,cx,C,H,Ts'):
            one('ops::test_convlstm_weight_gradient_in_partial_slots', ('cell', cx, C, 1, 1), B, H, H, tcount=Ts[0], hint=hint, has_part=1)
        for B, cx, C, H, W in params(S.test_convlstm_weight_gradient_in_partial_slots, 'B,cx,C,H,W'):
            one('shapes::test_convlstm_weight_gradient_in_partial_slots', ('cell', cx, C, 1, 1), B, H, W, tcount=2, hint=hint, has_part=1)
    for B, cx, C, H in params(T.test_wgrad5x5_bf16_exact_on_bf16_operands, 'B,cx,C,H'):
        one('bf16::test_wgrad5x5_bf16_exact_on_bf16_operands', ('cell', cx, C, 1, 1), B, H, H, operand=BF16)
    for hint in (0, 1, 2):
        for B, cx, C, H, T_ in params(T.test_wgrad5x5_bf16_batch_of_timesteps, 'B,cx,C,H,T'):
            one('bf16::test_wgrad5x5_bf16_batch_of_timesteps', ('cell', cx, C, 1, 1), B, H, H, operand=BF16, tcount=T_, hint=hint)
    for operand in (FP16X3, BF16X6):
        for B, cx, C, H, T_ in params(T.test_wgrad5x5_fp16x3_batch_of_timesteps, 'B,cx,C,H,T'):
            one('bf16::test_wgrad5x5_fp16x3_batch_of_timesteps', ('cell', cx, C, 1, 1), B, H, H, operand=operand, tcount=T_)
        for B, cx, C, H, W in S.SERVED:
            one('shapes::test_wgrad5x5_forms', ('cell', cx, C, 1, 1), B, H, W, operand=operand, tcount=2)
    for B, cx, C, H, W in S.SERVED:
        one('shapes::test_wgrad5x5_forms', ('cell', cx, C, 1, 1), B, H, W, operand=BF16, tcount=2)
    return forms


def test_no_form_that_neither_a_layer_nor_a_gpu_case_reaches(exe):
    if not LAYER_FORMS:      # selected on its own: the grid of frames reaches what the layers reach
        test_every_operand_form_batch_partial_buffer_and_hint_on_a_grid_of_frames(exe)
    cases = gpu_case_forms(exe)
    every = set(FORM.values()) - {FORM['None']}
    orphans = sorted(NAME[f] for f in every - LAYER_FORMS - set(cases))
    assert not orphans, 'forms no product layer and no GPU case reaches: %r' % orphans
    # today every form has a GPU case of its own, the ones no product layer reaches (the 64-column slot forms: an op entry's hint) included
    assert set(cases) == every, sorted(NAME[f] for f in every - set(cases))
    assert FORM['None'] in LAYER_FORMS and {FORM['Slot5x5_8x2'], FORM['Slot5x5_16x2']} <= LAYER_FORMS      # (the grid test asks with the hints)


@pytest.mark.parametrize('B,cx,C,H,W', [(2, 32, 32, 8, 24), (2, 32, 32, 16, 40)])
def test_two_image_tiles_several_to_a_row_get_a_packed_form_that_covers_every_tile(exe, B, cx, C, H, W):
    """Maps 24 and 40 wide (lstm5 of a 64 x 192 frame, lstm1 of 128 x 80) are no multiple of 16 wide and take the 8-wide tiles of two images, three and five to
    a row -- the geometry tests/test_gpu_backward_shapes.py's SERVED runs on the GPU.  Every packed operand form must answer with an 8-wide Packed form whose
    pixel splits cover the (B / 2) (H / 8) (W / 8) T tiles of the launch, none of them empty."""
    for operand in (BF16, BF16X6, FP16X3):
        for T in (1, 2, 4):
            for hint in ((0, 1, 2) if operand == BF16 else (0,)):
                for has_h in (1, 0):
                    got = ask(exe, 256, operand, T, hint, 0, 0, ('cell', cx, C, has_h, 1), [B], [(H, W)])[0][0]
                    assert got == ref_launch(cell_shape(cx, C, has_h, B, H, W), operand, T, hint, hint, 0, 0, 256), (operand, T, hint, has_h, got)
                    form, gy, tps = NAME[got[0]], got[2], got[5]
                    n_tiles = (B // 2) * (H // 8) * (W // 8) * T
                    assert form.startswith('Packed') and form.endswith('_8'), (operand, T, hint, form)
                    assert gy * tps >= n_tiles > (gy - 1) * tps, (operand, T, hint, form, gy, tps, n_tiles)
        # ... and an odd batch cannot pair its images: refused, whatever the form
        assert ask(exe, 256, operand, 2, 0, 0, 0, ('cell', cx, C, 1, 1), [B + 1], [(H, W)])[0][0] == NONE


def test_the_restatement_agrees_with_the_built_library():
    """part_floats of the slot form against pivp_wgrad5x5_f32_part_floats (the larger of the launch with and without the h operand), of the 3x3 layers against
    pivp_conv_backward_part_floats: the library asks the header, the restatement is the parent's arithmetic"""
    lib = _lib.load()
    for cx, C, level in CELLS:
        for H, W in GRID + [(48, 40), (16, 64)]:
            for B in (1, 2, 3, 8, 31, 32, 64):
                for hint in (0, 1, 2):
                    h, w = H // level, W // level
                    want = 0
                    if wp_ok_shape(cell_shape(cx, C, 1, B, h, w)):
                        want = max(ref_launch(cell_shape(cx, C, has_h, B, h, w), F32, 1, hint, hint, 0, 1, 256)[6] for has_h in (1, 0))
                    assert lib.pivp_wgrad5x5_f32_part_floats(cx, C, B, h, w, hint) == want, (cx, C, B, h, w, hint)
    for mode, c, ldx, ldy, level in ENCS:
        for H, W in GRID:
            for B in (1, 2, 3, 8, 31, 32, 64):
                h, w = H // level, W // level
                assert lib.pivp_conv_backward_part_floats(mode, c, c, B, h, w) == ref_launch(enc_shape(mode, c, c, c, B, h, w), F32, 1, 0, 0, 0, 1, 256)[6], (mode, c, B, h, w)
    for mode, B, cin, cout, H, W in [(1, 2, 32, 32, 4, 16), (0, 2, 32, 32, 12, 16), (0, 2, 32, 64, 8, 16), (1, 2, 64, 32, 4, 8)]:      # generic planes; cin != cout
        assert lib.pivp_conv_backward_part_floats(mode, cin, cout, B, H, W) == ref_launch(enc_shape(mode, cin, cin, cout, B, H, W, cout), F32, 1, 0, 0, 0, 1, 256)[6]


def test_slot_entries_refuse_widths_the_sizing_never_checked():
    """pivp_wgrad5x5_f32_batch (part != NULL) and pivp_wgrad5x5_f32_reduce take cx and C unchecked and size the slot buffer first: a width of zero or less on
    a map the slot form does not serve is PIVP_ERR_BADARG, as it was when the sizing asked wgrad5x5p_ok before anything else -- in front of every launch, so
    this runs without a device (the pointers are never read).  And the header's grid rules answer such a shape instead of dividing by its tile count."""
    import ctypes
    lib = _lib.load()
    buf = (ctypes.c_float * 16)()
    p = ctypes.addressof(buf)
    for cx, C, B, H, W in [(32, 0, 2, 6, 8), (32, -15, 2, 6, 8), (32, 0, 2, 12, 20), (0, 0, 2, 9, 8), (-32, 32, 2, 6, 8)]:
        for form in (0, 1, 2):
            assert lib.pivp_wgrad5x5_f32_batch(p, cx, cx, p, C, p, p, 1, p, p, B, H, W, 1, 0, 0, 0, form, None) == -1, (cx, C, B, H, W, form)
            assert lib.pivp_wgrad5x5_f32_reduce(cx, C, 1, p, p, p, B, H, W, form, None) == -1, (cx, C, B, H, W, form)
