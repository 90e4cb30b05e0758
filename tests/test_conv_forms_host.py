"""The plain convolutions' launch forms (csrc/conv_form.h) on the host: a stand-alone program that includes nothing but that header is compiled for the
host and prints the form of every product layer over the whole domain the plan accepts, and of every row of tests/conv_form_cases.py.  The first is
compared with a restatement of the dispatchers as they stood inside igemm_conv / igemm_small / conv_enc0 before the header existed (so the refactor
moved no launch), and every form it reaches must have a row in the table (so a new form or a moved threshold fails here, not silently); the second
holds each row to the form it names.  Then the C-ABI surface of include/pivp_conv_forms.h against `_lib.CONV_FORMS_SIGNATURES` and the built library."""
import os
import re
import subprocess
import sys

import pytest

from pivp_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_form_cases as CF  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(os.path.dirname(_lib.LIB_PATH), 'csrc')
HS = range(16, 257, 8)       # frame heights and widths plan_serves_forward accepts: multiples of 8 from 16, W + 4 <= 256
WS = range(16, 249, 8)
BS = range(1, 65)

PROGRAM = r'''
#include <stdio.h>
#include <stdlib.h>
#include "conv_form.h"
int main(int argc, char** argv) {
    if (argc == 2 && argv[1][0] == 'l') {      // every layer over the plan's domain: layer aligned B H W form
        static const struct { int deconv, c, div; } layer[5] = {{0, 32, 2}, {0, 64, 4}, {1, 128, 8}, {1, 96, 4}, {1, 64, 2}};
        for (int l = 0; l < 5; ++l)
            for (int aligned = 0; aligned < 2; ++aligned)
                for (int B = 1; B <= 64; ++B)
                    for (int H = 16; H <= 256; H += 8)
                        for (int W = 16; W <= 248; W += 8)
                            printf("%d %d %d %d %d %d\n", l, aligned, B, H, W,
                                   (int)pivp::conv_form(layer[l].deconv, layer[l].c, layer[l].c, B, H / layer[l].div, W / layer[l].div, aligned, 0));
        return 0;
    }
    if (argc == 9 && argv[1][0] == 'c') {      // c deconv cin cout B H W aligned
        printf("%d\n", (int)pivp::conv_form(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), atoi(argv[6]), atoi(argv[7]), atoi(argv[8]), 0));
        return 0;
    }
    if (argc == 6 && argv[1][0] == 'e') {      // e B H W weights_aligned
        printf("%d\n", (int)pivp::enc0_form(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5])));
        return 0;
    }
    return 2;
}
'''


def dispatch(deconv, cin, cout, B, Hin, Win, aligned):
    """igemm_conv's choice for a 3x3 stride-2 conv / transposed conv without a K split, line by line as it stood before csrc/conv_form.h (with igemm_small's ntb)"""
    nt = cout // 32
    if deconv and Hin % 8 == 0 and Win % 16 == 0 and B * (Hin // 8) * (Win // 16) * nt >= 16:
        return 'deconv_tile'
    M, nphase = (B * Hin * Win, 4) if deconv else (B * (Hin // 2) * (Win // 2), 1)
    full = (M + 127) // 128 * nphase
    big = full * ((nt + 3) // 4)
    chunks = (4 if deconv else 9) * (cin // 32)
    if aligned and (big < 128 or chunks <= 40):
        mblk = (M + 31) // 32
        if nt % 3 == 0 and mblk * (nt // 3) * nphase >= 1024:
            return 'small3'
        if nt % 2 == 0 and mblk * (nt // 2) * nphase >= 1024:
            return 'small2'
        return 'small1'
    if nt > 4:
        if nt % 4 == 0:
            return 'f32_128x128' if full * (nt // 4) >= 256 else 'f32_64x128'
        if nt % 3 == 0:
            return 'f32_128x96'
        if nt % 2 == 0:
            return 'f32_128x64' if full * (nt // 2) >= 256 else 'f32_64x64'
        return 'f32_128x32'
    if full >= 256:
        return {1: 'f32_128x32', 2: 'f32_128x64', 3: 'f32_128x96', 4: 'f32_128x128'}[nt]
    if nt == 4 and full * 2 < 256:
        return 'f32_32x128'
    if nt == 4:
        return 'f32_64x128'
    if nt == 2 and full * 2 >= 128:
        return 'f32_64x64'
    return 'f32_128x32'


def enc0_dispatch(H, W, weights_aligned=1):
    """conv_enc0's choice, as it stood inside the launcher"""
    H2, W2 = H // 2, W // 2
    if W2 in (8, 16, 32, 64) and H2 % (64 // W2) == 0 and weights_aligned:
        rows = 64 // W2
        R = 2 * rows + 3
        if W + 3 <= 256 and R <= 4 * (256 // (W + 3)):
            return 'rows'
    return 'generic'


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp('conv_form')
    src, out = str(d / 'conv_form.cpp'), str(d / 'conv_form')
    with open(src, 'w') as f:
        f.write(PROGRAM)
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')      # the compiler build.py uses; host only: plain C++, no device code, no library
    subprocess.check_call([hipcc, '-x', 'c++', '-std=c++17', '-O1', '-Wall', '-Werror', '-I', CSRC, src, '-o', out])
    return out


@pytest.fixture(scope='module')
def layer_table(exe):
    rows = [tuple(int(v) for v in line.split()) for line in subprocess.check_output([exe, 'l']).decode().splitlines()]
    assert len(rows) == 5 * 2 * len(BS) * len(HS) * len(WS)
    return rows


def test_the_header_chooses_what_the_launchers_chose(layer_table):
    name = {v: k for k, v in CF.FORM.items()}
    for l, aligned, B, H, W, form in layer_table:
        _, op, c, div = CF.LAYERS[l]
        assert name[form] == dispatch(op == 'deconv', c, c, B, H // div, W // div, aligned), (CF.LAYERS[l], aligned, B, H, W)


def test_every_form_a_layer_reaches_has_a_row(layer_table):
    reached = {}
    for l, aligned, B, H, W, form in layer_table:
        if aligned:          # the plan's buffers are 16-byte aligned
            reached.setdefault((CF.LAYERS[l][1], form), (CF.LAYERS[l][0], B, H, W))
    covered = {(c.op, CF.FORM[c.form]) for c in CF.CASES}
    missing = {k: v for k, v in reached.items() if k not in covered}
    assert not missing, 'forms without a row in conv_form_cases (op, form): first (layer, B, H, W) that reaches it: %r' % missing
    # and the product layers really are a mix: igemm_small with every ntb and the tile kernel
    assert {f for _, f in reached} == {CF.FORM[n] for n in ('small1', 'small2', 'small3', 'deconv_tile')}
    # the thresholds the issue names: 72 x 40 frames, enc6 takes two column tiles from B = 12 and enc5 three from B = 46; 72 x 64, enc4 two from B = 57
    by = {(l, B, H, W): f for l, aligned, B, H, W, f in layer_table if aligned}
    assert [by[(4, B, 72, 40)] for B in (11, 12)] == [CF.FORM['small1'], CF.FORM['small2']]
    assert [by[(3, B, 72, 40)] for B in (45, 46)] == [CF.FORM['small1'], CF.FORM['small3']]
    assert [by[(2, B, 72, 64)] for B in (56, 57)] == [CF.FORM['small1'], CF.FORM['small2']]


def test_every_row_takes_the_form_it_names(exe):
    for c in CF.CASES:
        got = int(subprocess.check_output([exe, 'c', str(int(c.op == 'deconv')), str(c.cin), str(c.cout), str(c.B), str(c.H), str(c.W), str(int(c.bias_off == 0))]))
        assert got == CF.FORM[c.form], c
        assert c.form == dispatch(c.op == 'deconv', c.cin, c.cout, c.B, c.H, c.W, c.bias_off == 0), c
    for c in CF.ENC0_CASES:
        assert int(subprocess.check_output([exe, 'e', str(c.B), str(c.H), str(c.W), '1'])) == CF.ENC0_FORM[c.form], c
        assert c.form == enc0_dispatch(c.H, c.W), c
        assert int(subprocess.check_output([exe, 'e', str(c.B), str(c.H), str(c.W), '0'])) == CF.ENC0_FORM['generic'], c      # weights off their alignment
    # every group shares one input
    for g in {c.group for c in CF.CASES if c.group}:
        assert len({(c.op, c.B, c.cin, c.H, c.W) for c in CF.CASES if c.group == g}) == 1, g
    # the partial counts the GPU test expects, on the layers whose producers a rollout asks: enc0 at 64 x 64 in 16 row tiles, enc6 in 16 patches x 2 column tiles
    assert CF.partials_per_sample('enc0', 'rows', 32, 64, 64) == 16 and CF.partials_per_sample('deconv', 'deconv_tile', 64, 32, 32) == 16
    assert CF.partials_per_sample('deconv', 'small2', 64, 50, 55) == 0 and CF.partials_per_sample('conv', 'small3', 96, 120, 140) == 0      # 4,200 anchors
    assert CF.partials_per_sample('conv', 'small3', 96, 128, 128) == 128 and CF.partials_per_sample('conv', 'f32_64x128', 128, 128, 128) == 64


def _declared(header):
    return set(re.findall(r'\b(pivp_[a-z0-9_]+)\s*\(', open(os.path.join(ROOT, 'include', header)).read()))


def test_conv_forms_header_library_and_ctypes_table_agree():
    import __graft_entry__ as g
    from pivp_amd import _digest
    g.build()
    declared = _declared('pivp_conv_forms.h')
    exported = set(re.findall(r' T (pivp_[a-z0-9_]+)', subprocess.check_output(['nm', '-D', _lib.LIB_PATH]).decode()))
    assert declared == set(_lib.CONV_FORMS_SIGNATURES) == {'pivp_conv_form', 'pivp_conv_enc0_form', 'pivp_conv3x3s2_ln_fits', 'pivp_conv3x3s2_ln',
                                                           'pivp_conv_layernorm_scratch_floats', 'pivp_conv_layernorm'}
    assert declared <= exported
    assert not any(declared & set(table) for header, table in _lib.HEADER_SIGNATURES.items() if header != 'pivp_conv_forms.h')
    lib = _lib.load()
    assert lib.pivp_abi_version() == 17 and len(_declared('pivp_hip.h') - {'pivp_config', 'pivp_plan'}) == 118 == len(_lib.SIGNATURES)
    assert 'pivp_conv_forms.h' in [os.path.basename(p) for p in _digest.source_files()] and 'conv_form.h' in [os.path.basename(p) for p in _digest.source_files()]
    header = open(os.path.join(ROOT, 'include', 'pivp_conv_forms.h')).read()
    i, f, vp, ll = _lib._i, _lib._f, _lib._vp, _lib._ll
    for name, (res, args) in _lib.CONV_FORMS_SIGNATURES.items():
        fn = getattr(lib, name)                                                    # load() bound the new table too
        assert fn.argtypes == args and fn.restype is res
        # the header's prototype, argument by argument
        ret, proto = re.search(r'(int|long long) %s\(([^)]*)\);' % name, header).groups()
        assert res is (ll if ret == 'long long' else i), name
        kinds = ['p' if '*' in a else ('f' if a.strip().startswith('float') else 'i') for a in proto.split(',')]
        want = ['i' if a is i else 'f' if a is f else 'p' for a in args]
        assert kinds == want, name
    # the codes: the header's #defines, the ctypes module's and the table's
    codes = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r'#define PIVP_CONV_FORM_(\w+) (\d+)', header)}
    assert codes == {k.replace('small', 'small_'): v for k, v in CF.FORM.items()} and CF.FORM == _lib.CONV_FORM
    enc0 = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r'#define PIVP_ENC0_FORM_(\w+) (\d+)', header)}
    assert enc0 == CF.ENC0_FORM == _lib.ENC0_FORM
    kinds = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r'#define PIVP_CONV_KIND_(\w+) (\d+)', header)}
    assert kinds == _lib.CONV_KIND
    # the struct, field by field
    body = re.search(r'typedef struct pivp_enc3_epilogue \{(.*?)\} pivp_enc3_epilogue_t;', header, re.S).group(1)
    fields = [(m.group(2), vp if '*' in m.group(1) else i) for m in re.finditer(r'((?:const )?(?:float\*|int)) (\w+);', body)]
    assert fields == list(_lib.PivpEnc3Epilogue._fields_)


def test_the_exported_choice_is_the_header_s_and_refuses_bad_sizes():
    """pivp_conv_form / pivp_conv_enc0_form are host only: they answer on a machine without a device."""
    lib = _lib.load()
    for c in CF.CASES:
        assert lib.pivp_conv_form(int(c.op == 'deconv'), c.cin, c.cout, c.B, c.H, c.W, int(c.bias_off == 0)) == CF.FORM[c.form], c
    for c in CF.ENC0_CASES:
        assert lib.pivp_conv_enc0_form(c.B, c.H, c.W) == CF.ENC0_FORM[c.form], c
    good = dict(deconv=0, cin=32, cout=32, B=2, Hin=16, Win=16, aligned=1)
    for over in (dict(deconv=2), dict(deconv=-1), dict(cin=0), dict(cin=48), dict(cout=0), dict(cout=40), dict(B=0), dict(Hin=0), dict(Win=-2), dict(Hin=15),
                 dict(Win=7), dict(B=1 << 20, Hin=256, Win=256)):
        a = dict(good, **over)
        assert lib.pivp_conv_form(a['deconv'], a['cin'], a['cout'], a['B'], a['Hin'], a['Win'], a['aligned']) == -1, over
    assert lib.pivp_conv_form(1, 32, 32, 2, 15, 7, 1) == CF.FORM['small1']      # the transposed conv takes odd maps
    for B, H, W in ((0, 16, 16), (1, 0, 16), (1, 16, 0), (1, 15, 16), (1, 16, 18 + 1)):
        assert lib.pivp_conv_enc0_form(B, H, W) == -1
    # the LayerNorm-on-load conv's geometry: whole 32-channel chunks, even maps, 32-anchor tiles inside one sample
    fits = lib.pivp_conv3x3s2_ln_fits
    assert fits(32, 32, 3, 16, 8) == 1 and fits(64, 64, 2, 16, 16) == 1 and fits(64, 64, 8, 128, 128) == 1 and fits(32, 96, 8, 120, 140) == 0
    assert fits(32, 96, 8, 128, 140) == 1 and fits(32, 32, 3, 10, 6) == 0 and fits(48, 32, 3, 16, 8) == 0 and fits(32, 40, 3, 16, 8) == 0 and fits(32, 32, 3, 15, 8) == 0
    assert fits(0, 32, 3, 16, 8) == 0 and fits(32, 32, 0, 16, 8) == 0
    # null pointers and bad kinds are refused before anything is launched
    assert lib.pivp_conv3x3s2_ln(None, 32, None, None, None, None, 1e-6, None, None, 32, 32, 1, None, 0, None, None, 3, 16, 8, None) == -1
    assert lib.pivp_conv_layernorm(3, None, 32, 32, None, None, None, 32, 0, None, None, None, 32, None, 1e-6, 0, 2, 16, 16, None, None) == -1
    assert lib.pivp_conv_layernorm_scratch_floats(3, 32, 2, 16, 16) == -1 and lib.pivp_conv_layernorm_scratch_floats(0, 64, 2, 16, 16) == -1
    assert lib.pivp_conv_layernorm_scratch_floats(1, 32, 2, 16, 16) == 2 * 2 * 4 and lib.pivp_conv_layernorm_scratch_floats(2, 64, 1, 32, 32) == 256 * 4
