"""The launch forms of the plain convolutions, as one table: every row names an op, a shape, its strides and the form the launcher must take for it
(csrc/conv_form.h; include/pivp_conv_forms.h exports it as pivp_conv_form / pivp_conv_enc0_form).  tests/test_conv_forms_host.py holds the rows to the
header and the forms the model's layers reach to the rows; tests/test_gpu_conv_forms.py runs every row against the float64 oracle.  No torch here.

The shapes are the smallest found on each side of each threshold of the dispatcher:
  igemm_small (32-anchor tiles) takes ntb = 3 / 2 column tiles per block once ceil(M / 32) * (cout / 32 / ntb) * phases >= 1024, else 1;
  the transposed conv's tile kernel takes maps of 8 x 16 input patches with at least 16 blocks;
  the main kernel's tiles (f32_*) serve K > 40 chunks (cin >= 160 for a 3x3 conv) once 128-row tiles alone give >= 128 blocks, and whatever
  igemm_small cannot store (a bias or output that is not 16-byte aligned)."""
from collections import namedtuple

# PIVP_CONV_FORM_* / PIVP_ENC0_FORM_* (include/pivp_conv_forms.h)
FORM = {'deconv_tile': 1, 'long_k_dgrad': 2, 'small1': 11, 'small2': 12, 'small3': 13, 'f32_128x32': 21, 'f32_128x64': 22, 'f32_128x96': 23,
        'f32_128x128': 24, 'f32_64x64': 25, 'f32_64x128': 26, 'f32_32x128': 27}
ENC0_FORM = {'rows': 1, 'generic': 2}

# op: 'conv' (3x3 stride 2) / 'deconv' (transposed 3x3 stride 2) on a B x cin x H x W input to cout channels.  relus: the ReLU settings to run.
# bias_off: floats the bias pointer is moved off its 16-byte alignment.  group: rows of one group share their input (and one float64 reference).
Case = namedtuple('Case', 'op B cin H W cout form relus bias_off group note')


def _c(op, B, cin, H, W, cout, form, relus=(True,), bias_off=0, group=None, note=''):
    return Case(op, B, cin, H, W, cout, form, tuple(relus), bias_off, group, note)


BOTH = (True, False)
CONV_CASES = [
    _c('conv', 3, 32, 10, 6, 32, 'small1', BOTH, note='M = 45: one full and one partial tile'),
    _c('conv', 8, 32, 128, 128, 64, 'small2', BOTH, note='exactly at mblk = 1024'),
    _c('conv', 8, 32, 128, 126, 64, 'small1', note='just under the threshold'),
    _c('conv', 7, 32, 130, 146, 64, 'small2', group='c7', note='partial last tile'),
    _c('conv', 8, 32, 120, 140, 96, 'small3', BOTH),
    _c('conv', 7, 32, 130, 146, 96, 'small3', group='c7', note='partial last tile'),
    # K = 45 chunks: the main kernel's tiles, with a bias and a ReLU
    _c('conv', 4, 160, 128, 128, 32, 'f32_128x32', BOTH, group='k160'),
    _c('conv', 4, 160, 128, 128, 64, 'f32_64x64', group='k160'),
    _c('conv', 4, 160, 128, 128, 96, 'f32_128x32', group='k160', note='three column blocks'),
    _c('conv', 4, 160, 128, 128, 128, 'f32_64x128', group='k160'),
    # a bias that is not 16-byte aligned: igemm_small cannot add it as float4 rows
    _c('conv', 2, 32, 32, 32, 32, 'f32_128x32', BOTH, bias_off=1, note='unaligned fallback'),
    # ... which also reaches the main kernel's remaining tiles at a short K (beyond the issue's rows: every tile of the tail has a row)
    _c('conv', 3, 32, 10, 6, 32, 'f32_128x32', bias_off=1, note='M = 45: a 128-row tile with 45 rows'),
    _c('conv', 2, 32, 32, 32, 128, 'f32_32x128', bias_off=1),
    _c('conv', 8, 32, 128, 128, 64, 'f32_128x64', bias_off=1, group='u8'),
    _c('conv', 8, 32, 128, 128, 96, 'f32_128x96', bias_off=1, group='u8'),
    _c('conv', 8, 32, 128, 128, 128, 'f32_128x128', bias_off=1, group='u8'),
]
DECONV_CASES = [
    _c('deconv', 3, 64, 48, 60, 64, 'small2', BOTH),
    _c('deconv', 3, 64, 48, 56, 64, 'small1'),
    _c('deconv', 3, 96, 48, 60, 96, 'small3'),
    _c('deconv', 2, 128, 36, 60, 128, 'small2', note='nt = 4: two column blocks'),
    _c('deconv', 3, 64, 50, 55, 64, 'small2', note='M % 32 = 26'),
    _c('deconv', 1, 64, 32, 32, 64, 'deconv_tile', BOTH, note='exactly 16 blocks'),
    _c('deconv', 1, 64, 24, 32, 64, 'small1', note='12 blocks: too few for the tile kernel'),
]
CASES = CONV_CASES + DECONV_CASES

# enc0 on B x 3 x H x W frames.  (32 x 128: the row kernel's W/2 = 64 form does not exist -- its 5-row patch of 131 columns needs more than the four patch rows a
# thread stages -- so every 128-wide frame takes the generic kernel, whatever the launcher's list of widths says.)
Enc0Case = namedtuple('Enc0Case', 'B H W form note')
ENC0_CASES = [
    Enc0Case(3, 16, 16, 'rows', 'W/2 = 8: eight output rows per block'),
    Enc0Case(3, 32, 32, 'rows', 'W/2 = 16'),
    Enc0Case(3, 64, 64, 'rows', 'W/2 = 32 (the product frame)'),
    Enc0Case(3, 32, 128, 'generic', 'W/2 = 64: the row kernel cannot stage its patch'),
    Enc0Case(3, 72, 40, 'generic', '2,160 pixels: a partial last block'),
    Enc0Case(3, 24, 16, 'generic', 'H/2 = 12 is no multiple of the 8 rows of a block'),
]

# the five layers that go through igemm_conv, as the plan calls them on an H x W frame: (name, op, cin = cout, frame divisor of the INPUT map)
LAYERS = (('enc1', 'conv', 32, 2), ('enc2', 'conv', 64, 4), ('enc4', 'deconv', 128, 8), ('enc5', 'deconv', 96, 4), ('enc6', 'deconv', 64, 2))


def small_ntb(form):
    return {'small1': 1, 'small2': 2, 'small3': 3}[form]


def partials_per_sample(op, form, cout, H, W):
    """LayerNorm partials per sample the producer's epilogue reports for an H x W INPUT map (0: none), by the launchers' own formulas:
    igemm_small one per block when no 32-anchor tile straddles two samples, the transposed conv's tile kernel one per 8 x 16 patch and column tile,
    the main kernel one per block tile, enc0's row kernel one per block of 64 pixels."""
    nt = cout // 32
    if op == 'enc0':
        return (H // 2) * (W // 2) // 64 if form == 'rows' else 0
    anchors, phases = ((H // 2) * (W // 2), 1) if op == 'conv' else (H * W, 4)
    if form == 'deconv_tile':
        return (H // 8) * (W // 16) * nt
    if form.startswith('small'):
        return anchors // 32 * (nt // small_ntb(form)) * phases if anchors % 32 == 0 else 0
    bm, bn = (int(v) for v in form[4:].split('x'))
    return anchors // bm * (cout // bn) * phases if anchors % bm == 0 else 0
