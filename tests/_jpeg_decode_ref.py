"""numpy restatement of the JPEG reader's device stage (dequantise, libjpeg's ISLOW integer IDCT, its upsampling rules, YCbCr -> RGB)
and the grid of Pillow-written files the reader's tests share.  Written from the specification in DESIGN.md 4.5.3, not from the
kernels: coefficients + tables in, the RGB image Pillow would return out."""
import io

import numpy as np

SIZES = [(8, 8), (16, 16), (17, 23), (37, 53), (31, 33), (48, 40), (1, 1), (2, 3), (9, 5), (24, 3), (5, 40), (65, 47)]   # (h, w)
CONTENTS = ['noise', 'smooth']
# encoder settings: name -> (mode, Image.save keyword arguments)
SETTINGS = {
    '444': ('RGB', dict(subsampling=0, quality=75)),
    '422': ('RGB', dict(subsampling=1, quality=75)),
    '420': ('RGB', dict(subsampling=2, quality=75)),
    '420_rst': ('RGB', dict(subsampling=2, quality=75, restart_marker_blocks=2)),
    '420_opt_q30': ('RGB', dict(subsampling=2, quality=30, optimize=True)),
    'gray': ('L', dict(quality=75)),
    '420_q95': ('RGB', dict(subsampling=2, quality=95)),
}

F_0_298, F_0_390, F_0_541, F_0_765, F_0_899, F_1_175 = 2446, 3196, 4433, 6270, 7373, 9633
F_1_501, F_1_847, F_1_961, F_2_053, F_2_562, F_3_072 = 12299, 15137, 16069, 16819, 20995, 25172


def source_array(h, w, content, seed=0):
    """seeded HxWx3 uint8 content: uniform noise, or a smooth colour ramp with a little noise"""
    rs = np.random.RandomState(seed * 7919 + h * 131 + w)
    if content == 'noise':
        return rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    base = np.stack([255 * xx / max(w - 1, 1), 255 * yy / max(h - 1, 1), 128 + 100 * np.sin(xx / 7.0 + yy / 5.0)], -1)
    return np.clip(base + rs.normal(0, 3, base.shape), 0, 255).astype(np.uint8)


def encode(arr, setting):
    """HxWx3 uint8 -> JPEG bytes under SETTINGS[setting]"""
    from PIL import Image
    mode, kw = SETTINGS[setting]
    img = Image.fromarray(arr)
    if mode == 'L':
        img = img.convert('L')
    buf = io.BytesIO()
    img.save(buf, 'JPEG', **kw)
    return buf.getvalue()


def pillow_rgb(data):
    from PIL import Image
    with Image.open(io.BytesIO(data)) as img:
        return np.array(img.convert('RGB'))


def grid_cases(contents=CONTENTS):
    """[(id, jpeg bytes)] over SIZES x contents x SETTINGS"""
    out = []
    for h, w in SIZES:
        for content in contents:
            for s in SETTINGS:
                out.append(('%dx%d-%s-%s' % (h, w, content, s), encode(source_array(h, w, content), s)))
    return out


def _ds(x, n):
    return (x + (1 << (n - 1))) >> n


def _idct_pass(x, sh):
    """jidctint.c, one 1-D pass along axis 0 of an (8, ...) int64 array, descaled by sh"""
    x0, x1, x2, x3, x4, x5, x6, x7 = [x[i] for i in range(8)]
    z1 = (x2 + x6) * F_0_541
    t2, t3 = z1 - x6 * F_1_847, z1 + x2 * F_0_765
    t0, t1 = (x0 + x4) << 13, (x0 - x4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a0, a1, a2, a3 = x7, x5, x3, x1
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = (z3 + z4) * F_1_175
    a0, a1, a2, a3 = a0 * F_0_298, a1 * F_2_053, a2 * F_3_072, a3 * F_1_501
    z1, z2 = z1 * -F_0_899, z2 * -F_2_562
    z3, z4 = z3 * -F_1_961 + z5, z4 * -F_0_390 + z5
    a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
    return np.stack([_ds(t10 + a3, sh), _ds(t11 + a2, sh), _ds(t12 + a1, sh), _ds(t13 + a0, sh),
                     _ds(t13 - a0, sh), _ds(t12 - a1, sh), _ds(t11 - a2, sh), _ds(t10 - a3, sh)])


def plane_from_coef(coef, qt, bh, bw):
    """coef: int16 [bh * bw * 64] (block-row-major, natural order), qt [64] -> uint8 plane [bh * 8][bw * 8]"""
    b = coef.reshape(bh * bw, 8, 8).astype(np.int64) * np.asarray(qt, np.int64).reshape(1, 8, 8)
    b = _idct_pass(b.transpose(1, 0, 2), 11).transpose(1, 0, 2)          # columns: along the row index
    b = _idct_pass(b.transpose(2, 0, 1), 18).transpose(1, 2, 0)          # rows: along the column index
    b = np.clip(b + 128, 0, 255).astype(np.uint8)
    return b.reshape(bh, bw, 8, 8).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


def _h2v1(p):
    """fancy h2v1 of a (dh, dw) plane, dw > 2 -> (dh, 2 dw)"""
    p = p.astype(np.int64)
    left, right = np.concatenate([p[:, :1], p[:, :-1]], 1), np.concatenate([p[:, 1:], p[:, -1:]], 1)
    even, odd = (3 * p + left + 1) >> 2, (3 * p + right + 2) >> 2
    even[:, 0], odd[:, -1] = p[:, 0], p[:, -1]
    return np.stack([even, odd], -1).reshape(p.shape[0], -1)


def _h2v2(p):
    """fancy h2v2 of a (dh, dw) plane, dw > 2 -> (2 dh, 2 dw)"""
    p = p.astype(np.int64)
    dh = p.shape[0]
    rows = []
    for y in range(2 * dh):
        cy = y >> 1
        far = min(cy + 1, dh - 1) if y & 1 else max(cy - 1, 0)
        cs = 3 * p[cy] + p[far]
        left, right = np.concatenate([cs[:1], cs[:-1]]), np.concatenate([cs[1:], cs[-1:]])
        even, odd = (3 * cs + left + 8) >> 4, (3 * cs + right + 7) >> 4
        even[0], odd[-1] = (4 * cs[0] + 8) >> 4, (4 * cs[-1] + 7) >> 4
        rows.append(np.stack([even, odd], -1).reshape(-1))
    return np.stack(rows)


def upsample(plane, h, w, hs, vs):
    """a chroma plane (padded) -> (h, w) under luma sampling (hs, vs): the real extent ceil(w / hs) x ceil(h / vs) is cut out first"""
    dw, dh = -(-w // hs), -(-h // vs)
    p = plane[:dh, :dw]
    if hs == 1:
        return p[:h, :w].astype(np.int64)
    if dw <= 2:
        up = np.repeat(p, 2, 1)
        up = np.repeat(up, 2, 0) if vs == 2 else up
    else:
        up = _h2v2(p) if vs == 2 else _h2v1(p)
    return up[:h, :w].astype(np.int64)


def _fix(x):
    return int(x * 65536.0 + 0.5)


def decode_from_coef(info, coef):
    """info: the probe result (height, width, ncomp, h_samp, v_samp, blocks_w, blocks_h, qt), coef: the int16 array of
    rart_jpeg_entropy_decode -> the HxWx3 uint8 RGB image"""
    h, w, nc = info.height, info.width, info.ncomp
    planes, off = [], 0
    for c in range(nc):
        bw, bh = info.blocks_w[c], info.blocks_h[c]
        planes.append(plane_from_coef(coef[off:off + bw * bh * 64], np.array(info.qt[c][:]), bh, bw))
        off += bw * bh * 64
    y = planes[0][:h, :w].astype(np.int64)
    if nc == 1:
        return np.repeat(y[:, :, None], 3, 2).astype(np.uint8)
    hs, vs = info.h_samp[0], info.v_samp[0]
    cb, cr = upsample(planes[1], h, w, hs, vs) - 128, upsample(planes[2], h, w, hs, vs) - 128
    half = 32768
    r = y + ((_fix(1.40200) * cr + half) >> 16)
    b = y + ((_fix(1.77200) * cb + half) >> 16)
    g = y + ((-_fix(0.34414) * cb + half - _fix(0.71414) * cr) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)
