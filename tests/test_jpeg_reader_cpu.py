"""Host half of the JPEG reader (csrc/jpeg_entropy.h through rart_jpeg_probe / rart_jpeg_entropy_decode), no GPU: the coefficients
it produces, taken through the numpy restatement of the device stage (_jpeg_decode_ref.py), equal Pillow bit for bit; files outside the
supported set are refused without touching the coefficient buffer; malformed input never reads or writes out of bounds."""
import io
import os
import subprocess

import numpy as np
import pytest
from PIL import Image

import _jpeg_decode_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, UNSUPPORTED = 0, 2


def test_entropy_decoder_and_the_numpy_device_stage_equal_pillow_on_the_grid():
    """12 sizes x 2 contents x 7 encoder settings = 168 files"""
    from robustart_amd.noise.imagenet_s import jpeg_entropy_decode, jpeg_probe
    cases = R.grid_cases()
    assert len(cases) == 168
    bad = []
    for name, data in cases:
        info = jpeg_probe(data)
        assert info.status == OK, name
        coef = np.full(info.coef_count, 12345, np.int16)
        assert jpeg_entropy_decode(data, info, coef) == OK, name
        if not np.array_equal(R.decode_from_coef(info, coef), R.pillow_rgb(data)):
            bad.append(name)
    assert not bad, bad


def test_probe_reports_sizes_samplings_block_grids_and_tables():
    from robustart_amd.noise.imagenet_s import jpeg_probe
    info = jpeg_probe(R.encode(R.source_array(37, 53, 'noise'), '420'))
    assert (info.status, info.height, info.width, info.ncomp) == (OK, 37, 53, 3)
    assert list(info.h_samp) == [2, 1, 1] and list(info.v_samp) == [2, 1, 1]
    assert list(info.blocks_w) == [8, 4, 4] and list(info.blocks_h) == [6, 3, 3]            # 4 x 3 MCUs of 16 x 16
    assert info.coef_count == 64 * (48 + 12 + 12)
    with Image.open(io.BytesIO(R.encode(R.source_array(37, 53, 'noise'), '420'))) as img:
        zigzag = img.quantization                   # Pillow hands the tables out in natural order since 8.3
    assert list(info.qt[0]) == list(zigzag[0]) and list(info.qt[1]) == list(zigzag[1]) == list(info.qt[2])
    gray = jpeg_probe(R.encode(R.source_array(9, 5, 'noise'), 'gray'))
    assert (gray.ncomp, list(gray.blocks_w)[:1], list(gray.blocks_h)[:1], gray.coef_count) == (1, [1], [2], 128)
    s422 = jpeg_probe(R.encode(R.source_array(17, 23, 'noise'), '422'))
    assert list(s422.blocks_w) == [4, 2, 2] and list(s422.blocks_h) == [3, 3, 3]


def _save(arr, fmt='JPEG', mode=None, **kw):
    img = Image.fromarray(arr)
    if mode:
        img = img.convert(mode)
    buf = io.BytesIO()
    img.save(buf, fmt, **kw)
    return buf.getvalue()


def test_unsupported_files_are_refused_and_leave_the_coefficients_unwritten():
    """progressive, CMYK, an RGB file with Adobe transform 0, a PNG.  Pillow refuses to chroma-subsample an RGB-stored file
    (keep_rgb with subsampling raises OSError), so the transform-0 file is 4:4:4."""
    from robustart_amd.noise.imagenet_s import jpeg_entropy_decode, jpeg_probe
    arr = R.source_array(37, 53, 'smooth')
    files = {'progressive': _save(arr, progressive=True, subsampling=2),
             'cmyk': _save(arr, mode='CMYK'),
             'adobe_rgb': _save(arr, keep_rgb=True),
             'png': _save(arr, 'PNG')}
    assert b'Adobe' in files['adobe_rgb'] and b'JFIF' not in files['adobe_rgb']
    for name, data in files.items():
        info = jpeg_probe(data)
        assert info.status == UNSUPPORTED, name
        coef = np.full(4096, 12345, np.int16)
        assert jpeg_entropy_decode(data, info, coef) == UNSUPPORTED, name
        assert (coef == 12345).all(), name
    # a supported file under an info that is not its own, or with too little room, is an error and writes nothing either
    good = R.encode(arr, '420')
    info = jpeg_probe(good)
    coef = np.full(info.coef_count - 1, 12345, np.int16)
    assert jpeg_entropy_decode(good, info, coef) == 1 and (coef == 12345).all()


def test_truncated_and_corrupt_streams_are_errors_not_guesses():
    from robustart_amd.noise.imagenet_s import jpeg_entropy_decode, jpeg_probe
    data = R.encode(R.source_array(48, 40, 'noise'), '420_rst')
    info = jpeg_probe(data)
    coef = np.zeros(info.coef_count, np.int16)
    assert jpeg_entropy_decode(data, info, coef) == OK
    assert jpeg_entropy_decode(data[:len(data) // 2], info, coef) == 1
    assert jpeg_entropy_decode(data[:-2] + b'\x00\x00', info, coef) in (OK, 1)          # the EOI itself is not needed
    swapped = data.replace(b'\xff\xd0', b'\xff\xd3', 1)                                   # a restart marker out of order
    assert swapped != data and jpeg_entropy_decode(swapped, info, coef) == 1


def test_malformed_input_under_sanitizers_as_a_stand_alone_program(tmp_path):
    """every prefix truncation and every single-byte overwrite (0x00 / 0xFF / 0x7F) over the header and the first 256 scan bytes of a
    17 x 23 4:2:0 file with restart markers, through a g++ -fsanitize=address,undefined build of tests/host/jpeg_entropy_fuzz.cpp"""
    src = os.path.join(ROOT, 'tests', 'host', 'jpeg_entropy_fuzz.cpp')
    exe = str(tmp_path / 'jpeg_entropy_fuzz')
    r = subprocess.run(['g++', '-std=c++17', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', src, '-o', exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    jpg = tmp_path / 'in.jpg'
    jpg.write_bytes(R.encode(R.source_array(17, 23, 'noise'), '420_rst'))
    r = subprocess.run([exe, str(jpg)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'ERROR' not in r.stderr and 'runtime error' not in r.stderr, r.stderr
    assert r.stdout.startswith('runs '), r.stdout
