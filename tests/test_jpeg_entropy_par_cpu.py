"""The parallel entropy decoder's host half (csrc/jpeg_entropy_par.h through rart_jpeg_scan_plan / rart_jpeg_entropy_emulate), no
GPU: the emulation of the device's rounds, prefix sums and write pass returns the status and the coefficients of the sequential
decoder rart_jpeg_entropy_decode (which test_jpeg_reader_cpu.py holds to Pillow) element for element; the round cap gives a status,
never a guess; the entries refuse bad arguments before any launch; malformed input never reads or writes out of bounds."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import _jpeg_decode_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, UNSUPPORTED, WORKSPACE = 0, 1, 2, 3
NEW = ['rart_jpeg_scan_plan', 'rart_jpeg_entropy_workspace_bytes', 'rart_jpeg_entropy_decode_gpu', 'rart_jpeg_entropy_emulate']


def test_new_symbols_are_declared_exported_and_bound():
    from robustart_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'robustart_hip.h')).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r'\b%s\s*\(' % name, src), name
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES and getattr(_lib.load(), name).argtypes is not None, name
    assert ctypes.sizeof(_lib.JpegScan) == 128
    for macro, value in (('RART_JPEG_DEFAULT_SUBSEQ_BYTES', _lib.JPEG_DEFAULT_SUBSEQ_BYTES),
                         ('RART_JPEG_DEFAULT_MAX_ROUNDS', _lib.JPEG_DEFAULT_MAX_ROUNDS), ('RART_JPEG_MAX_SUBSEQ', _lib.JPEG_MAX_SUBSEQ),
                         ('RART_JPEG_MAX_TABLES', _lib.JPEG_MAX_TABLES), ('RART_JPEG_HUFF_PITCH', _lib.JPEG_HUFF_PITCH)):
        assert re.search(r'#define %s %d\b' % (macro, value), src), macro
    assert _lib.load().rart_version() == _lib.ABI_VERSION == 110


def _good():
    from robustart_amd.noise.imagenet_s import jpeg_probe, jpeg_scan_plan
    data = R.encode(R.source_array(17, 23, 'noise'), '420')
    info = jpeg_probe(data)
    scan, tabs = jpeg_scan_plan(data, info)
    return data, info, scan, tabs


def test_entries_refuse_bad_arguments_before_any_launch():
    """null pointers, a subseq_bytes that is no power of two or below 4, a staging region one byte short, a workspace one byte
    short: all decided on the host copy of the descriptors (no GPU here, and no pointer is ever dereferenced)"""
    from robustart_amd import _lib
    lib = _lib.load()
    data, info, scan, tabs = _good()
    one = ctypes.c_void_p(4096)          # stands for a device buffer: never dereferenced, the checks run first
    s = (_lib.JpegScan * 1)()
    ctypes.memmove(ctypes.addressof(s), ctypes.addressof(scan), 128)
    host = ctypes.addressof(s)
    nblk = info.coef_count // 64
    ws = lib.rart_jpeg_entropy_workspace_bytes(host, 1)
    assert ws > 0 and ws % 256 == 0 and lib.rart_jpeg_entropy_workspace_bytes(None, 1) == 0
    ntab = scan.ntab * _lib.JPEG_HUFF_PITCH

    def call(dev=one, hst=host, n=1, scans=one, scans_bytes=scan.scan_len, tabs_=one, tabs_bytes=ntab, coef=one, blocks=nblk, sb=0, mr=0,
             status=one, rounds=one, wsp=one, ws_bytes=ws):
        return lib.rart_jpeg_entropy_decode_gpu(dev, hst, n, scans, scans_bytes, tabs_, tabs_bytes, coef, blocks, sb, mr, status, rounds, wsp,
                                                ws_bytes, None)

    for kw in (dict(dev=None), dict(hst=None), dict(scans=None), dict(tabs_=None), dict(coef=None), dict(status=None), dict(rounds=None)):
        assert call(**kw) == INVALID and b'bad arguments' in lib.rart_last_error_string(), kw
    assert call(n=0) == INVALID and b'descriptor count' in lib.rart_last_error_string()
    for sb in (3, 2, 1, 6, 48, 100, -4):
        assert call(sb=sb) == INVALID and b'power of two' in lib.rart_last_error_string(), sb
    assert call(mr=-1) == INVALID and b'max_rounds' in lib.rart_last_error_string()
    assert call(scans_bytes=scan.scan_len - 1) == INVALID and b'scan bytes outside' in lib.rart_last_error_string()
    assert call(tabs_bytes=ntab - 1) == INVALID and b'tables outside' in lib.rart_last_error_string()
    assert call(blocks=nblk - 1) == INVALID and b'blocks outside' in lib.rart_last_error_string()
    assert call(wsp=None) == WORKSPACE and call(ws_bytes=ws - 1) == WORKSPACE and b'workspace' in lib.rart_last_error_string()
    assert call(sb=64) == INVALID and b'nsub' in lib.rart_last_error_string()          # planned at the default, called at 64
    s[0].dc_tab[1] = scan.ntab
    assert call() == INVALID and b'table index' in lib.rart_last_error_string()
    s[0].dc_tab[1] = scan.dc_tab[1]
    s[0].sub_start = 1
    assert call() == INVALID and b'sub_start' in lib.rart_last_error_string()
    # the plan and the emulation
    sc = _lib.JpegScan()
    tb = (ctypes.c_ubyte * ntab)()
    assert lib.rart_jpeg_scan_plan(None, 0, ctypes.byref(info), 0, ctypes.byref(sc), tb, ntab) == INVALID
    assert lib.rart_jpeg_scan_plan(data, len(data), ctypes.byref(info), 12, ctypes.byref(sc), tb, ntab) == INVALID
    assert lib.rart_jpeg_scan_plan(data, len(data), ctypes.byref(info), 0, ctypes.byref(sc), tb, ntab - 1) == INVALID
    assert lib.rart_jpeg_scan_plan(data, len(data), ctypes.byref(info), 0, ctypes.byref(sc), tb, ntab) == OK
    assert lib.rart_jpeg_scan_plan(b'not a jpeg', 10, ctypes.byref(info), 0, ctypes.byref(sc), tb, ntab) == UNSUPPORTED
    coef = np.full(info.coef_count, 12345, np.int16)
    used = ctypes.c_int32(0)
    for sb in (3, 2, 24):
        assert lib.rart_jpeg_entropy_emulate(data, len(data), ctypes.byref(info), sb, 0, coef.ctypes.data, coef.size, ctypes.byref(used)) == INVALID
    assert lib.rart_jpeg_entropy_emulate(data, len(data), ctypes.byref(info), 0, 0, None, coef.size, ctypes.byref(used)) == INVALID
    assert lib.rart_jpeg_entropy_emulate(data, len(data), ctypes.byref(info), 0, 0, coef.ctypes.data, coef.size - 1, ctypes.byref(used)) == INVALID
    assert (coef == 12345).all()


def test_plan_reports_the_scan_the_tables_and_the_geometry():
    from robustart_amd import _lib
    data, info, scan, tabs = _good()
    assert scan.host_path == 0 and scan.ncomp == 3 and (scan.h_samp, scan.v_samp) == (2, 2) and (scan.mcux, scan.mcuy) == (2, 2)
    assert list(scan.blocks_w) == list(info.blocks_w) and list(scan.blocks_h) == list(info.blocks_h)
    assert data[scan.scan_pos - 14:scan.scan_pos - 12] == b'\xff\xda'                   # SOS of three components: 2 + 12 bytes
    assert data[scan.scan_pos + scan.scan_len:] == b'\xff\xd9'                          # the scan ends at EOI
    assert scan.nsub == -(-scan.scan_len // _lib.JPEG_DEFAULT_SUBSEQ_BYTES)
    assert scan.ntab == 4 and list(scan.dc_tab) == [0, 2, 2] and list(scan.ac_tab) == [1, 3, 3]      # luma DC, AC, chroma DC, AC
    gray = R.encode(R.source_array(9, 5, 'noise'), 'gray')
    from robustart_amd.noise.imagenet_s import jpeg_probe, jpeg_scan_plan
    g, _ = jpeg_scan_plan(gray, jpeg_probe(gray), 4)
    assert (g.ncomp, g.ntab, g.mcux, g.mcuy, g.host_path) == (1, 2, 1, 2, 0) and g.nsub == -(-g.scan_len // 4)


@pytest.fixture(scope='module')
def grid():
    """[(name, data, info, sequential status, sequential coefficients)] over the 168 files of the reader's grid"""
    from robustart_amd.noise.imagenet_s import jpeg_entropy_decode, jpeg_probe
    out = []
    for name, data in R.grid_cases():
        info = jpeg_probe(data)
        coef = np.zeros(info.coef_count, np.int16)
        out.append((name, data, info, jpeg_entropy_decode(data, info, coef), coef))
    assert len(out) == 168
    return out


@pytest.mark.parametrize('subseq_bytes', [4, 8, 32, 0])
def test_emulation_equals_the_sequential_decoder_on_the_grid(grid, subseq_bytes):
    """max_rounds = subsequence count + 1 always suffices: round r makes the exits of subsequences 0 .. r - 1 final"""
    from robustart_amd.noise.imagenet_s import jpeg_entropy_emulate, jpeg_scan_plan
    bad = []
    for name, data, info, want_status, want in grid:
        scan, _ = jpeg_scan_plan(data, info, subseq_bytes)
        assert scan.host_path == (1 if '420_rst' in name else 0), name
        coef = np.full(info.coef_count, 12345, np.int16)
        status, used = jpeg_entropy_emulate(data, info, coef, subseq_bytes, scan.nsub + 1)
        if scan.host_path:
            assert (scan.nsub, scan.scan_len, scan.ntab, used) == (0, 0, 0, 0), name
        else:
            assert 1 <= used <= scan.nsub + 1, name
        if status != want_status or status != OK or not np.array_equal(coef, want):
            bad.append((name, status, used))
    assert not bad, bad


def test_round_cap_gives_a_status_never_a_guess():
    """the 17 x 23 noise 4:2:0 file at subseq_bytes 8: several rounds are needed; exactly that many suffice, one fewer is
    RART_ERR_UNSUPPORTED"""
    from robustart_amd.noise.imagenet_s import jpeg_entropy_decode, jpeg_entropy_emulate, jpeg_probe
    data = R.encode(R.source_array(17, 23, 'noise'), '420')
    info = jpeg_probe(data)
    want = np.zeros(info.coef_count, np.int16)
    assert jpeg_entropy_decode(data, info, want) == OK
    coef = np.zeros(info.coef_count, np.int16)
    status, used = jpeg_entropy_emulate(data, info, coef, 8, 10 ** 6)
    assert status == OK and used >= 3 and np.array_equal(coef, want)
    coef[:] = 12345
    assert jpeg_entropy_emulate(data, info, coef, 8, used) == (OK, used) and np.array_equal(coef, want)
    assert jpeg_entropy_emulate(data, info, coef, 8, used - 1) == (UNSUPPORTED, used - 1)


def test_truncated_and_corrupt_scans_get_the_sequential_status():
    from robustart_amd.noise.imagenet_s import jpeg_entropy_decode, jpeg_entropy_emulate, jpeg_probe, jpeg_scan_plan
    data = R.encode(R.source_array(48, 40, 'noise'), '420')
    info = jpeg_probe(data)
    scan, _ = jpeg_scan_plan(data, info)
    cut = data[:scan.scan_pos + scan.scan_len // 2]
    marker = bytearray(data)
    marker[scan.scan_pos + 40:scan.scan_pos + 42] = b'\xff\xd9'
    tail = data[:-2] + b'\x00\x00'                                   # bytes after the last block are ignored
    for name, d in (('cut', cut), ('marker', bytes(marker)), ('tail', tail)):
        want = np.zeros(info.coef_count, np.int16)
        ws = jpeg_entropy_decode(d, info, want)
        for sb in (4, 32, 0):
            coef = np.zeros(info.coef_count, np.int16)
            status, _ = jpeg_entropy_emulate(d, info, coef, sb, 10 ** 6)
            assert status == ws, (name, sb)
            assert ws != OK or np.array_equal(coef, want), (name, sb)
        assert ws == (OK if name == 'tail' else INVALID), name


def test_default_max_rounds_is_twice_the_measured_maximum():
    """the largest rounds_used at the default subseq_bytes over the grid and the two 375 x 500 quality-90 files of
    profiles/jpeg_reader_ab.py, times two"""
    from robustart_amd import _lib
    from robustart_amd.noise.imagenet_s import jpeg_entropy_emulate, jpeg_probe
    from PIL import Image
    import io
    files = [d for _, d in R.grid_cases()]
    for content in ('smooth', 'noise'):
        buf = io.BytesIO()
        Image.fromarray(R.source_array(375, 500, content, seed=1)).save(buf, 'JPEG', quality=90, subsampling=2)
        files.append(buf.getvalue())
    worst = 0
    for d in files:
        info = jpeg_probe(d)
        coef = np.zeros(info.coef_count, np.int16)
        status, used = jpeg_entropy_emulate(d, info, coef, 0, 10 ** 6)
        assert status == OK
        worst = max(worst, used)
    assert _lib.JPEG_DEFAULT_MAX_ROUNDS == 2 * worst


def test_malformed_input_under_sanitizers_as_a_stand_alone_program(tmp_path):
    """every prefix truncation and every single-byte overwrite (0x00 / 0xFF / 0xD0 / complement) of the first 256 scan bytes of a
    17 x 23 4:2:0 file, at subseq_bytes 4 and 32, through a g++ -fsanitize=address,undefined build of
    tests/host/jpeg_entropy_par_fuzz.cpp: the emulation's status is the sequential decoder's, the coefficients too when both are OK"""
    src = os.path.join(ROOT, 'tests', 'host', 'jpeg_entropy_par_fuzz.cpp')
    exe = str(tmp_path / 'jpeg_entropy_par_fuzz')
    r = subprocess.run(['g++', '-std=c++17', '-g', '-O1', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', src, '-o', exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    jpg = tmp_path / 'in.jpg'
    jpg.write_bytes(R.encode(R.source_array(17, 23, 'noise'), '420'))
    r = subprocess.run([exe, str(jpg)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'ERROR' not in r.stderr and 'runtime error' not in r.stderr, r.stderr
    assert r.stdout.startswith('runs '), r.stdout


def test_entropy_keyword_is_validated_without_a_gpu(tmp_path):
    from robustart_amd.noise.imagenet_s import decode_batch_gpu
    from robustart_amd.train.cls_solver import FileImageNet
    with pytest.raises(ValueError, match='entropy'):
        decode_batch_gpu([b''], entropy='x')
    (tmp_path / 'c0').mkdir()
    with pytest.raises(ValueError, match='entropy'):
        FileImageNet.from_folder(str(tmp_path), reader='hip', entropy='x')
    assert FileImageNet.from_folder(str(tmp_path), reader='hip').entropy == 'host'
    assert FileImageNet.from_folder(str(tmp_path), reader='hip', entropy='gpu').entropy == 'gpu'
