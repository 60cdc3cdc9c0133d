"""Entropy decoding on the GPU (csrc/jpeg_entropy_gpu.hip): rart_jpeg_entropy_decode_gpu against its host emulation (status, rounds
and coefficients, element for element), decode_batch_gpu(entropy='gpu') and FileImageNet(entropy='gpu') against Pillow / the 'pil'
reader, bit for bit; corrupt files end as status words inside guard bands that stay intact."""
import ctypes
import os

import numpy as np
import pytest
import torch
from PIL import Image

import _jpeg_decode_ref as R

pytestmark = pytest.mark.gpu
OK, INVALID, UNSUPPORTED = 0, 1, 2
UNLIMITED = 4097                       # RART_JPEG_MAX_SUBSEQ + 1 rounds always suffice
GUARD = 4096                           # sentinel bytes on each side of a guarded buffer


def run_entry(files, subseq_bytes=0, max_rounds=0):
    """one rart_jpeg_entropy_decode_gpu call over `files` (host-path images first, as the entry demands; their coefficients come from
    the sequential decoder) with sentinel bytes around the coefficient buffer and the status / rounds arrays
    -> {file index: (status, rounds_used, coefficients, host_path)}, guards_intact"""
    from robustart_amd import _lib
    from robustart_amd.noise.imagenet_s import jpeg_entropy_decode, jpeg_probe, jpeg_scan_plan
    lib = _lib.load()
    planned = []
    for data in files:
        info = jpeg_probe(data)
        assert info.status == OK
        planned.append((data, info) + jpeg_scan_plan(data, info, subseq_bytes))
    order = sorted(range(len(files)), key=lambda k: (0 if planned[k][2].host_path else 1, k))
    m = len(order)
    scans = (_lib.JpegScan * m)()
    blk = sub = tab_bytes = scan_bytes = 0
    for j, k in enumerate(order):
        data, info, scan, _ = planned[k]
        ctypes.memmove(ctypes.addressof(scans[j]), ctypes.addressof(scan), 128)
        scans[j].block_start, scans[j].sub_start, scans[j].tab_off, scans[j].scan_off = blk, sub, tab_bytes, scan_bytes
        blk += info.coef_count // 64
        sub += scan.nsub
        tab_bytes += scan.ntab * _lib.JPEG_HUFF_PITCH
        scan_bytes += scan.scan_len                      # packed back to back: no slack behind a scan
    tabs = np.zeros(max(tab_bytes, 16), np.uint8)
    raw = np.zeros(max(scan_bytes, 16), np.uint8)
    coef = np.full(GUARD + blk * 64 + GUARD, 0x5A5A, np.int16)
    for j, k in enumerate(order):
        data, info, scan, tb = planned[k]
        s = scans[j]
        if s.host_path:
            assert jpeg_entropy_decode(data, info, coef[GUARD + s.block_start * 64:GUARD + s.block_start * 64 + info.coef_count]) == OK
        else:
            tabs[s.tab_off:s.tab_off + s.ntab * _lib.JPEG_HUFF_PITCH] = np.ctypeslib.as_array(tb)[:s.ntab * _lib.JPEG_HUFF_PITCH]
            raw[s.scan_off:s.scan_off + s.scan_len] = np.frombuffer(data, np.uint8, s.scan_len, s.scan_pos)
    d_scan = torch.from_numpy(np.frombuffer(bytes(scans), np.uint8).copy()).cuda()
    d_tabs, d_raw, d_coef = torch.from_numpy(tabs).cuda(), torch.from_numpy(raw).cuda(), torch.from_numpy(coef).cuda()
    d_stat = torch.full((GUARD // 4 + 2 * m + GUARD // 4,), 0x5A5A5A5A, dtype=torch.int32, device='cuda')
    nb = lib.rart_jpeg_entropy_workspace_bytes(ctypes.addressof(scans), m)
    ws = torch.zeros(nb, dtype=torch.uint8, device='cuda')
    st = lib.rart_jpeg_entropy_decode_gpu(_lib.ptr(d_scan), ctypes.addressof(scans), m, _lib.ptr(d_raw), scan_bytes, _lib.ptr(d_tabs), tab_bytes,
                                          d_coef.data_ptr() + 2 * GUARD, blk, subseq_bytes, max_rounds, d_stat.data_ptr() + GUARD,
                                          d_stat.data_ptr() + GUARD + 4 * m, _lib.ptr(ws), nb, _lib.stream_ptr())
    assert st == OK, lib.rart_last_error_string()
    torch.cuda.synchronize()
    coef_out, stat_out = d_coef.cpu().numpy(), d_stat.cpu().numpy()
    intact = bool((coef_out[:GUARD] == 0x5A5A).all() and (coef_out[GUARD + blk * 64:] == 0x5A5A).all() and
                  (stat_out[:GUARD // 4] == 0x5A5A5A5A).all() and (stat_out[GUARD // 4 + 2 * m:] == 0x5A5A5A5A).all())
    out = {}
    for j, k in enumerate(order):
        lo = GUARD + scans[j].block_start * 64
        out[k] = (int(stat_out[GUARD // 4 + j]), int(stat_out[GUARD // 4 + m + j]), coef_out[lo:lo + planned[k][1].coef_count],
                  bool(scans[j].host_path))
    return out, intact


def emulate(data, subseq_bytes=0, max_rounds=0):
    from robustart_amd.noise.imagenet_s import jpeg_entropy_emulate, jpeg_probe
    info = jpeg_probe(data)
    coef = np.zeros(info.coef_count, np.int16)
    status, used = jpeg_entropy_emulate(data, info, coef, subseq_bytes, max_rounds)
    return status, used, coef


@pytest.fixture(scope='module')
def noise_grid():
    cases = R.grid_cases(contents=['noise'])
    assert len(cases) == 84
    return cases


@pytest.mark.parametrize('subseq_bytes', [4, 0])
def test_grid_in_one_call_equals_the_emulation(noise_grid, subseq_bytes):
    """12 sizes (1 x 1 up to 65 x 47) x 7 encoder settings: all samplings, grayscale, optimised tables, restart markers (host path);
    at 4 bytes a block spans many subsequences and subsequences start inside FF 00 pairs"""
    files = [d for _, d in noise_grid]
    got, intact = run_entry(files, subseq_bytes, UNLIMITED)
    assert intact
    bad = []
    for k, (name, data) in enumerate(noise_grid):
        status, used, coef, host_path = got[k]
        assert host_path == ('420_rst' in name), name
        want_status, want_used, want = emulate(data, subseq_bytes, UNLIMITED)
        assert want_status == OK, name
        if (status, used) != (OK, want_used) or not np.array_equal(coef, want):
            bad.append((name, status, used, want_used, int((coef != want).sum())))
    assert not bad, bad
    if subseq_bytes == 4:
        raw = b''.join(files)
        assert b'\xff\x00' in raw                                    # stuffed bytes are in play


@pytest.fixture(scope='module')
def mixed_batch(noise_grid):
    """the 86-file batch of test_jpeg_reader_gpu.py -> ([bytes], [Pillow's RGB], the number of restart-marker files)"""
    files = [data for _, data in noise_grid]
    files.append(R.encode(R.source_array(375, 500, 'smooth', seed=1), '420'))
    files.append(R.encode(R.source_array(224, 224, 'noise', seed=2), '420'))
    assert len(files) == 86
    return files, [R.pillow_rgb(f) for f in files], sum(1 for name, _ in noise_grid if '420_rst' in name)


def _equal_pillow(images, want):
    return [k for k in range(len(want)) if images[k].dtype != torch.uint8 or not images[k].is_cuda
            or not torch.equal(images[k].cpu(), torch.from_numpy(want[k]))]


def test_mixed_batch_equals_pillow_with_one_entropy_launch_for_1_and_8_workers(mixed_batch):
    from robustart_amd.noise import imagenet_s as S
    files, want, n_rst = mixed_batch
    got = {}
    for workers in (1, 8):
        before = (S.decode_launches, S.entropy_launches, dict(S.entropy_stats))
        images, used = S.decode_batch_gpu(files, num_workers=workers, entropy='gpu')
        assert S.decode_launches - before[0] == 1 and S.entropy_launches - before[1] == 1
        delta = {k: S.entropy_stats[k] - before[2][k] for k in S.entropy_stats}
        assert delta == {'gpu': 86 - n_rst, 'host_dri': n_rst, 'host_not_converged': 0, 'invalid': 0}
        assert len(images) == 86 and all(used)
        assert not _equal_pillow(images, want), workers
        got[workers] = [im.cpu() for im in images]
    assert all(torch.equal(a, b) for a, b in zip(got[1], got[8]))


def test_images_that_do_not_converge_are_decoded_on_the_host(mixed_batch):
    """max_rounds one below the largest rounds_used of the batch (from the emulation): that image at least goes to the host decoder"""
    from robustart_amd.noise import imagenet_s as S
    files, want, n_rst = mixed_batch
    rounds = [emulate(f, 0, UNLIMITED)[1] for f in files]
    cap = max(rounds) - 1
    assert cap >= 1
    late = sum(1 for r in rounds if r > cap)
    before = dict(S.entropy_stats)
    images, used = S.decode_batch_gpu(files, entropy='gpu', max_rounds=cap)
    delta = {k: S.entropy_stats[k] - before[k] for k in S.entropy_stats}
    assert delta['host_not_converged'] == late >= 1 and delta['invalid'] == 0 and delta['gpu'] == 86 - n_rst - late
    assert all(used) and not _equal_pillow(images, want)


@pytest.fixture(scope='module')
def corrupt_batch():
    """six good files, one truncated in the middle of its scan, one with two scan bytes overwritten by FF D9"""
    from robustart_amd.noise.imagenet_s import jpeg_probe, jpeg_scan_plan
    good = [R.encode(R.source_array(h, w, 'noise', seed=4), s) for (h, w), s in
            (((48, 40), '420'), ((37, 53), '444'), ((65, 47), '422'), ((31, 33), 'gray'), ((17, 23), '420_opt_q30'), ((24, 35), '420_rst'))]
    victim = R.encode(R.source_array(64, 80, 'noise', seed=5), '420')
    scan, _ = jpeg_scan_plan(victim, jpeg_probe(victim))
    truncated = victim[:scan.scan_pos + scan.scan_len // 2]
    marked = bytearray(victim)
    marked[scan.scan_pos + scan.scan_len // 3:scan.scan_pos + scan.scan_len // 3 + 2] = b'\xff\xd9'
    files = good[:3] + [truncated] + good[3:5] + [bytes(marked)] + good[5:]
    return files, (3, 6)


@pytest.mark.parametrize('subseq_bytes', [4, 0])
def test_corrupt_files_are_status_words_and_the_guard_bands_stay_intact(corrupt_batch, subseq_bytes):
    from robustart_amd.noise.imagenet_s import jpeg_entropy_decode, jpeg_probe
    files, corrupt = corrupt_batch
    got, intact = run_entry(files, subseq_bytes, UNLIMITED)
    assert intact
    for k, data in enumerate(files):
        status, used, coef, host_path = got[k]
        info = jpeg_probe(data)
        want = np.zeros(info.coef_count, np.int16)
        assert jpeg_entropy_decode(data, info, want) == (INVALID if k in corrupt else OK)
        assert status == (INVALID if k in corrupt else OK), k
        assert (status, used) == emulate(data, subseq_bytes, UNLIMITED)[:2], k
        if k not in corrupt:
            assert np.array_equal(coef, want), k


def test_corrupt_files_go_through_pillow_as_under_host_entropy_decoding(corrupt_batch):
    """the others equal Pillow; each corrupt file ends as under entropy='host': the same image, or the same exception"""
    from robustart_amd.noise import imagenet_s as S
    files, corrupt = corrupt_batch
    good = [f for k, f in enumerate(files) if k not in corrupt]
    for c in corrupt:
        batch = good[:2] + [files[c]] + good[2:]
        outcome = {}
        for mode in ('host', 'gpu'):
            before = dict(S.entropy_stats)
            try:
                images, used = S.decode_batch_gpu(batch, entropy=mode)
                outcome[mode] = ('images', used, [im.cpu() for im in images])
            except Exception as e:                                   # what Pillow raises for the corrupt file propagates
                outcome[mode] = ('raised', type(e), str(e))
            if mode == 'gpu':
                assert S.entropy_stats['invalid'] - before['invalid'] == 1
        assert outcome['host'][0] == outcome['gpu'][0]
        if outcome['host'][0] == 'raised':
            assert outcome['host'][1:] == outcome['gpu'][1:]
        else:
            assert outcome['host'][1] == outcome['gpu'][1] and outcome['gpu'][1][2] is False
            assert all(torch.equal(a, b) for a, b in zip(outcome['host'][2], outcome['gpu'][2]))
    images, used = S.decode_batch_gpu(good, entropy='gpu')
    assert all(used) and not _equal_pillow(images, [R.pillow_rgb(f) for f in good])


@pytest.fixture(scope='module')
def folder(tmp_path_factory):
    """the folder of test_jpeg_reader_gpu.py: three class folders, 12 files: 10 baseline JPEGs (all samplings, one grayscale, one with
    restart markers), one progressive JPEG and one PNG"""
    root = tmp_path_factory.mktemp('jpeg_entropy_folder')
    specs = [('444', 37, 53), ('422', 65, 47), ('420', 48, 40), ('gray', 31, 33),
             ('420_rst', 100, 75), ('420_q95', 17, 23), ('420_opt_q30', 120, 90), ('422', 24, 35),
             ('420', 375, 500), ('444', 64, 64), ('progressive', 50, 70), ('png', 40, 60)]
    for k, (kind, h, w) in enumerate(specs):
        d = root / ('class%d' % (k % 3))
        d.mkdir(exist_ok=True)
        arr = R.source_array(h, w, 'smooth' if k % 2 else 'noise', seed=3)
        if kind == 'progressive':
            Image.fromarray(arr).save(str(d / ('img%02d.jpg' % k)), 'JPEG', progressive=True)
        elif kind == 'png':
            Image.fromarray(arr).save(str(d / ('img%02d.png' % k)), 'PNG')
        else:
            (d / ('img%02d.jpg' % k)).write_bytes(R.encode(arr, kind))
    return str(root)


@pytest.mark.parametrize('transform', ['ONECROP', 'STANDARD'])
def test_gpu_entropy_reader_equals_pil_reader_through_the_public_path(folder, transform):
    from robustart_amd.train.cls_solver import FileImageNet
    pil = FileImageNet.from_folder(folder, 64, 73, transform, reader='pil', seed=5)
    hip = FileImageNet.from_folder(folder, 64, 73, transform, reader='hip', seed=5, entropy='gpu')
    assert hip.entropy == 'gpu' and len(pil) == len(hip) == 12
    a, la = pil.batch(range(12), 'cuda')
    b, lb = hip.batch(range(12), 'cuda')
    assert a.shape == b.shape == (12, 64, 64, 3) and torch.equal(a, b) and torch.equal(la, lb)
    assert hip.decode_stats == {'gpu': 10, 'fallback': 2}


def test_image_reader_entropy_reaches_the_dataset_from_a_config(folder, tmp_path):
    from robustart_amd.noise import imagenet_s as NS
    from robustart_amd.train import cls_solver as S
    meta = tmp_path / 'meta.txt'
    names = sorted(os.path.join(d, f) for d in os.listdir(folder) for f in os.listdir(os.path.join(folder, d)))
    meta.write_text(''.join('%s %d\n' % (n, k) for k, n in enumerate(names)))
    dcfg = {'read_from': 'fs', 'input_size': 32, 'test_resize': 36, 'num_workers': 3,
            'test': {'root_dir': folder, 'meta_file': str(meta), 'image_reader': {'type': 'hip', 'entropy': 'gpu'},
                     'transforms': {'type': 'ONECROP'}}}
    ds = S.make_dataset(dcfg, 0, 32, 'test')
    assert (ds.reader, ds.entropy, ds.num_workers) == ('hip', 'gpu', 3)
    assert S.make_dataset(dict(dcfg, test=dict(dcfg['test'], image_reader={'type': 'hip'})), 0, 32, 'test').entropy == 'host'
    ref = S.make_dataset(dict(dcfg, test=dict(dcfg['test'], image_reader={'type': 'pil'})), 0, 32, 'test')
    before = NS.entropy_launches
    a, la = ds.batch(range(12), 'cuda')
    b, lb = ref.batch(range(12), 'cuda')
    assert NS.entropy_launches - before == 1
    assert torch.equal(a, b) and torch.equal(la, lb) and ds.decode_stats == {'gpu': 10, 'fallback': 2}
    with pytest.raises(ValueError, match='entropy'):
        S.make_dataset(dict(dcfg, test=dict(dcfg['test'], image_reader={'type': 'hip', 'entropy': 'x'})), 0, 32, 'test')


def test_a_375_x_500_file_converges_at_the_default_parameters():
    from robustart_amd import _lib
    from robustart_amd.noise import imagenet_s as S
    data = R.encode(R.source_array(375, 500, 'noise', seed=7), '420')
    got, intact = run_entry([data])
    status, used, coef, host_path = got[0]
    assert intact and not host_path and status == OK and 2 <= used <= _lib.JPEG_DEFAULT_MAX_ROUNDS
    want_status, want_used, want = emulate(data)
    assert (want_status, want_used) == (OK, used) and np.array_equal(coef, want)
    before = dict(S.entropy_stats)
    images, used_gpu = S.decode_batch_gpu([data], entropy='gpu')
    assert used_gpu == [True] and S.entropy_stats['gpu'] - before['gpu'] == 1
    assert torch.equal(images[0].cpu(), torch.from_numpy(R.pillow_rgb(data)))
