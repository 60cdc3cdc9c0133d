"""The JPEG reader on the GPU: decode_batch_gpu (host entropy decode + rart_jpeg_decode_u8) and FileImageNet(reader='hip') against
Pillow / the 'pil' reader, bit for bit."""
import ctypes
import os

import numpy as np
import pytest
import torch
from PIL import Image

import _jpeg_decode_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def mixed_batch():
    """the 12 sizes x 7 encoder settings with noise content, a 375 x 500 and a 224 x 224 4:2:0 file -> ([bytes], [Pillow's RGB])"""
    files = [data for _, data in R.grid_cases(contents=['noise'])]
    files.append(R.encode(R.source_array(375, 500, 'smooth', seed=1), '420'))
    files.append(R.encode(R.source_array(224, 224, 'noise', seed=2), '420'))
    assert len(files) == 86
    return files, [R.pillow_rgb(f) for f in files]


def test_mixed_batch_equals_pillow_in_one_launch_chain_for_1_and_8_workers(mixed_batch):
    """images of 1 x 1 up to 375 x 500, all three samplings, grayscale, restart markers and optimised tables in ONE call: every image
    equals Pillow, none falls back, rart_jpeg_decode_u8 is called once, and the worker count changes nothing"""
    from robustart_amd.noise import imagenet_s as S
    files, want = mixed_batch
    got = {}
    for workers in (1, 8):
        before = S.decode_launches
        images, used = S.decode_batch_gpu(files, num_workers=workers)
        assert S.decode_launches - before == 1
        assert len(images) == len(files) and all(used)
        bad = [k for k in range(len(files)) if images[k].dtype != torch.uint8 or not images[k].is_cuda
               or not torch.equal(images[k].cpu(), torch.from_numpy(want[k]))]
        assert not bad, ('workers %d' % workers, bad)
        got[workers] = [im.cpu() for im in images]
    assert all(torch.equal(a, b) for a, b in zip(got[1], got[8]))


def test_paths_and_fallback_items_mix_with_gpu_items(tmp_path):
    from robustart_amd.noise import imagenet_s as S
    arr = R.source_array(37, 53, 'smooth')
    p = tmp_path / 'a.jpg'
    p.write_bytes(R.encode(arr, '422'))
    prog = tmp_path / 'p.jpg'
    Image.fromarray(arr).save(str(prog), 'JPEG', progressive=True)
    images, used = S.decode_batch_gpu([str(prog), str(p), R.encode(arr, 'gray')], num_workers=2)
    assert used == [False, True, True]
    for im, src in zip(images, [str(prog), str(p), R.encode(arr, 'gray')]):
        assert torch.equal(im.cpu(), torch.from_numpy(S.decode(src, 'pil')))
    images, used = S.decode_batch_gpu([str(prog)])                  # nothing for the GPU: no launch, same result
    assert used == [False] and torch.equal(images[0].cpu(), torch.from_numpy(S.decode(str(prog), 'pil')))
    with pytest.raises(Exception):                                   # what Pillow raises propagates, as with the 'pil' reader
        S.decode_batch_gpu([b'not an image at all'])


@pytest.fixture(scope='module')
def folder(tmp_path_factory):
    """three class folders, 12 files: 10 baseline JPEGs (all samplings, one grayscale, one with restart markers), one progressive
    JPEG and one PNG"""
    root = tmp_path_factory.mktemp('jpeg_folder')
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
def test_hip_reader_equals_pil_reader_through_the_public_path(folder, transform):
    from robustart_amd.train.cls_solver import FileImageNet
    pil = FileImageNet.from_folder(folder, 64, 73, transform, reader='pil', seed=5)
    hip = FileImageNet.from_folder(folder, 64, 73, transform, reader='hip', seed=5)
    assert len(pil) == len(hip) == 12 and pil.items == hip.items
    for epoch in (0, 1):
        a, la = pil.batch(range(12), 'cuda', epoch)
        b, lb = hip.batch(range(12), 'cuda', epoch)
        assert a.shape == b.shape == (12, 64, 64, 3) and torch.equal(a, b) and torch.equal(la, lb)
    assert hip.decode_stats == {'gpu': 20, 'fallback': 4}            # two batches of 10 + 2
    assert pil.decode_stats == {'gpu': 0, 'fallback': 0}
    one = FileImageNet.from_folder(folder, 64, 73, transform, reader='hip', seed=5, num_workers=1)
    c, lc = one.batch(range(12), 'cuda')
    assert torch.equal(c, pil.batch(range(12), 'cuda')[0]) and torch.equal(lc, la)
    assert one.decode_stats == {'gpu': 10, 'fallback': 2}


def test_image_reader_type_hip_reaches_the_dataset_from_a_config(folder, tmp_path):
    from robustart_amd.train import cls_solver as S
    meta = tmp_path / 'meta.txt'
    names = sorted(os.path.join(d, f) for d in os.listdir(folder) for f in os.listdir(os.path.join(folder, d)))
    meta.write_text(''.join('%s %d\n' % (n, k) for k, n in enumerate(names)))
    dcfg = {'read_from': 'fs', 'input_size': 32, 'test_resize': 36, 'num_workers': 3,
            'test': {'root_dir': folder, 'meta_file': str(meta), 'image_reader': {'type': 'hip'}, 'transforms': {'type': 'ONECROP'}}}
    ds = S.make_dataset(dcfg, 0, 32, 'test')
    assert ds.reader == 'hip' and ds.num_workers == 3
    ref = S.make_dataset(dict(dcfg, test=dict(dcfg['test'], image_reader={'type': 'pil'})), 0, 32, 'test')
    a, la = ds.batch(range(12), 'cuda')
    b, lb = ref.batch(range(12), 'cuda')
    assert torch.equal(a, b) and torch.equal(la, lb) and ds.decode_stats == {'gpu': 10, 'fallback': 2}


def test_decode_entry_validates_before_any_launch():
    """descriptor count 0, a workspace one byte short, an output buffer one byte short: an error status and untouched buffers"""
    from robustart_amd import _lib
    from robustart_amd.noise.imagenet_s import jpeg_entropy_decode, jpeg_probe
    lib = _lib.load()
    data = R.encode(R.source_array(9, 5, 'noise'), 'gray')              # 2 blocks of one component
    info = jpeg_probe(data)
    coef = np.zeros(info.coef_count, np.int16)
    assert jpeg_entropy_decode(data, info, coef) == 0
    d = (_lib.JpegDesc * 1)()
    d[0].height, d[0].width, d[0].ncomp, d[0].h_samp, d[0].v_samp = 9, 5, 1, 1, 1
    d[0].blocks_w[0], d[0].blocks_h[0] = 1, 2
    d[0].block_start[0], d[0].block_start[1], d[0].block_start[2] = 0, 2, 2
    d[0].plane_off[0], d[0].plane_off[1], d[0].plane_off[2] = 0, 128, 128
    host = np.frombuffer(bytes(d), np.uint8)
    ddev = torch.from_numpy(host.copy()).cuda()
    cdev = torch.from_numpy(coef).cuda()
    qdev = torch.from_numpy(np.ctypeslib.as_array(info.qt).astype(np.int16).reshape(-1)).cuda()
    need = lib.rart_jpeg_decode_workspace_bytes(ctypes.addressof(d), 1)
    assert need == 256
    ws = torch.full((need,), 7, dtype=torch.uint8, device='cuda')
    out = torch.full((9 * 5 * 3,), 7, dtype=torch.uint8, device='cuda')

    def call(n, ws_bytes, out_bytes):
        return lib.rart_jpeg_decode_u8(_lib.ptr(ddev), ctypes.addressof(d), n, _lib.ptr(cdev), 2, _lib.ptr(qdev), 192, _lib.ptr(ws), ws_bytes,
                                       _lib.ptr(out), out_bytes, _lib.stream_ptr())
    assert call(0, need, out.numel()) == 1 and b'descriptor count' in lib.rart_last_error_string()
    assert call(1, need - 1, out.numel()) == 3 and b'workspace' in lib.rart_last_error_string()
    assert call(1, need, out.numel() - 1) == 1 and b'out of' in lib.rart_last_error_string()
    torch.cuda.synchronize()
    assert bool((ws == 7).all()) and bool((out == 7).all())             # nothing was launched
    assert call(1, need, out.numel()) == 0
    assert torch.equal(out.view(9, 5, 3).cpu(), torch.from_numpy(R.pillow_rgb(data)))
