"""The batched variable-size resize without a device: the host-only plan entry, the validation rart_resize_batch_u8 does before any
launch, and the ImageNet-S loop's argument handling in cls_solver."""
import argparse
import ctypes
import json

import numpy as np
import pytest
import torch

FAKE = 1 << 20            # a non-null, 16-byte aligned "device address": nothing here dereferences it


def _descs(sizes, boxes=None):
    from robustart_amd import _lib
    d = (_lib.ResizeDesc * len(sizes))()
    for k, (h, w) in enumerate(sizes):
        d[k].src, d[k].h, d[k].w = FAKE + 4096 * k, h, w
        d[k].box_y, d[k].box_x, d[k].box_h, d[k].box_w = (boxes[k] if boxes else None) or (0, 0, h, w)
    return d


def _plan(d, f=1, target=(36, 36), crop=(2, 2, 32, 32), n=None, fill=True):
    """-> (status, header, host buffer or None)"""
    from robustart_amd import _lib
    lib = _lib.load()
    n = len(d) if n is None else n
    sizes = _lib.ResizePlan()
    st = lib.rart_resize_batch_plan(ctypes.addressof(d), n, f, target[0], target[1], *crop, None, 0, ctypes.byref(sizes))
    if st != 0 or not fill:
        return st, sizes, None
    host = np.zeros(sizes.total_bytes, np.uint8)
    st = lib.rart_resize_batch_plan(ctypes.addressof(d), n, f, target[0], target[1], *crop, host.ctypes.data, host.size, ctypes.byref(sizes))
    return st, sizes, host


def _read(host, sizes, n):
    from robustart_amd import _lib
    d = (_lib.ResizeDesc * n).from_buffer(host, sizes.desc_off)
    prefix = host[sizes.prefix_off:sizes.prefix_off + 8 * (n + 1)].view(np.int64)
    return d, prefix


def test_plan_shares_tables_between_equal_sizes():
    st, sizes, host = _plan(_descs([(33, 47), (75, 100), (33, 47), (75, 47)]), f=2)
    assert st == 0
    d, prefix = _read(host, sizes, 4)
    assert (d[0].tab_h, d[0].tab_v, d[0].ks_h, d[0].ks_v) == (d[2].tab_h, d[2].tab_v, d[2].ks_h, d[2].ks_v)
    assert d[1].tab_h != d[0].tab_h and d[1].tab_v != d[0].tab_v
    assert d[3].tab_h == d[0].tab_h and d[3].tab_v == d[1].tab_v          # a table is per (in_size, out_size), not per image
    # four distinct tables of 36 rows: 47 -> 36 and 33 -> 36 (bicubic: 7 and 5 taps), 100 -> 36 and 75 -> 36 (13 and 11 taps)
    assert sizes.table_count == 36 * ((7 + 2) + (5 + 2) + (13 + 2) + (11 + 2))
    # the first pass covers the rows the crop window's vertical taps read: more of them for the taller source
    assert [int(prefix[k + 1] - prefix[k]) for k in range(4)] == [d[k].mid_count * 32 * 3 for k in range(4)]
    assert d[1].mid_count > d[0].mid_count and prefix[0] == 0
    assert sizes.workspace_bytes == (int(prefix[4]) + 255) // 256 * 256
    assert [d[k].vfirst for k in range(4)] == [0, 0, 0, 0]


def test_plan_sizes_grow_with_n_as_documented():
    for n in (1, 2, 3, 8, 33):
        st, sizes, _ = _plan(_descs([(33, 47)] * n), fill=False)
        assert st == 0 and sizes.n == n
        assert (sizes.desc_off, sizes.prefix_off) == (80, 80 + 64 * n)
        assert sizes.table_off == sizes.prefix_off + (8 * (n + 1) + 15) // 16 * 16
        assert sizes.total_bytes == sizes.table_off + 4 * sizes.table_count
        assert sizes.table_count == 36 * ((5 + 2) + (3 + 2))                # bilinear, 47 -> 36 (5 taps) and 33 -> 36 (3): once each, whatever n
    st, sizes, host = _plan(_descs([(33, 47), (900, 7)]), f=0)              # NEAREST: index tables, no intermediate
    assert st == 0 and sizes.workspace_bytes == 0 and sizes.table_count == 4 * 36
    d, prefix = _read(host, sizes, 2)
    assert prefix.tolist() == [0, 0, 0]
    tabs = host[sizes.table_off:].view(np.int32)
    assert tabs[d[1].tab_v:d[1].tab_v + 36].tolist() == [int(12.5 + 25 * y) for y in range(36)]


def test_plan_follows_pillows_pass_order():
    """PIL's Image.resize runs the vertical pass first when the source is more than 100 times as tall as wide and the height shrinks"""
    st, sizes, host = _plan(_descs([(900, 700), (900, 700), (201, 2), (200, 2), (30, 1)], [(100, 50, 800, 2), None, None, None, None]))
    assert st == 0
    d, prefix = _read(host, sizes, 5)
    assert [d[k].vfirst for k in range(5)] == [1, 0, 1, 0, 0]
    assert (d[0].mid_first, d[0].mid_count) == (0, 2) and int(prefix[1]) == 32 * 2 * 3       # crop rows x the box's columns


def test_refusals_need_no_device():
    from robustart_amd import _lib
    lib = _lib.load()
    err = lib.rart_last_error_string
    two = [(33, 47), (75, 100)]
    assert _plan(_descs(two), n=0)[0] == 1 and b'count' in err()
    assert _plan(_descs(two), f=6)[0] == 1 and b'filter' in err()
    assert _plan(_descs(two), f=-1)[0] == 1 and b'filter' in err()
    assert _plan(_descs(two, [(0, 0, 34, 47), None]))[0] == 1 and b'box' in err()
    assert _plan(_descs(two, [None, (-1, 0, 75, 100)]))[0] == 1 and b'box' in err()
    assert _plan(_descs(two, [None, (0, 0, 0, 100)]))[0] == 1 and b'box' in err()
    assert _plan(_descs(two), crop=(2, 5, 32, 32))[0] == 1 and b'crop window' in err()
    assert _plan(_descs(two), crop=(0, 0, 37, 36))[0] == 1 and b'crop window' in err()
    st, sizes, host = _plan(_descs(two), f=5)
    assert st == 0
    need, out_bytes = int(sizes.workspace_bytes), 2 * 32 * 32 * 3

    def call(h=host, ws_bytes=need, out=out_bytes):
        return lib.rart_resize_batch_u8(FAKE, h.ctypes.data, h.size, FAKE, ws_bytes, FAKE, out, None)

    def edited(offset, ctype, value):
        h = host.copy()
        ctype.from_buffer(h, offset).value = value
        return h

    P, D = _lib.ResizePlan, _lib.ResizeDesc
    assert call(edited(P.n.offset, ctypes.c_int32, 0)) == 1 and b'count' in err()
    assert call(edited(P.n.offset, ctypes.c_int32, 3)) == 1 and b'region offsets' in err()
    assert call(edited(P.filter.offset, ctypes.c_int32, 6)) == 1 and b'filter' in err()
    assert call(edited(P.crop_y.offset, ctypes.c_int32, 5)) == 1 and b'crop window' in err()
    assert call(edited(sizes.desc_off + D.box_w.offset, ctypes.c_int32, 48)) == 1 and b'box' in err()
    assert call(edited(sizes.desc_off + D.tab_h.offset, ctypes.c_int32, int(sizes.table_count) - 8)) == 1 and b'table offset' in err()
    assert call(edited(sizes.desc_off + D.ks_v.offset, ctypes.c_int32, 1 << 20)) == 1 and b'table offset' in err()
    assert call(edited(sizes.desc_off + D.mid_count.offset, ctypes.c_int32, 34)) == 1 and b'intermediate range' in err()
    d0 = _read(host, sizes, 2)[0][0]
    row = sizes.table_off + 4 * (d0.tab_h + 2 * (d0.ks_h + 2))            # the first row the crop window reads (crop_x = 2)
    assert call(edited(row + 4, ctypes.c_int32, d0.ks_h + 1)) == 1 and b'taps' in err()                 # a tap count past the row
    assert call(edited(row, ctypes.c_int32, 47)) == 1 and b'taps' in err()                              # taps that leave the box
    assert call(edited(sizes.prefix_off + 8, ctypes.c_int64, 7)) == 1 and b'prefix' in err()
    assert call(host[:host.size - 4]) == 1 and b'plan_bytes' in err()
    assert call(ws_bytes=need - 1) == 3 and b'workspace' in err()
    assert call(out=out_bytes - 1) == 1 and b'out of' in err()


def test_imagenet_s_ops_parsing():
    from robustart_amd.noise.imagenet_s import CV_MODES, PIL_FILTERS
    from robustart_amd.train import cls_solver as S
    eleven = list(PIL_FILTERS) + list(CV_MODES)
    assert S.imagenet_s_ops(None) == eleven and S.imagenet_s_ops('') == eleven and len(eleven) == 11
    assert eleven[0] == 'pil-nearest' and eleven[6] == 'opencv-nearest'
    assert S.imagenet_s_ops('pil-lanczos, opencv-area') == ['pil-lanczos', 'opencv-area']
    with pytest.raises(ValueError, match='unknown resize operator'):
        S.imagenet_s_ops('pil-bilinear,pil-sinc')
    with pytest.raises(ValueError, match='every operator once'):
        S.imagenet_s_ops('pil-box,pil-box')
    # an unknown name fails in main() before the config is read or a model built
    with pytest.raises(ValueError, match='unknown resize operator'):
        S.main(['--config', '/nonexistent.yaml', '--evaluate', '--imagenet-s', '--imagenet-s-ops', 'bicubic'])
    with pytest.raises(ValueError, match='--evaluate'):
        S.main(['--config', '/nonexistent.yaml', '--imagenet-s'])


def test_batch_transfer_refuses_what_the_single_form_refuses():
    from robustart_amd.noise import imagenet_s as NS
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            NS.image_transfer_batch([b''], decoded=[np.zeros((4, 4, 3), np.uint8)])
        return
    for dec in ('opencv', 'ffmpeg'):
        with pytest.raises(NotImplementedError, match='OpenCV / ffmpeg'):
            NS.image_transfer_batch([b''], decoder_type=dec, decoded=[np.zeros((4, 4, 3), np.uint8)])
    with pytest.raises(NotImplementedError):
        NS.image_transfer_batch([b''], resize_type='pil-sinc', decoded=[np.zeros((4, 4, 3), np.uint8)])


def _args(**kw):
    base = dict(attack=None, corruption=None, imagenet_s=True, imagenet_s_ops=None, engine='hip', precision=None, save_dir=None,
                src_name=None)
    base.update(kw)
    return argparse.Namespace(**base)


# exprs/exp/imagenet_s_loop/config_vit_base.yaml:79-101, restated
LOOP_TEST = {'save_acc_var_neg': True, 'root_dir': '/data/val/', 'meta_file': '/data/meta/val.txt', 'image_reader': {'type': 'pil'},
             'sampler': {'type': 'distributed'}, 'limit_samples': None,
             'transforms': [{'type': 'Resize', 'kwargs': {'size': [256, 256]}}, {'type': 'CenterCrop', 'kwargs': {'size': [224, 224]}},
                            {'type': 'ToTensor'},
                            {'type': 'Normalize', 'kwargs': {'mean': [0.485, 0.456, 0.406], 'std': [0.229, 0.224, 0.225]}}]}


def test_loop_refuses_other_noise_and_the_cpu():
    from robustart_amd.train import cls_solver as S
    cfg = {'model': {'type': 'resnet50_official'}, 'data': {'read_from': 'fs', 'input_size': 224, 'test': dict(LOOP_TEST)}}
    cpu = torch.device('cpu')
    for kw in (dict(attack='pgd_linf'), dict(corruption='fog'), dict(attack='fgsm', corruption='fog')):
        with pytest.raises(ValueError, match='cannot be combined'):
            S.evaluate_imagenet_s(cfg, _args(**kw), 0, 1, cpu)
    natural = {'model': cfg['model'], 'data': dict(cfg['data'], test=dict(LOOP_TEST, **{'imagenet_a&o': True}))}
    with pytest.raises(ValueError, match='cannot be combined'):
        S.evaluate_imagenet_s(natural, _args(), 0, 1, cpu)
    with pytest.raises(ValueError, match='unknown resize operator'):
        S.evaluate_imagenet_s(cfg, _args(imagenet_s_ops='nope'), 0, 1, cpu)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        S.evaluate_imagenet_s(cfg, _args(), 0, 1, cpu)
    with pytest.raises(RuntimeError, match='no CPU fallback'):             # evaluate() hands --imagenet-s to the loop
        S.evaluate(cfg, _args(attack='none'), 0, 1, cpu)


def test_loop_configs_list_form_test_transforms_parse():
    from robustart_amd.train import cls_solver as S
    dcfg = {'read_from': 'fs', 'input_size': 224, 'test_resize': 256, 'test': json.loads(json.dumps(LOOP_TEST))}
    assert S.read_transforms(dcfg, 'test') == {'type': 'ONECROP', 'test_resize': 256, 'jitter': None, 'flip': True}
    ds = S.make_dataset(dict(dcfg, test=dict(dcfg['test'], meta_file=None, root_dir=None) | {'root_dir': '/', 'meta_file': '/dev/null'}),
                        0, 224, 'test')
    assert isinstance(ds, S.FileImageNet) and (ds.transform, ds.size, ds.test_resize, ds.reader) == ('ONECROP', 224, 256, 'pil')
    assert callable(ds.transform) and len(ds) == 0                          # the name is also the transform step
