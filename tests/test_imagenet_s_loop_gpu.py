"""`cls_solver --evaluate --imagenet-s` on the GPU: ten files of different sizes -> one decode per batch -> eleven resize operators
(six through the batched Pillow-exact kernel, five through the per-image OpenCV restatement) -> HIP engine logits -> one result file
per operator -> ImageNetSEvaluator.  The uint8 batches the loop fed are compared with Pillow alone, the result files with the engine's
logits on those batches."""
import contextlib
import io
import itertools
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

import _jpeg_decode_ref as J
import _resize_batch_ref as R

pytestmark = pytest.mark.gpu

BS = 4
SEED = 5
# 8 baseline JPEGs and 2 PNGs, every size different, every side above 256: where an axis is upscaled NEAREST and BOX agree, and the
# operators could not be told apart
FILES = [('444', 300, 340), ('422', 420, 298), ('420', 375, 500), ('gray', 290, 410), ('420_rst', 333, 290), ('png', 310, 305),
         ('420_q95', 450, 320), ('420_opt_q30', 296, 385), ('png', 400, 300), ('422', 350, 351)]
PIL_OPS = ['pil-nearest', 'pil-bilinear', 'pil-cubic', 'pil-box', 'pil-hamming', 'pil-lanczos']
CV_OPS = ['opencv-nearest', 'opencv-bilinear', 'opencv-cubic', 'opencv-area', 'opencv-lanczos']
OPS = PIL_OPS + CV_OPS


def _run(S, NS, argv):
    """S.main(argv) with spies on the decode step and on image_transfer_batch -> (result, stdout, spy record)"""
    rec = {'decode_indices': 0, 'decode': 0, 'fed': [], 'datasets': []}
    real_di, real_d, real_itb = S.FileImageNet.decode_indices, S.FileImageNet.decode, NS.image_transfer_batch

    def decode_indices(self, indices, dev):
        rec['decode_indices'] += 1
        if not any(self is d for d in rec['datasets']):
            rec['datasets'].append(self)
        return real_di(self, indices, dev)

    def decode(self, i):
        rec['decode'] += 1
        return real_d(self, i)

    def itb(items, decoder_type='pil', resize_type='pil-bilinear', *a, **k):
        out = real_itb(items, decoder_type, resize_type, *a, **k)
        rec['fed'].append((resize_type, out.cpu()))
        return out

    S.FileImageNet.decode_indices, S.FileImageNet.decode, NS.image_transfer_batch = decode_indices, decode, itb
    try:
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            res = S.main(argv)
    finally:
        S.FileImageNet.decode_indices, S.FileImageNet.decode, NS.image_transfer_batch = real_di, real_d, real_itb
    return res, buf.getvalue(), rec


@pytest.fixture(scope='module')
def setup(tmp_path_factory):
    from robustart_amd.model import get_model
    from robustart_amd.model.resnet_torch import randomize_bn_stats
    from robustart_amd.noise import imagenet_s as NS
    from robustart_amd.train import cls_solver as S
    root = tmp_path_factory.mktemp('imagenet_s')
    os.makedirs(str(root / 'val'))
    names, arrays = [], []
    for k, (kind, h, w) in enumerate(FILES):
        arr = J.source_array(h, w, 'noise', seed=SEED + k)       # on smooth content cubic and lanczos agree too often
        name = 'img%02d.%s' % (k, 'png' if kind == 'png' else 'jpg')
        if kind == 'png':
            Image.fromarray(arr).save(str(root / 'val' / name), 'PNG')
        else:
            (root / 'val' / name).write_bytes(J.encode(arr, kind))
        names.append(name)
        with Image.open(str(root / 'val' / name)) as im:
            arrays.append(np.array(im.convert('RGB')))                    # what Pillow decodes: the loop's input by definition
    labels = [(37 * k + 11) % 1000 for k in range(len(FILES))]
    meta = str(root / 'meta.txt')
    with open(meta, 'w') as f:
        f.write(''.join(json.dumps({'filename': n, 'label': lab}) + '\n' for n, lab in zip(names, labels)))
    torch.manual_seed(SEED)
    model = randomize_bn_stats(get_model({'type': 'resnet50_official'}), SEED).eval()
    mean = torch.tensor(S.IMAGENET_MEAN).view(1, 3, 1, 1).cuda()
    std = torch.tensor(S.IMAGENET_STD).view(1, 3, 1, 1).cuda()
    probe = torch.from_numpy(np.stack([R.pillow(a, (224, 224), 1) for a in arrays[:8]])).cuda().permute(0, 3, 1, 2).float() / 255.0
    model.cuda()
    with torch.no_grad():
        model.fc.bias -= model((probe - mean) / std).mean(0)             # centred, so that the prediction depends on the image
    model.cpu()
    ckpt = str(root / 'weights.pth')
    torch.save({'model': model.state_dict()}, ckpt)
    runs = {}
    for reader in ('pil', 'hip'):
        cfg = {'model': {'type': 'resnet50_official', 'kwargs': {'num_classes': 1000}},
               'data': {'type': 'imagenet', 'read_from': 'fs', 'batch_size': BS, 'input_size': 224, 'test_resize': 256, 'num_workers': 4,
                        'test': {'save_acc_var_neg': True, 'root_dir': str(root / 'val'), 'meta_file': meta,
                                 'image_reader': {'type': reader}, 'sampler': {'type': 'distributed'},
                                 'transforms': [{'type': 'Resize', 'kwargs': {'size': [256, 256]}},
                                                {'type': 'CenterCrop', 'kwargs': {'size': [224, 224]}}, {'type': 'ToTensor'},
                                                {'type': 'Normalize', 'kwargs': {'mean': [0.485, 0.456, 0.406],
                                                                                 'std': [0.229, 0.224, 0.225]}}]}},
               'saver': {'pretrain': {'path': ckpt}}}
        path = str(root / ('cfg_%s.yaml' % reader))
        with open(path, 'w') as f:
            json.dump(cfg, f)                # JSON is YAML
        save = str(root / reader)
        res, out, rec = _run(S, NS, ['--config', path, '--evaluate', '--imagenet-s', '--precision', 'fp32x', '--save-dir', save])
        runs[reader] = {'res': res, 'stdout': out, 'rec': rec, 'save': save}
    return {'root': root, 'model': model, 'arrays': arrays, 'labels': labels, 'names': names, 'runs': runs}


def _file(save, op):
    return os.path.join(save, 'resnet50_official', 'imagenet_s_pil_%s' % op, 'results.txt.all')


def _read(save, op):
    with open(_file(save, op)) as f:
        return [json.loads(ln) for ln in f]


def _fed(run, op):
    """the uint8 batches the loop fed for `op`, in batch order, as one (10, 224, 224, 3) array"""
    return np.concatenate([b.numpy() for name, b in run['rec']['fed'] if name == op])


@pytest.mark.parametrize('reader', ['pil', 'hip'])
def test_eleven_result_files_in_index_order(setup, reader):
    run = setup['runs'][reader]
    dirs = sorted(os.listdir(os.path.join(run['save'], 'resnet50_official')))
    assert dirs == sorted(['imagenet_s_pil_%s' % op for op in OPS] + ['imagenet_s_summary.json'])
    for op in OPS:
        recs = _read(run['save'], op)
        assert len(recs) == 10 and [r['index'] for r in recs] == list(range(10))
        assert [r['label'] for r in recs] == setup['labels'] and all(len(r['score']) == 1000 for r in recs)
    assert [name for name, _ in run['rec']['fed']] == OPS * 3               # three batches (4, 4, 2), every operator on each, in order


def test_pillow_alone_tells_the_operators_apart(setup):
    """a loop that applied one operator eleven times must fail: by Pillow alone, any two of the six PIL operators give inputs that
    differ in at least 20 % of the bytes on every file of the folder -- asserted before the kernel's batches are compared"""
    want = {op: np.stack([R.pillow(a, (256, 256), f, crop=(16, 16, 224, 224)) for a in setup['arrays']]) for f, op in enumerate(PIL_OPS)}
    worst = min((float((want[a][k] != want[b][k]).mean()), a, b, k) for a, b in itertools.combinations(PIL_OPS, 2) for k in range(10))
    print('smallest pairwise difference: %.1f %% of the bytes (%s vs %s, file %d)' % (100 * worst[0], worst[1], worst[2], worst[3]))
    assert worst[0] >= 0.20
    for reader in ('pil', 'hip'):
        for op in PIL_OPS:
            assert np.array_equal(_fed(setup['runs'][reader], op), want[op]), (reader, op)


@pytest.mark.parametrize('reader', ['pil', 'hip'])
def test_fed_batches_and_scores(setup, reader):
    """OpenCV operators: the existing per-image cv_resize; every operator: image_transfer_batch on the files of the same batches; the
    score rows: the engine's logits on the fed batches, exactly"""
    from robustart_amd.model.engine import EngineModel
    from robustart_amd.noise import imagenet_s as NS
    from robustart_amd.train import cls_solver as S
    run = setup['runs'][reader]
    dev = [torch.from_numpy(a).cuda() for a in setup['arrays']]
    for op in CV_OPS:
        want = torch.stack([NS.cv_resize(d[None], (256, 256), NS.CV_MODES[op], crop=(16, 16, 224, 224))[0] for d in dev]).cpu().numpy()
        assert np.array_equal(_fed(run, op), want), op
    paths = [os.path.join(str(setup['root'] / 'val'), n) for n in setup['names']]
    eng = EngineModel(setup['model'].cuda().eval(), takes_normalized=False, precision='fp32x').rart_engine
    varied = set()
    for op in OPS:
        fed = _fed(run, op)
        again = torch.cat([NS.image_transfer_batch(paths[s:s + BS], 'pil', op, 'val', 224) for s in range(0, 10, BS)])
        assert again.is_cuda and again.dtype == torch.uint8 and np.array_equal(again.cpu().numpy(), fed), op
        logits = torch.cat([eng.logits_from_u8(torch.from_numpy(fed[s:s + BS]).cuda(), S.IMAGENET_MEAN, S.IMAGENET_STD).float().cpu()
                            for s in range(0, 10, BS)]).numpy()
        recs = _read(run['save'], op)
        assert np.array_equal(np.array([r['score'] for r in recs], dtype=np.float32), logits), op
        assert [r['prediction'] for r in recs] == logits.argmax(1).tolist()
        varied |= set(r['prediction'] for r in recs)
    assert len(varied) > 1


@pytest.mark.parametrize('reader', ['pil', 'hip'])
def test_printed_metrics_equal_the_evaluator_on_the_files(setup, reader):
    from robustart_amd import metrics as M
    run = setup['runs'][reader]
    lines = [ln for ln in run['stdout'].splitlines() if ln.startswith('{')]
    assert len(lines) == 1
    printed = json.loads(lines[0])
    assert json.loads(json.dumps(run['res'])) == printed
    assert set(printed) == {'imagenet_s', 'Mean', 'Std.', 'count', 'world_size', 'seconds'}
    assert printed['count'] == 10 and printed['world_size'] == 1
    ev = M.ImageNetSEvaluator()
    want = {}
    for op in OPS:
        want['pil/%s' % op] = ev.eval(_file(run['save'], op), 'pil', op)[('pil', op)]
    assert printed['imagenet_s'] == want and list(printed['imagenet_s']) == ['pil/%s' % op for op in OPS]
    assert printed['Mean'] == ev.get_mean()['Mean'] and printed['Std.'] == ev.get_std()['Std.']
    with open(os.path.join(run['save'], 'resnet50_official', 'imagenet_s_summary.json')) as f:
        summary = json.load(f)
    assert summary['acc'] == want and summary['mean'] == printed['Mean'] and summary['neg_std'] == -printed['Std.']
    assert summary['var'] == pytest.approx(printed['Std.'] ** 2, rel=1e-12, abs=1e-12)


def test_every_file_is_decoded_once_per_batch(setup):
    pil, hip = setup['runs']['pil']['rec'], setup['runs']['hip']['rec']
    assert pil['decode_indices'] == 3 and pil['decode'] == 10               # not 11 times as many
    assert hip['decode_indices'] == 3 and len(hip['datasets']) == 1
    assert hip['datasets'][0].decode_stats == {'gpu': 8, 'fallback': 2}    # 8 baseline JPEGs on the GPU, the 2 PNGs through Pillow
    assert hip['decode'] == 0


def test_the_two_readers_give_identical_files(setup):
    for op in OPS:
        with open(_file(setup['runs']['pil']['save'], op), 'rb') as a, open(_file(setup['runs']['hip']['save'], op), 'rb') as b:
            assert a.read() == b.read(), op
