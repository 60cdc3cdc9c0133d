"""`data.test.imagenet_a&o` through cls_solver.main on the GPU: three image folders on disk -> PIL decode -> resize + crop on the GPU ->
HIP engine logits -> rart_logit_confidence_f32 over each set's class subset -> ConfidenceWriter files -> the evaluators.
Every line of the three result files is compared with the definition (tests/_confidence_ref.py, fp64) applied to engine logits that
the test recomputes through `logits_from_u8` on the same batches."""
import contextlib
import io
import json
import os

import numpy as np
import pytest
import torch

from _confidence_ref import conf_bound, reference, torch_fp32_error

pytestmark = pytest.mark.gpu

WNIDS = ['n%08d' % (7 * i + 3) for i in range(1000)]            # made-up, sorted: line number = class index
A_CLASSES = [WNIDS[i] for i in (0, 217, 480, 733, 999)]
O_CLASSES = [WNIDS[i] for i in (5, 301, 302, 870)]
BS = 4
SEED = 3


def _image(rs, h, w):
    """a smooth coloured pattern plus noise; colour, frequency and noise level differ from image to image, so that a random network
    does not answer every sample alike"""
    yy, xx = np.mgrid[0:h, 0:w]
    col, f, ph = rs.rand(3) * 255, 3.0 + 40 * rs.rand(), rs.rand() * 6
    base = np.stack([col[c] * (0.5 + 0.5 * np.sin(xx / f + ph + c) * np.cos(yy / (f * 1.7) + c * ph)) for c in range(3)], -1)
    return np.clip(base + rs.randn(h, w, 3) * rs.rand() * 40, 0, 255).astype(np.uint8)


def _folder(root, classes, per_class, rs):
    from PIL import Image
    k = 0
    for c in classes:
        os.makedirs(os.path.join(root, c))
        for j in range(per_class):
            h, w = 200 + 13 * (k % 5), 230 + 17 * (k % 4)
            Image.fromarray(_image(rs, h, w)).save(os.path.join(root, c, 'img_%d.png' % j))
            k += 1
    return root


@pytest.fixture(scope='module')
def setup(tmp_path_factory):
    from robustart_amd.model import get_model
    from robustart_amd.model.resnet_torch import randomize_bn_stats
    from robustart_amd.train import cls_solver as S
    root = tmp_path_factory.mktemp('natural')
    rs = np.random.RandomState(SEED)
    cif = str(root / 'classes.txt')
    with open(cif, 'w') as f:
        f.write('\n'.join(WNIDS) + '\n')
    torch.manual_seed(SEED)
    model = randomize_bn_stats(get_model({'type': 'resnet50_official'}), SEED).eval()
    # a random network's logits differ far more between classes than between images: centre them on a few probe images, so that the
    # prediction inside a subset depends on the image
    mean = torch.tensor(S.IMAGENET_MEAN).view(1, 3, 1, 1).cuda()
    std = torch.tensor(S.IMAGENET_STD).view(1, 3, 1, 1).cuda()
    probe = torch.from_numpy(np.stack([_image(rs, 224, 224) for _ in range(8)])).cuda().permute(0, 3, 1, 2).float() / 255.0
    model.cuda()
    with torch.no_grad():
        model.fc.bias -= model((probe - mean) / std).mean(0)
    model.cpu()
    ckpt = str(root / 'weights.pth')
    torch.save({'model': model.state_dict()}, ckpt)
    cfg = {'model': {'type': 'resnet50_official', 'kwargs': {'num_classes': 1000}},
           'data': {'type': 'imagenet', 'read_from': 'fs', 'batch_size': BS, 'input_size': 224, 'test_resize': 256,
                    'test': {'imagenet_a&o': True, 'class_index_file': cif, 'imagenet_val_root_dir': str(root / 'val'),
                             'imagenet_a_root_dir': _folder(str(root / 'a'), A_CLASSES, 3, rs),
                             'imagenet_o_root_dir': _folder(str(root / 'o'), O_CLASSES, 2, rs),
                             'imagenet_o_folder': _folder(str(root / 'o_in'), O_CLASSES, 3, rs),
                             'sampler': {'type': 'distributed'}, 'transforms': {'type': 'ONECROP'}}},
           'saver': {'pretrain': {'path': ckpt}}}
    path = str(root / 'cfg.yaml')
    with open(path, 'w') as f:
        json.dump(cfg, f)                    # JSON is YAML
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        res = S.main(['--config', path, '--evaluate', '--precision', 'fp32x', '--save-dir', str(root / 'hip')])
    return {'root': root, 'cfg': cfg, 'cfg_path': path, 'model': model, 'res': res, 'stdout': out.getvalue()}


def _read(save_dir, noise):
    with open(os.path.join(save_dir, 'resnet50_official', noise + '_0', 'results.txt.all')) as f:
        return [json.loads(ln) for ln in f]


SETS = (('imagenet_a', 'imagenet_a_root_dir', A_CLASSES, 15, True), ('imagenet_o_in', 'imagenet_o_folder', O_CLASSES, 12, True),
        ('imagenet_o_out', 'imagenet_o_root_dir', O_CLASSES, 8, False))


@pytest.fixture(scope='module')
def engine_logits(setup):
    """fp32x engine logits of the three sets, recomputed on the solver's batches: {noise name: (selected logits fp32 [n][K], labels)}"""
    from robustart_amd.model.engine import EngineModel
    from robustart_amd.train import cls_solver as S
    eng = EngineModel(setup['model'].cuda().eval(), takes_normalized=False, precision='fp32x').rart_engine
    out = {}
    for noise, key, classes, n, _ in SETS:
        ds = S.FileImageNet.from_folder(setup['cfg']['data']['test'][key], 224, 256, 'ONECROP')
        assert len(ds) == n and ds.classes == classes
        sub = [WNIDS.index(c) for c in classes]
        rows, labs = [], []
        for s in range(0, n, BS):                                 # the last batch is partial
            imgs, lab = ds.batch(list(range(s, min(s + BS, n))), 'cuda')
            rows.append(eng.logits_from_u8(imgs, S.IMAGENET_MEAN, S.IMAGENET_STD).float().cpu().numpy()[:, sub])
            labs += lab.tolist()
        out[noise] = (np.concatenate(rows), np.array(labs))
    return out


def test_result_files_follow_the_definition_on_engine_logits(setup, engine_logits):
    save = str(setup['root'] / 'hip')
    varied = set()
    for noise, _, classes, n, labelled in SETS:
        recs = _read(save, noise)
        assert len(recs) == n and [r['index'] for r in recs] == list(range(n))
        assert all(list(r) == ['confidence', 'correct', 'num_correct', 'prediction', 'label', 'index'] for r in recs)
        z, labels = engine_logits[noise]
        pred, conf = reference(z)
        assert [r['prediction'] for r in recs] == pred.tolist()
        want_correct = (pred == labels).astype(int).tolist() if labelled else [0] * n
        assert [r['correct'] for r in recs] == [[b] for b in want_correct] and [r['num_correct'] for r in recs] == want_correct
        assert [r['label'] for r in recs] == (labels.tolist() if labelled else [-1] * n)
        assert labels.tolist() == sorted(labels.tolist()) and set(labels.tolist()) == set(range(len(classes)))    # folder order
        got = np.array([r['confidence'][0] for r in recs])
        assert (got.astype(np.float32) == got).all()                       # fp32 values, written without loss
        err = float((np.abs(got - conf) / conf).max())
        bound = conf_bound(torch_fp32_error(z, conf))
        print('%-15s n %2d  conf rel err %.3e  bound %.3e' % (noise, n, err, bound))
        assert err <= bound
        varied |= set(pred.tolist())
    assert len(varied) > 1                                                 # the samples do not all predict alike


def test_printed_metrics_equal_the_evaluators_on_the_files(setup):
    from robustart_amd import metrics as M
    save = str(setup['root'] / 'hip')
    lines = [ln for ln in setup['stdout'].splitlines() if ln.startswith('{')]
    assert len(lines) == 1
    printed = json.loads(lines[0])
    res = setup['res']
    assert json.loads(json.dumps(res)) == printed
    assert set(printed) == {'imagenet_a', 'imagenet_o', 'world_size', 'seconds'} and printed['world_size'] == 1
    assert set(printed['imagenet_a']) == {'top1', 'RMS_calib_error', 'AURRA', 'count'}
    assert set(printed['imagenet_o']) == {'AUPR', 'AUROC', 'FPR95', 'count_in', 'count_out'}
    path = lambda noise: os.path.join(save, 'resnet50_official', noise + '_0', 'results.txt.all')      # noqa: E731
    a = M.ImageNetAEvaluator().eval(path('imagenet_a'))
    assert printed['imagenet_a'] == dict(a, count=15)
    assert a['RMS_calib_error'] is None           # 15 samples are fewer than one bin of 100
    recs = _read(save, 'imagenet_a')
    assert a['top1'] == 100 * np.mean([r['num_correct'] for r in recs])
    assert M.ImageNetAEvaluator(beta=5).eval(path('imagenet_a'))['RMS_calib_error'] >= 0.0
    ev = M.ImageNetOEvaluator()
    o = ev.eval(path('imagenet_o_in'), path('imagenet_o_out'))
    assert printed['imagenet_o'] == {'AUPR': o['AUPR'], 'AUROC': ev.last_measures['AUROC'], 'FPR95': ev.last_measures['FPR95'],
                                     'count_in': 12, 'count_out': 8}
    c_in = [r['confidence'][0] for r in _read(save, 'imagenet_o_in')]
    c_out = [r['confidence'][0] for r in _read(save, 'imagenet_o_out')]
    auroc, aupr, fpr = M.get_measures(-np.array(c_out), -np.array(c_in))
    assert (o['AUPR'], ev.last_measures['AUROC'], ev.last_measures['FPR95']) == (100 * aupr, 100 * auroc, 100 * fpr)


def test_torch_engine_feeds_the_same_kernel(setup, engine_logits):
    """--engine torch: the torch module's fp32 logits through the same kernel and writer.  prediction and correct equal the HIP
    engine's wherever the fp64 gap between the two largest subset logits exceeds 1e-3; at most 2 of the 35 samples may fall below."""
    from robustart_amd.train import cls_solver as S
    save_t = str(setup['root'] / 'torch')
    with contextlib.redirect_stdout(io.StringIO()):
        res = S.main(['--config', setup['cfg_path'], '--evaluate', '--engine', 'torch', '--save-dir', save_t])
    assert res['imagenet_a']['count'] == 15 and res['imagenet_o']['count_in'] == 12 and res['imagenet_o']['count_out'] == 8
    left_out = 0
    for noise, _, classes, n, _ in SETS:
        hip, tor = _read(str(setup['root'] / 'hip'), noise), _read(save_t, noise)
        assert len(tor) == n and [r['index'] for r in tor] == list(range(n))
        z = np.sort(engine_logits[noise][0].astype(np.float64), axis=1)
        clear = (z[:, -1] - z[:, -2]) > 1e-3
        left_out += int((~clear).sum())
        for i in np.where(clear)[0]:
            assert (tor[i]['prediction'], tor[i]['correct'], tor[i]['label']) == (hip[i]['prediction'], hip[i]['correct'], hip[i]['label'])
            assert abs(tor[i]['confidence'][0] - hip[i]['confidence'][0]) < 0.05
    assert left_out <= 2
