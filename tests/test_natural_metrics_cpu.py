"""ImageNet-A / -O / -P metrics on the CPU: calibration.py against numbers produced by running the reference's calibration_tools.py
and imagenetp_evaluator.py (tests/golden/make_natural_golden.py) and against sklearn itself, the evaluators and their result files,
the host side of the subset confidence (index validation, the entry's argument checks) and the solver's config errors."""
import ctypes
import json
import os

import numpy as np
import pytest

from robustart_amd import metrics as M
from robustart_amd.metrics import calibration as CAL

HERE = os.path.dirname(os.path.abspath(__file__))
REL = 1e-12


@pytest.fixture(scope='module')
def gold():
    with open(os.path.join(HERE, 'golden', 'natural_ref.json')) as f:
        return json.load(f)


def _close(got, want):
    return abs(got - want) <= REL * abs(want)


def test_calib_err_and_aurra_equal_the_reference(gold):
    assert [c['n'] for c in gold['calib']] == [750, 800, 150]
    for c in gold['calib']:
        conf, corr = np.array(c['confidence']), np.array(c['correct'])
        assert (conf[::7] == 1.0).all() and (conf.astype(np.float32) == conf).all()       # fp32 values, ties at exactly 1.0
        for p, want in c['calib_err'].items():
            got = CAL.calib_err(conf, corr, p=p, beta=c['beta'])
            assert _close(got, want), (c['n'], p, got, want)
        assert _close(CAL.aurra(conf, corr), c['aurra'])
    one_bin = gold['calib'][2]
    assert CAL.calib_err(np.array(one_bin['confidence']), np.array(one_bin['correct'])) == 0.0     # the only bin is the last: left out


def test_calib_err_leaves_out_its_last_bin(gold):
    """the mirrored defect, stated on its own: changing the samples of the last bin does not change the error"""
    c = gold['calib'][0]
    conf, corr = np.array(c['confidence']), np.array(c['correct'])
    order = np.argsort(conf)
    last = order[600:]                       # 750 samples, beta 100: bins [0,100) ... [500,600), [600,750)
    flipped = corr.copy()
    flipped[last] = 1.0 - flipped[last]
    assert CAL.calib_err(conf, flipped, p='2') == CAL.calib_err(conf, corr, p='2')
    first = order[:100]
    flipped = corr.copy()
    flipped[first] = 1.0 - flipped[first]
    assert CAL.calib_err(conf, flipped, p='2') != CAL.calib_err(conf, corr, p='2')


def test_fewer_samples_than_beta_is_a_value_error():
    with pytest.raises(ValueError, match=r'99 .*100'):
        CAL.calib_err(np.linspace(0, 1, 99), np.ones(99), beta=100)
    with pytest.raises(ValueError):
        CAL.calib_err(np.ones(100), np.ones(100), p='3')
    assert CAL.calib_err(np.linspace(0, 1, 100), np.ones(100), beta=100) == 0.0


def test_get_measures_equals_the_reference(gold):
    assert [m['name'] for m in gold['measures']] == ['ties', 'separable']
    for m in gold['measures']:
        auroc, aupr, fpr = CAL.get_measures(m['pos'], m['neg'], m['recall_level'])
        assert _close(auroc, m['auroc']) and _close(aupr, m['aupr']) and _close(fpr, m['fpr']), (m['name'], auroc, aupr, fpr)
    ties = gold['measures'][0]
    assert len(set(ties['pos']) | set(ties['neg'])) < 250          # 950 scores on far fewer distinct values
    assert CAL.get_measures(gold['measures'][1]['pos'], gold['measures'][1]['neg']) == (1.0, 1.0, 0.0)


def test_get_measures_equals_sklearn(gold):
    sk = pytest.importorskip('sklearn.metrics')
    cases = [(np.array(m['pos']), np.array(m['neg'])) for m in gold['measures']]
    for c in gold['calib']:                  # confidences with a run of ties at exactly 1.0, as ImageNetOEvaluator scores them
        conf = np.array(c['confidence'])
        cases.append((-conf[:len(conf) // 3], -conf[len(conf) // 3:]))
    for pos, neg in cases:
        y = np.r_[np.ones(len(pos), np.int32), np.zeros(len(neg), np.int32)]
        s = np.r_[pos, neg]
        auroc, aupr, _ = CAL.get_measures(pos, neg)
        assert _close(auroc, sk.roc_auc_score(y, s)) and _close(aupr, sk.average_precision_score(y, s))


def test_imagenet_p_flip_rate_equals_the_reference(gold, tmp_path):
    g = gold['imagenet_p']
    assert len(g['predictions']) == 5 and all(len(s) == 31 for s in g['predictions'])
    path = str(tmp_path / 'results.txt.all')
    with open(path, 'w') as f:
        for seq in g['predictions']:
            f.write(json.dumps({'predictions': seq}) + '\n')
    ev = M.ImageNetPEvaluator()
    for pert, want in g['flip_rate'].items():
        assert _close(ev.eval(path, pert)[pert], want)
    assert g['flip_rate']['gaussian_noise'] != g['flip_rate']['brightness']        # first-frame vs previous-frame comparison
    assert _close(ev.get_mean()['Mean'], np.mean(list(g['flip_rate'].values())))


def _write_conf(path, conf, correct):
    with open(path, 'w') as f:
        for i, (c, b) in enumerate(zip(conf, correct)):
            f.write(json.dumps({'confidence': [float(c)], 'correct': [int(b)], 'num_correct': int(b), 'prediction': 0, 'label': 0,
                                'index': i}) + '\n')


def test_the_three_get_mean_methods_run_over_the_values(gold, tmp_path):
    c = gold['calib'][0]
    conf, corr = np.array(c['confidence']), np.array(c['correct'])
    p_in, p_out = str(tmp_path / 'in.all'), str(tmp_path / 'out.all')
    _write_conf(p_in, conf[:500], corr[:500])
    _write_conf(p_out, conf[500:], corr[500:])
    a = M.ImageNetAEvaluator()
    ra = a.eval(p_in)
    assert set(ra) == {'top1', 'RMS_calib_error', 'AURRA'}
    assert ra['top1'] == 100 * corr[:500].mean()
    assert ra['RMS_calib_error'] == 100 * CAL.calib_err(conf[:500], corr[:500], p='2') and ra['AURRA'] == 100 * CAL.aurra(conf[:500], corr[:500])
    assert _close(a.get_mean()['Mean'], np.mean(list(ra.values())))
    o = M.ImageNetOEvaluator()
    ro = o.eval(p_in, p_out)
    assert set(ro) == {'AUPR'} and o.get_mean() == {'Mean': ro['AUPR']} and o.metric.cmp_key == 'Mean'
    assert set(o.last_measures) == {'AUROC', 'AUPR', 'FPR95'}
    p = M.ImageNetPEvaluator()
    p.metric.update({'gaussian_noise': 0.5, 'brightness': 0.25})
    assert p.get_mean() == {'Mean': 0.375}
    for ev in (a, o, p):
        ev.clear()
        assert ev.metric.metric == {}


def test_confidence_writer_merges_shards_by_index_and_feeds_the_evaluator(gold, tmp_path):
    import torch
    c = gold['calib'][1]
    conf = torch.tensor(c['confidence'][:40], dtype=torch.float32)
    corr = torch.tensor(c['correct'][:40], dtype=torch.uint8)
    pred = torch.arange(40, dtype=torch.int32) % 7
    lab = torch.where(corr.bool(), pred.long(), pred.long() + 1)
    idx = list(range(40))

    def run(d, world, bs):
        per = (40 + world - 1) // world
        writers = [M.ConfidenceWriter(d, r, world) for r in range(world)]
        for r, w in enumerate(writers):
            mine = idx[r * per:(r + 1) * per]
            for s in range(0, len(mine), bs):
                it = mine[s:s + bs]
                w.write_batch(pred[it], conf[it], corr[it], lab[it], it)
        for w in reversed(writers):          # rank 0 merges last, once every shard is closed
            out = w.close()
        return out
    one = run(str(tmp_path / 'w1'), 1, 40)
    two = run(str(tmp_path / 'w2'), 2, 7)
    assert open(one, 'rb').read() == open(two, 'rb').read()
    recs = [json.loads(ln) for ln in open(two)]
    assert [r['index'] for r in recs] == idx
    assert list(recs[3]) == ['confidence', 'correct', 'num_correct', 'prediction', 'label', 'index']
    assert [r['confidence'] for r in recs] == [[float(v)] for v in conf] and [r['correct'] for r in recs] == [[int(v)] for v in corr]
    assert [r['num_correct'] for r in recs] == corr.tolist() and [r['prediction'] for r in recs] == pred.tolist()
    # a set without labels, as the out-of-distribution pass writes it
    w = M.ConfidenceWriter(str(tmp_path / 'w3'))
    w.write_batch(pred[20:], conf[20:], torch.zeros(20, dtype=torch.uint8), None, idx[20:])
    out = w.close()
    assert all(json.loads(ln)['label'] == -1 and json.loads(ln)['correct'] == [0] for ln in open(out))
    # fed to ImageNetOEvaluator: the measures of the same arrays
    w = M.ConfidenceWriter(str(tmp_path / 'w4'))
    w.write_batch(pred[:20], conf[:20], corr[:20], lab[:20], idx[:20])
    p_in = w.close()
    ev = M.ImageNetOEvaluator()
    res = ev.eval(p_in, out)
    auroc, aupr, fpr = CAL.get_measures(-conf[20:].double().numpy(), -conf[:20].double().numpy())
    assert res == {'AUPR': 100 * aupr} and ev.last_measures == {'AUROC': 100 * auroc, 'AUPR': 100 * aupr, 'FPR95': 100 * fpr}


def test_class_subset_validates_on_the_host():
    import torch
    t = M.class_subset([0, 3, 999], 1000, 'cpu')
    assert t.dtype == torch.int32 and t.tolist() == [0, 3, 999]
    for bad in ([3, 1], [1, 1], [-1, 2], [0, 1000], [0, 1.5], [True, 2]):
        with pytest.raises(ValueError):
            M.class_subset(bad, 1000, 'cpu')
    with pytest.raises(RuntimeError, match='CUDA'):          # no CPU path
        M.subset_confidence(torch.zeros(2, 10), None, None)


def test_logit_confidence_argument_checks_without_gpu():
    """Validation happens before any HIP call, so these are safe without a GPU."""
    from robustart_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(16)           # never dereferenced: the checks run first
    f = lib.rart_logit_confidence_f32
    assert f(None, 0, 1000, 1000, None, 0, None, None, None, None, None) == 0          # no rows: nothing launched
    bad = [(one, -1, 1000, 1000, None, 0, None, one, one, one),          # rows < 0
           (one, 4, 0, 1000, None, 0, None, one, one, one),              # classes < 1
           (one, 4, 1000, 999, None, 0, None, one, one, one),            # ld < classes
           (one, 4, 1000, 1000, one, -1, None, one, one, one),           # n_subset < 0
           (one, 4, 1000, 1000, one, 1001, None, one, one, one),         # n_subset > classes
           (None, 4, 1000, 1000, None, 0, None, one, one, one),          # NULL logits
           (one, 4, 1000, 1000, None, 0, None, None, one, one),          # NULL pred
           (one, 4, 1000, 1000, None, 0, None, one, None, one),          # NULL conf
           (one, 4, 1000, 1000, None, 0, None, one, one, None)]          # NULL correct
    for args in bad:
        assert f(*args, None) == 1, args
        assert b'rart_logit_confidence_f32' in lib.rart_last_error_string()


# ---- the solver's config errors: all raised on the host, before a model is built or a device is touched ----------------------------

def _tree(root, classes, files=1):
    for c in classes:
        os.makedirs(os.path.join(root, c))
        for k in range(files):
            with open(os.path.join(root, c, 'img_%d.png' % k), 'wb') as f:
                f.write(b'x')
    return root


def _natural_cfg(tmp_path, n_map=1000, a=('n00000003', 'n00000010'), o=('n00000005', 'n00000020'), o_in=None):
    os.makedirs(str(tmp_path))
    wnids = ['n%08d' % i for i in range(n_map)]
    cif = str(tmp_path / 'classes.txt')
    with open(cif, 'w') as f:
        f.write('\n'.join(wnids) + '\n')
    cfg = {'model': {'type': 'resnet50_official', 'kwargs': {'num_classes': 1000}},
           'data': {'type': 'imagenet', 'read_from': 'fs', 'batch_size': 4, 'input_size': 224, 'test_resize': 256,
                    'test': {'imagenet_a&o': True, 'class_index_file': cif, 'imagenet_val_root_dir': str(tmp_path / 'val'),
                             'imagenet_a_root_dir': _tree(str(tmp_path / 'a'), a),
                             'imagenet_o_root_dir': _tree(str(tmp_path / 'o'), o),
                             'imagenet_o_folder': _tree(str(tmp_path / 'o_in'), o if o_in is None else o_in),
                             'sampler': {'type': 'distributed'}, 'transforms': {'type': 'ONECROP'}}}}
    path = str(tmp_path / 'cfg.yaml')
    with open(path, 'w') as f:
        json.dump(cfg, f)                    # JSON is YAML
    return path, cfg


def test_solver_config_errors_of_the_natural_mode(tmp_path):
    from robustart_amd.train import cls_solver as S
    save = str(tmp_path / 'res')
    path, cfg = _natural_cfg(tmp_path / 'ok')
    with pytest.raises(ValueError, match='--save-dir'):
        S.main(['--config', path, '--evaluate'])
    with pytest.raises(ValueError, match='--attack'):
        S.main(['--config', path, '--evaluate', '--save-dir', save, '--attack', 'pgd_linf'])
    with pytest.raises(ValueError, match='--attack / --corruption'):
        S.main(['--config', path, '--evaluate', '--save-dir', save, '--corruption', 'gaussian_noise'])
    # the valid config resolves on the host: folder sets in sorted order, subsets = the ranks of the folders' classes
    plan = S.natural_datasets(cfg)
    assert plan['a'][1] == [3, 10] and plan['o_in'][1] == plan['o_out'][1] == [5, 20]
    assert plan['a'][0].classes == ['n00000003', 'n00000010'] and plan['a'][0].items == [('n00000003/img_0.png', 0), ('n00000010/img_0.png', 1)]
    path, _ = _natural_cfg(tmp_path / 'count', n_map=999)
    with pytest.raises(ValueError, match='999 classes.*1000'):
        S.main(['--config', path, '--evaluate', '--save-dir', save])
    path, _ = _natural_cfg(tmp_path / 'unknown', a=('n00000003', 'n99999999'))
    with pytest.raises(ValueError, match='n99999999'):
        S.main(['--config', path, '--evaluate', '--save-dir', save])
    path, _ = _natural_cfg(tmp_path / 'o_in', o_in=('n00000005', 'n00000021'))
    with pytest.raises(ValueError, match='imagenet_o_folder'):
        S.main(['--config', path, '--evaluate', '--save-dir', save])
    # without class_index_file the map is the sorted folder names of imagenet_val_root_dir, and its count is checked the same way
    path, cfg = _natural_cfg(tmp_path / 'val')
    del cfg['data']['test']['class_index_file']
    _tree(cfg['data']['test']['imagenet_val_root_dir'], ['n%08d' % i for i in range(30)], files=0)
    with pytest.raises(ValueError, match='imagenet_val_root_dir.* 30 classes'):
        S.natural_datasets(cfg)
    cfg['model']['kwargs']['num_classes'] = 30
    assert S.natural_datasets(cfg)['a'][1] == [3, 10]
    assert not os.path.exists(save)          # every error came before anything was written


def test_a_config_without_the_key_evaluates_as_before():
    from robustart_amd.train import cls_solver as S
    assert not S.natural_mode({'test': {'root_dir': 'x', 'meta_file': 'y'}}) and not S.natural_mode({}) and not S.natural_mode({'test': None})
    with pytest.raises(ValueError, match='needs data.test.root_dir and data.test.meta_file'):
        S.make_dataset({'read_from': 'fs', 'test': {}}, 0, 224, 'test')


def test_imagenet_a_evaluator_on_a_file_smaller_than_one_bin(gold, tmp_path):
    """fewer samples than beta: no bin, no calibration error -- None, with accuracy and AURRA still reported"""
    c = gold['calib'][0]
    conf, corr = np.array(c['confidence'][:15]), np.array(c['correct'][:15])
    path = str(tmp_path / 'small.all')
    _write_conf(path, conf, corr)
    ev = M.ImageNetAEvaluator()
    res = ev.eval(path)
    assert res == {'top1': 100 * corr.mean(), 'RMS_calib_error': None, 'AURRA': 100 * CAL.aurra(conf, corr)}
    assert _close(ev.get_mean()['Mean'], (res['top1'] + res['AURRA']) / 2)
    assert M.ImageNetAEvaluator(beta=5).eval(path)['RMS_calib_error'] == 100 * CAL.calib_err(conf, corr, p='2', beta=5)
