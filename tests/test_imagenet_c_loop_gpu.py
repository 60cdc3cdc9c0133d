"""`cls_solver --evaluate --imagenet-c` on the GPU against the path that existed before it: one `--corruption NAME --severity S`
evaluation per pair.  Fake data at 224, 8 images in batches of 4.  A tiny registered model on the torch engine covers the 14
corruptions that need no photographs at all five severities; ViT-B/16 with one block covers the HIP engine, the fused noise launch
at two severities and frost with photographs from a folder."""
import contextlib
import io
import json
import os

import numpy as np
import pytest
import torch

import _topk_score_ref as T
from _tiny_eval_model import tiny_eval_model

pytestmark = pytest.mark.gpu

N, BS, SEED = 8, 4, 0


class _Args:
    engine = 'torch'
    corruption = None
    attack = None
    eps = '2/255'
    steps = 0
    severity = 3
    seed = SEED
    precision = None
    save_dir = None
    src_name = None
    tgt_name = None
    tgt_type = None
    imagenet_c = False
    imagenet_c_names = None
    imagenet_c_severities = None
    imagenet_c_frost_dir = None
    imagenet_c_scores = False


def _args(**kw):
    a = _Args()
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _cfg(model):
    return {'model': model, 'data': {'fake_size': N, 'batch_size': BS, 'input_size': 224, 'read_from': 'fake'}}


def _quiet(fn, *a, **k):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        res = fn(*a, **k)
    return res, buf.getvalue()


def _file(save, name, c, s):
    return os.path.join(save, name, '%s_%d' % (c, s), 'results.txt.all')


def _read(path):
    with open(path) as f:
        return [json.loads(ln) for ln in f]


def _single_runs(S, cfg, model, pairs, save, **kw):
    """the parent's way: evaluate() once per pair through the existing --corruption path -> {pair: (top-1 count, top-5 count)}"""
    rank, world, device = S.init_dist()
    out = {}
    for c, s in pairs:
        res, _ = _quiet(S.evaluate, cfg, _args(corruption=c, severity=s, save_dir=save, src_name='m', **kw), rank, world, device, model=model)
        assert res['count'] == N
        out[(c, s)] = (round(res['top1'] * N), round(res['top5'] * N))
    return out


def _loop(S, cfg, model, **kw):
    rank, world, device = S.init_dist()
    return _quiet(S.evaluate, cfg, _args(imagenet_c=True, src_name='m', **kw), rank, world, device, model=model)


def _counts(res, pairs):
    return {p: (round(res['imagenet_c']['%s/%d' % p]['top1'] * N / 100), round(res['imagenet_c']['%s/%d' % p]['top5'] * N / 100))
            for p in pairs}


@pytest.fixture(scope='module')
def tiny(tmp_path_factory):
    from robustart_amd.noise import imagenet_c as C
    from robustart_amd.train import cls_solver as S
    C.set_frost_textures([])                              # whatever an earlier test registered: this fixture runs without photographs
    root = tmp_path_factory.mktemp('imagenet_c_tiny')
    model = tiny_eval_model(N)
    cfg = _cfg({'type': 'tiny_imagenet_c_test'})
    names = [n for n in C.CORRUPTION_NAMES[:15] if n != 'frost']
    pairs = [(c, s) for c in names for s in (1, 2, 3, 4, 5)]
    single = _single_runs(S, cfg, model, pairs, str(root / 'single'))
    # spies: the batches the loop read (they must come back unchanged) and the fused noise launches
    seen, fused = [], []
    real_batch, real_ns = S.FakeImageNet.batch, C.noise_severities_

    def batch(self, indices, device):
        imgs, lab = real_batch(self, indices, device)
        seen.append((imgs, imgs.clone()))
        return imgs, lab

    def noise_severities_(b, outs, severities=(1, 2, 3, 4, 5), *a, **k):
        fused.append((k.get('corruption_id'), tuple(severities)))
        return real_ns(b, outs, severities, *a, **k)

    S.FakeImageNet.batch, C.noise_severities_ = batch, noise_severities_
    try:
        plain, plain_out = _loop(S, cfg, model)
    finally:
        S.FakeImageNet.batch, C.noise_severities_ = real_batch, real_ns
    torch.cuda.synchronize()
    unchanged = [bool(torch.equal(a, b)) for a, b in seen]
    scores, _ = _loop(S, cfg, model, save_dir=str(root / 'scores'), imagenet_c_scores=True)
    ranks, _ = _loop(S, cfg, model, save_dir=str(root / 'ranks'))
    return {'root': root, 'pairs': pairs, 'names': names, 'single': single, 'plain': plain, 'plain_out': plain_out, 'scores': scores,
            'ranks': ranks, 'unchanged': unchanged, 'fused': fused}


def test_the_scores_have_no_tie_at_the_boundaries_of_k(tiny):
    """evaluate() counts with torch.topk, whose order among equal scores on the device is not documented: the comparison of counts
    below means something only if no score equals the label's at the k = 1 and k = 5 boundaries"""
    spread = set()
    for c, s in tiny['pairs']:
        for rec in _read(_file(str(tiny['root'] / 'single'), 'm', c, s)):
            z = np.sort(np.array(rec['score'], dtype=np.float32))[::-1]
            assert z[0] > z[1] and z[4] > z[5], (c, s, rec['index'])
            spread.add(int(T.rank_ref(np.array([rec['score']], dtype=np.float32), [rec['label']])[0]))
    assert min(spread) == 0 and any(0 < r < 5 for r in spread) and max(spread) >= 5      # hits and misses for both k


def test_seventy_pairs_count_what_seventy_single_runs_count(tiny):
    res = tiny['plain']
    assert len(tiny['pairs']) == 70 and list(res['imagenet_c']) == ['%s/%d' % p for p in tiny['pairs']]
    assert _counts(res, tiny['pairs']) == tiny['single']
    assert len(set(tiny['single'].values())) > 1 and any(a > 0 for a, _ in tiny['single'].values())
    assert _counts(tiny['scores'], tiny['pairs']) == tiny['single'] and _counts(tiny['ranks'], tiny['pairs']) == tiny['single']


def test_printed_summary(tiny):
    res = tiny['plain']
    lines = [ln for ln in tiny['plain_out'].splitlines() if ln.startswith('{')]
    assert len(lines) == 1 and json.loads(lines[0]) == json.loads(json.dumps(res))
    assert set(res) == {'imagenet_c', 'error', 'Mean', 'skipped', 'count', 'world_size', 'seconds'}
    assert res['skipped'] == ['frost'] and res['count'] == N and res['world_size'] == 1
    assert list(res['error']) == tiny['names']
    for c in tiny['names']:
        top1 = [res['imagenet_c']['%s/%d' % (c, s)]['top1'] for s in (1, 2, 3, 4, 5)]
        assert res['error'][c] == pytest.approx(100.0 - sum(top1) / 5, abs=1e-9)
    assert res['Mean'] == pytest.approx(sum(res['error'].values()) / 14, abs=1e-9)


def test_the_source_batch_is_read_once_and_never_written(tiny):
    assert tiny['unchanged'] == [True, True]                           # two batches of four, each read once for all 70 pairs
    assert tiny['fused'] == [(0, (1, 2, 3, 4, 5))] * 2                 # gaussian_noise: one launch per batch for the five severities


def test_score_files_are_byte_identical_to_the_single_runs(tiny):
    for c, s in tiny['pairs']:
        with open(_file(str(tiny['root'] / 'single'), 'm', c, s), 'rb') as a, open(_file(str(tiny['root'] / 'scores'), 'm', c, s), 'rb') as b:
            assert a.read() == b.read(), (c, s)
    assert sorted(os.listdir(str(tiny['root'] / 'scores' / 'm'))) == sorted('%s_%d' % p for p in tiny['pairs'])


def test_compact_files_give_the_evaluator_the_same_numbers(tiny):
    from robustart_amd import metrics as M
    ev = M.ImageNetCEvaluator(topk=(1, 5))
    for c, s in tiny['pairs']:
        full, compact = _file(str(tiny['root'] / 'scores'), 'm', c, s), _file(str(tiny['root'] / 'ranks'), 'm', c, s)
        want, got = ev.eval(full).metric, ev.eval(compact).metric
        assert got == want and got == tiny['ranks']['imagenet_c']['%s/%d' % (c, s)], (c, s)
        recs, srecs = _read(compact), _read(full)
        assert [r['index'] for r in recs] == list(range(N)) and all(list(r) == ['prediction', 'label', 'rank', 'index'] for r in recs)
        z = np.array([r['score'] for r in srecs], dtype=np.float32)
        assert [r['rank'] for r in recs] == T.rank_ref(z, [r['label'] for r in srecs]).tolist(), (c, s)
        assert [r['prediction'] for r in recs] == [r['prediction'] for r in srecs] == T.pred_ref(z).tolist()
        assert [r['label'] for r in recs] == [r['label'] for r in srecs]
        assert os.path.getsize(compact) < 80 * N


@pytest.fixture(scope='module')
def vit(tmp_path_factory):
    from PIL import Image
    from robustart_amd.model import get_model
    from robustart_amd.noise import imagenet_c as C
    from robustart_amd.train import cls_solver as S
    root = tmp_path_factory.mktemp('imagenet_c_vit')
    os.makedirs(str(root / 'frost'))
    rs = np.random.RandomState(3)
    photos = {n: rs.randint(0, 256, (256, 256, 3)).astype(np.uint8) for n in ('f2.png', 'f1.png', 'f3.png')}
    for n, a in photos.items():
        Image.fromarray(a).save(str(root / 'frost' / n))
    C.set_frost_textures([])
    mcfg = {'type': 'vit_base', 'kwargs': {'depth': 1, 'num_classes': 1000}}
    torch.manual_seed(1)
    model = get_model(mcfg).eval()
    cfg = _cfg(mcfg)
    pairs = [(c, s) for c in ('gaussian_noise', 'frost', 'contrast') for s in (2, 4)]
    kw = {'engine': 'hip', 'imagenet_c_names': 'gaussian_noise,frost,contrast', 'imagenet_c_severities': '2,4',
          'imagenet_c_frost_dir': str(root / 'frost')}
    plain, _ = _loop(S, cfg, model, **kw)
    registered = [t.copy() for t in C._frost_textures]                 # the loop registered the folder's photographs ...
    ranks, _ = _loop(S, cfg, model, save_dir=str(root / 'ranks'), **kw)
    single = _single_runs(S, cfg, model, pairs, str(root / 'single'), engine='hip')      # ... and the single frost runs use them
    C.set_frost_textures([])                                           # leave the process as it was found
    return {'root': root, 'pairs': pairs, 'plain': plain, 'ranks': ranks, 'single': single, 'registered': registered, 'photos': photos}


def test_hip_engine_pairs_against_single_runs(vit):
    assert list(vit['plain']['imagenet_c']) == ['%s/%d' % p for p in vit['pairs']] and vit['plain']['skipped'] == []
    assert _counts(vit['plain'], vit['pairs']) == vit['single'] and _counts(vit['ranks'], vit['pairs']) == vit['single']
    assert list(vit['plain']['error']) == ['gaussian_noise', 'frost', 'contrast'] and vit['plain']['count'] == N
    for c, s in vit['pairs']:
        recs = _read(_file(str(vit['root'] / 'ranks'), 'm', c, s))
        srecs = _read(_file(str(vit['root'] / 'single'), 'm', c, s))
        z = np.array([r['score'] for r in srecs], dtype=np.float32)
        # the compact file of the loop is the single run's score file, reduced: same inputs, same engine, same logits
        assert [r['rank'] for r in recs] == T.rank_ref(z, [r['label'] for r in srecs]).tolist(), (c, s)
        assert [r['prediction'] for r in recs] == T.pred_ref(z).tolist() == [r['prediction'] for r in srecs], (c, s)
    # the pairs differ from each other: a loop that scored one input six times would not pass
    preds = {p: tuple(r['prediction'] for r in _read(_file(str(vit['root'] / 'ranks'), 'm', *p))) for p in vit['pairs']}
    scores = {p: _read(_file(str(vit['root'] / 'single'), 'm', *p))[0]['score'][:8] for p in vit['pairs']}
    assert len(set(map(tuple, scores.values()))) == len(vit['pairs']), preds


def test_frost_photographs_come_from_the_folder_in_sorted_order(vit):
    assert len(vit['registered']) == 3
    for got, n in zip(vit['registered'], ('f1.png', 'f2.png', 'f3.png')):
        assert np.array_equal(got, vit['photos'][n])
