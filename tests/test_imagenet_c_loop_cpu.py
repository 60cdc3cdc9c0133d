"""Host side of `cls_solver --evaluate --imagenet-c`: the argument and config errors (all raised before a model, a dataset or the
device is touched), the default corruption list, frost left out or refused, and RankWriter's files for world sizes 1 and 2."""
import json
import os

import numpy as np
import pytest
import torch

CPU = torch.device('cpu')


class _Args:
    engine = 'hip'
    evaluate = True
    imagenet_c = True
    imagenet_c_names = None
    imagenet_c_severities = None
    imagenet_c_frost_dir = None
    imagenet_c_scores = False
    imagenet_s = False
    corruption = None
    attack = None
    save_dir = None
    seed = 0


def _cfg(**test):
    # a model type the registry does not know: building it would raise NotImplementedError, so reaching the RuntimeError of the
    # device check proves that nothing was built before it
    return {'model': {'type': 'no_such_model'}, 'data': {'read_from': 'no_such_reader', 'batch_size': 4, 'test': dict(test)}}


@pytest.fixture
def no_frost(monkeypatch):
    from robustart_amd.noise import imagenet_c as C
    monkeypatch.setattr(C, '_frost_textures', [])
    monkeypatch.setattr(C, '_frost_dev', {})
    return C


def _args(**kw):
    a = _Args()
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_default_lists(no_frost):
    from robustart_amd.train import cls_solver as S
    C = no_frost
    assert S.imagenet_c_names() == (list(C.CORRUPTION_NAMES[:15]), False)
    assert S.imagenet_c_names()[0][-1] == 'jpeg_compression' and len(S.imagenet_c_names('all')[0]) == 19
    assert S.imagenet_c_names('all')[0][15:] == ['speckle_noise', 'gaussian_blur', 'spatter', 'saturate']
    assert S.imagenet_c_names(' fog, snow ') == (['fog', 'snow'], True)
    assert S.imagenet_c_severities() == [1, 2, 3, 4, 5] and S.imagenet_c_severities('5, 1') == [5, 1]


@pytest.mark.parametrize('kw', [
    {'imagenet_c_names': 'fog,smog'},                   # an unknown name
    {'imagenet_c_names': 'fog,fog'},
    {'imagenet_c_names': ' , '},                        # an empty list
    {'imagenet_c_names': ''},
    {'imagenet_c_severities': '0'},                     # outside 1..5
    {'imagenet_c_severities': '1,6'},
    {'imagenet_c_severities': '2.5'},
    {'imagenet_c_severities': ''},
    {'imagenet_c_severities': '3,3'},
    {'attack': 'pgd_linf'},
    {'corruption': 'fog'},
    {'imagenet_s': True},
    {'imagenet_c_scores': True},                        # without --save-dir
    {'imagenet_c_names': 'fog,frost'},                  # frost named explicitly, no photographs
])
def test_value_errors_before_anything_is_built(no_frost, kw):
    from robustart_amd.train import cls_solver as S
    with pytest.raises(ValueError):
        S.evaluate_imagenet_c(_cfg(), _args(**kw), 0, 1, CPU)
    with pytest.raises(ValueError):
        S.evaluate(_cfg(), _args(**kw), 0, 1, CPU)        # ... and through the dispatch, ahead of the ImageNet-S loop's own checks


def test_natural_mode_is_refused(no_frost):
    from robustart_amd.train import cls_solver as S
    with pytest.raises(ValueError, match='imagenet_a&o'):
        S.evaluate(_cfg(**{'imagenet_a&o': True}), _args(), 0, 1, CPU)


def test_cpu_device_is_a_runtime_error_after_the_checks(no_frost, tmp_path):
    from robustart_amd.train import cls_solver as S
    for kw in ({}, {'imagenet_c_names': 'fog', 'imagenet_c_severities': '2'}, {'imagenet_c_scores': True, 'save_dir': str(tmp_path)},
               {'attack': 'none'}):
        with pytest.raises(RuntimeError, match='GPU'):
            S.evaluate(_cfg(), _args(**kw), 0, 1, CPU)
    assert os.listdir(str(tmp_path)) == []                # no writer was opened either

    class Bare:                                           # an argument object from before this option: the old path, not the loop
        engine, corruption, attack, severity, seed = 'torch', None, None, 3, 0
    with pytest.raises(NotImplementedError):
        S.evaluate(_cfg(), Bare(), 0, 1, CPU)


def test_frost_is_left_out_implicitly_and_refused_explicitly(no_frost, tmp_path):
    from robustart_amd.train import cls_solver as S
    C = no_frost
    plan = S.imagenet_c_plan(_cfg(), _args())
    assert plan['skipped'] == ['frost'] and 'frost' not in plan['names'] and len(plan['names']) == 14
    assert plan['names'] == [n for n in C.CORRUPTION_NAMES[:15] if n != 'frost'] and plan['severities'] == [1, 2, 3, 4, 5]
    plan = S.imagenet_c_plan(_cfg(), _args(imagenet_c_names='all'))
    assert plan['skipped'] == ['frost'] and len(plan['names']) == 18
    with pytest.raises(ValueError, match='frost'):
        S.imagenet_c_plan(_cfg(), _args(imagenet_c_names='frost'))
    assert S.imagenet_c_plan(_cfg(), _args(imagenet_c_names='fog'))['skipped'] == []
    # photographs named by the option, by the config key, or registered earlier: frost runs
    for cfg, a in ((_cfg(), _args(imagenet_c_frost_dir=str(tmp_path))), (_cfg(imagenet_c_frost_dir=str(tmp_path)), _args())):
        plan = S.imagenet_c_plan(cfg, a)
        assert plan['skipped'] == [] and plan['names'] == list(C.CORRUPTION_NAMES[:15]) and plan['frost_dir'] == str(tmp_path)
    C.set_frost_textures([np.zeros((230, 230, 3), np.uint8)])
    plan = S.imagenet_c_plan(_cfg(), _args(imagenet_c_names='frost,fog'))
    assert plan['skipped'] == [] and plan['names'] == ['frost', 'fog'] and plan['frost_dir'] is None


def test_frost_folder_is_read_in_sorted_order(tmp_path):
    from PIL import Image
    from robustart_amd.train import cls_solver as S
    rs = np.random.RandomState(0)
    arrays = {n: rs.randint(0, 256, (230 + k, 240, 3)).astype(np.uint8) for k, n in enumerate(['b.png', 'a.png', 'c.png'])}
    for n, a in arrays.items():
        Image.fromarray(a).save(str(tmp_path / n))
    got = S.read_frost_textures(str(tmp_path))
    assert len(got) == 3 and all(g.dtype == np.uint8 for g in got)
    for g, n in zip(got, ['a.png', 'b.png', 'c.png']):
        assert np.array_equal(g, arrays[n])
    os.makedirs(str(tmp_path / 'empty'))
    for bad in (str(tmp_path / 'empty'), str(tmp_path / 'missing')):
        with pytest.raises(ValueError):
            S.read_frost_textures(bad)


def test_main_checks_the_options_before_the_config_is_read(tmp_path):
    from robustart_amd.train import cls_solver as S
    missing = str(tmp_path / 'no_config.yaml')
    with pytest.raises(ValueError, match='--evaluate'):
        S.main(['--config', missing, '--imagenet-c'])
    with pytest.raises(ValueError, match='smog'):
        S.main(['--config', missing, '--evaluate', '--imagenet-c', '--imagenet-c-names', 'smog'])
    with pytest.raises(ValueError, match='severity'):
        S.main(['--config', missing, '--evaluate', '--imagenet-c', '--imagenet-c-severities', '9'])


def test_rank_writer_round_trip_and_merge_order(tmp_path):
    from robustart_amd import metrics as M
    from robustart_amd.train.cls_solver import shard_indices
    n = 11
    pred = np.arange(n, dtype=np.int32) * 7 % 10
    rank = np.arange(n, dtype=np.int32) * 3 % 8
    lab = np.arange(n, dtype=np.int64) * 5 % 10
    files = {}
    for world in (1, 2):
        d = str(tmp_path / ('w%d' % world))
        writers = [M.RankWriter(d, r, world) for r in range(world)]
        for r in reversed(range(world)):                              # the higher rank writes first, in batches of 4
            idx = shard_indices(n, r, world)
            for s in range(0, len(idx), 4):
                it = idx[s:s + 4]
                writers[r].write_batch(torch.from_numpy(pred[it]), torch.from_numpy(rank[it]), lab[it], it)
        for r in reversed(range(1, world)):
            writers[r].close()
        files[world] = writers[0].close()                             # rank 0 merges
        recs = [json.loads(ln) for ln in open(files[world])]
        assert [r['index'] for r in recs] == list(range(n))
        assert [(r['prediction'], r['label'], r['rank']) for r in recs] == list(zip(pred.tolist(), lab.tolist(), rank.tolist()))
        assert all(list(r) == ['prediction', 'label', 'rank', 'index'] for r in recs)
    assert open(files[1], 'rb').read() == open(files[2], 'rb').read()
    m = M.ImageNetCEvaluator().eval(files[2]).metric
    assert m == {'top1': float((rank < 1).sum() * (100.0 / n)), 'top5': float((rank < 5).sum() * (100.0 / n))}
