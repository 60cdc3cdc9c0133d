"""cls_solver after its split into train/data.py, train/checkpoint.py and train/evaluate.py: every name tests and profiles import from
cls_solver is still there and is the home module's object, and the plain evaluation loop on the CPU (torch engine, fake data, a ragged
last batch) returns the counts a sort of the module's own logits gives and writes its result file in index order."""
import contextlib
import importlib
import io
import json
import os

import pytest
import torch

from _tiny_eval_model import tiny_eval_model

HOME = {
    'data': 'FileImageNet FakeImageNet StructuredFakeImageNet read_transforms make_dataset EpochSampler shard_indices IMAGENET_MEAN '
            'IMAGENET_STD',
    'checkpoint': 'load_pretrain load_checkpoint_file save_checkpoint build_model',
    'evaluate': 'parse_eps topk_correct all_reduce_counters evaluate evaluate_natural evaluate_imagenet_s evaluate_imagenet_c '
                'imagenet_c_plan imagenet_c_names imagenet_c_severities imagenet_s_ops read_frost_textures natural_mode natural_datasets',
    'cls_solver': 'cosine_lr resolve_schedule init_dist train main',
}
NAMES = [(mod, name) for mod, names in HOME.items() for name in names.split()]
N, BS = 8, 3


def test_every_name_is_reachable_from_cls_solver():
    from robustart_amd.train import cls_solver as S
    assert len(NAMES) == 32
    for _, name in NAMES:
        assert hasattr(S, name), name


@pytest.mark.parametrize('mod,name', NAMES)
def test_each_name_is_the_object_of_its_home_module(mod, name):
    from robustart_amd.train import cls_solver as S
    assert getattr(S, name) is getattr(importlib.import_module('robustart_amd.train.' + mod), name)


class _Args:
    engine = 'torch'
    corruption = None
    attack = None
    eps = '2/255'
    steps = 0
    severity = 3
    seed = 0
    precision = None
    save_dir = None
    src_name = None
    tgt_name = None
    tgt_type = None
    imagenet_c = False
    imagenet_s = False
    imagenet_s_ops = None
    imagenet_c_names = None
    imagenet_c_severities = None
    imagenet_c_frost_dir = None
    imagenet_c_scores = False


class _BareArgs:
    """what a caller's plain class carries at the least: no imagenet_* attribute, no precision, no names"""
    engine = 'torch'
    corruption = None
    attack = None


@pytest.fixture(scope='module')
def scored():
    """the model and, from its own logits by a full sort, the rank of every sample's label -> (model, top-1 count, top-5 count)"""
    from robustart_amd.train import cls_solver as S
    model = tiny_eval_model(N)
    x, y = S.FakeImageNet(N, 224).batch(range(N), 'cpu')
    mean, std = torch.tensor(S.IMAGENET_MEAN).view(1, 3, 1, 1), torch.tensor(S.IMAGENET_STD).view(1, 3, 1, 1)
    with torch.no_grad():
        lg = model((x.permute(0, 3, 1, 2).float() / 255.0 - mean) / std)
    vals, order = torch.sort(lg, dim=1, descending=True)
    assert bool((vals[:, :-1] > vals[:, 1:])[:, :8].all()), 'a tie among the top logits: the counts would depend on the tie rule'
    ranks = [order[i].tolist().index(int(y[i])) for i in range(N)]
    c1, c5 = sum(r < 1 for r in ranks), sum(r < 5 for r in ranks)
    assert 0 < c1 < c5 < N, ranks                       # labels on both sides of k = 1 and of k = 5
    return model, c1, c5, y.tolist(), lg.argmax(1).tolist()


def _evaluate(args, model):
    from robustart_amd.train import cls_solver as S
    cfg = {'model': {'type': 'tiny_eval_test'}, 'data': {'fake_size': N, 'batch_size': BS, 'input_size': 224, 'read_from': 'fake'}}
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        res = S.evaluate(cfg, args, 0, 1, torch.device('cpu'), model=model)
    assert json.loads(buf.getvalue()) == res            # one printed line on rank 0: the returned dict
    return res


def _check(res, scored):
    _, c1, c5, _, _ = scored
    assert res['count'] == N and res['world_size'] == 1 and res['noise'] == 'none'
    assert res['top1'] == c1 / N and res['top5'] == c5 / N


def test_plain_evaluate_on_the_cpu_counts_and_writes_in_index_order(tmp_path, scored):
    args = _Args()
    args.save_dir = str(tmp_path)
    _check(_evaluate(args, scored[0]), scored)
    with open(os.path.join(str(tmp_path), 'tiny_eval_test', 'none_0', 'results.txt.all')) as f:
        recs = [json.loads(ln) for ln in f]
    assert [r['index'] for r in recs] == list(range(N))           # 3 + 3 + 2: the ragged last batch is there, once
    assert [r['label'] for r in recs] == scored[3]
    assert [r['prediction'] for r in recs] == scored[4]


def test_plain_evaluate_takes_a_bare_argument_class(scored):
    _check(_evaluate(_BareArgs(), scored[0]), scored)
