"""CPU side of the ImageNet-C scorer: the numpy reference of rart_topk_score_f32 against metrics.evaluators._topk_acc and torch.topk,
the `rank` branch of ImageNetCEvaluator against its `score` branch, and the entry's argument validation (no GPU)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import _topk_score_ref as T


@pytest.mark.parametrize('classes', [1, 5, 6, 64, 200, 1000])
def test_argsort_position_equals_the_two_compares(classes):
    z, y = T.make_logits(41, classes, seed=classes)
    z[3, classes // 2] = np.nan
    z[4, y[4]] = np.nan
    z[5, 0], z[6, classes - 1] = np.inf, -np.inf
    z[7] = -np.inf
    y[8], y[9] = -1, classes
    got = T.rank_ref(z, y)
    assert np.array_equal(got, T.rank_by_counting(z, y))
    assert got[4] == classes and got[8] == classes and got[9] == classes and got[7] == y[7]
    assert got.min() >= 0 and got.max() <= classes


@pytest.mark.parametrize('classes', [5, 6, 200, 1000])
def test_reference_against_the_evaluators_topk(classes):
    """_topk_acc (the restatement of the reference's evaluator) counts a sample for k exactly when rank < k: with ties"""
    from robustart_amd.metrics.evaluators import _topk_acc
    z, y = T.make_logits(60, classes, seed=7 + classes)
    order = np.argsort(-z, axis=1, kind='stable')
    for r in range(0, 60, 2):                       # every other label among the first seven of its row, on both sides of k = 5
        y[r] = order[r, (r // 2) % min(7, classes)]
    rank = T.rank_ref(z, y)
    acc = _topk_acc(z, y, [1, 5])
    for k, h in zip((1, 5), T.hits_ref(rank, (1, 5), classes)):
        assert acc[k] == float(h * (100.0 / 60))
    assert 0 < T.hits_ref(rank, (1,), classes)[0] < T.hits_ref(rank, (5,), classes)[0] and (classes == 5 or (rank >= 5).any())


def test_reference_against_torch_topk_on_tie_free_rows():
    rs = np.random.RandomState(3)
    z = rs.permutation(64 * 300).reshape(64, 300).astype(np.float32)          # all values distinct
    y = rs.randint(0, 300, size=64).astype(np.int64)
    y[:8] = z[:8].argsort(axis=1)[:, -5:][np.arange(8), np.arange(8) % 5]       # some labels inside the first five
    rank = T.rank_ref(z, y)
    top = torch.from_numpy(z).topk(5, dim=1).indices.numpy()
    for k in (1, 5):
        assert np.array_equal(rank < k, (top[:, :k] == y[:, None]).any(axis=1))
    assert (rank < 5).sum() >= 8 and (rank >= 5).sum() > 0
    assert np.array_equal(T.pred_ref(z), top[:, 0].astype(np.int32))


def test_prediction_is_numpy_argmax_first_nan_first_maximum():
    z = np.array([[1, 3, 3, 2], [np.nan, 5, np.nan, 9], [2, np.nan, np.inf, 1], [-np.inf] * 4, [np.inf, 1, np.inf, 0]], dtype=np.float32)
    assert T.pred_ref(z).tolist() == [1, 0, 1, 0, 0]


def test_evaluator_reads_rank_files_as_it_reads_score_files(tmp_path):
    from robustart_amd import metrics as M
    z, y = T.make_logits(50, 40, seed=11)
    y[:3] = T.pred_ref(z)[:3]                        # three certain top-1 hits and one sample that only top-5 counts
    y[3] = np.argsort(-z[3], kind='stable')[2]
    idx = list(range(50))
    a, b = str(tmp_path / 'score'), str(tmp_path / 'rank')
    w = M.ResultWriter(a)
    w.write_batch(torch.from_numpy(z), torch.from_numpy(y), idx)
    pa = w.close()
    w = M.RankWriter(b)
    w.write_batch(T.pred_ref(z), T.rank_ref(z, y), y, idx)
    pb = w.close()
    ev = M.ImageNetCEvaluator(topk=(1, 5))
    ma, mb = ev.eval(pa), ev.eval(pb)
    assert ma.metric == mb.metric and set(mb.metric) == {'top1', 'top5'} and mb.cmp_key == 'top1' and mb.v == ma.v
    assert 0.0 < mb.metric['top1'] < mb.metric['top5'] < 100.0
    with open(os.path.join(b, 'metric')) as f:
        assert json.load(f) == mb.metric
    lines = [json.loads(ln) for ln in open(pb)]
    assert all(list(ln) == ['prediction', 'label', 'rank', 'index'] for ln in lines)
    assert [ln['prediction'] for ln in lines] == [json.loads(ln)['prediction'] for ln in open(pa)]
    assert max(len(ln) for ln in open(pb)) < 70          # a few bytes per sample, whatever the number of classes


def test_topk_score_argument_checks_without_gpu():
    """Validation happens before any HIP call, so these are safe without a GPU."""
    from robustart_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(16)           # never dereferenced: the checks run first
    f = lib.rart_topk_score_f32

    def ks(*v):
        return (ctypes.c_int * len(v))(*v)
    assert f(None, 0, 1000, 1000, None, None, None, ks(1, 5), 2, None, None) == 0          # no rows: nothing launched
    assert f(None, 0, 1000, 1000, None, None, None, None, 0, None, None) == 0
    bad = [(one, -1, 1000, 1000, one, one, one, ks(1, 5), 2, one),           # rows < 0
           (one, 4, 0, 1000, one, one, one, ks(1, 5), 2, one),               # classes < 1
           (one, 4, 1000, 999, one, one, one, ks(1, 5), 2, one),             # ld < classes
           (one, 4, 1000, 1000, one, one, one, ks(1, 5), -1, one),           # n_k < 0
           (one, 4, 1000, 1000, one, one, one, ks(*range(1, 10)), 9, one),   # n_k > 8
           (one, 4, 1000, 1000, one, one, one, ks(1, 0), 2, one),            # a k < 1
           (one, 0, 1000, 1000, one, one, one, ks(-3), 1, one),              # ... also without rows
           (one, 4, 1000, 1000, one, one, one, None, 2, one),                # NULL ks
           (None, 4, 1000, 1000, one, one, one, ks(1, 5), 2, one),           # NULL logits
           (one, 4, 1000, 1000, None, one, one, ks(1, 5), 2, one)]           # NULL labels
    for args in bad:
        assert f(*args, None) == 1, args
        assert b'rart_topk_score_f32' in lib.rart_last_error_string()


def test_topk_score_wrapper_refuses_host_tensors_and_bad_shapes():
    from robustart_amd import metrics as M
    with pytest.raises(RuntimeError, match='CUDA'):          # no CPU path
        M.topk_score(torch.zeros(2, 10), torch.zeros(2, dtype=torch.int64))
