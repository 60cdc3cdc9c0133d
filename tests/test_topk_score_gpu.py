"""rart_topk_score_f32 (csrc/topk_score.hip) against its numpy definition (tests/_topk_score_ref.py), exactly: the outputs are
integers.  Row lengths on both sides of the wave (64) and of the 16-byte quad, aligned rows (16-byte loads) and rows that start on
an odd float (element loads), ties, special values, labels outside the classes, and the counters: added to, never cleared."""
import numpy as np
import pytest
import torch

import _topk_score_ref as T

pytestmark = pytest.mark.gpu

CLASSES = [1, 5, 6, 63, 64, 65, 200, 1000, 1024, 1025, 21841]
# one trip of the grid-stride loop covers kMaxBlocks * kWaves = 2048 * 4 rows (csrc/topk_score.hip)
ROWS_PER_TRIP = 2048 * 4


def _device_view(z, pad, offset):
    """z [rows, classes] -> a CUDA view with row stride classes + pad whose first element sits `offset` floats into a fresh
    allocation; the padding holds +inf, which would outrank everything if the kernel read it"""
    rows, classes = z.shape
    ld = classes + pad
    buf = torch.full((rows * ld + offset,), float('inf'), dtype=torch.float32, device='cuda')
    view = buf[offset:offset + rows * ld].view(rows, ld)[:, :classes]
    view.copy_(torch.from_numpy(z))
    return view


def _run(z, y, pad=0, offset=0, ks=(1, 5), hits=None, pred=True, rank=True):
    from robustart_amd.metrics import topk_score
    view = _device_view(z, pad, offset)
    assert view.data_ptr() % 16 == (4 * offset) % 16
    p, r = topk_score(view, torch.from_numpy(np.asarray(y, dtype=np.int64)).cuda(), ks=ks, hits=hits, pred=pred, rank=rank)
    return (None if p is None else p.cpu().numpy()), (None if r is None else r.cpu().numpy())


def _check(z, y, pad=0, offset=0, ks=(1, 5)):
    hits = torch.zeros(len(ks), dtype=torch.int64, device='cuda')
    p, r = _run(z, y, pad, offset, ks, hits)
    want = T.rank_ref(z, y)
    assert p.dtype == np.int32 and r.dtype == np.int32
    assert np.array_equal(r, want)
    assert np.array_equal(p, T.pred_ref(z))
    assert hits.tolist() == T.hits_ref(want, ks, z.shape[1])
    return p, r


@pytest.mark.parametrize('layout', ['dense', 'odd'])
@pytest.mark.parametrize('classes', CLASSES)
def test_rank_prediction_and_hits_equal_the_reference(classes, layout):
    """dense: ld == classes, aligned base (16-byte loads when classes % 4 == 0).  odd: ld == classes + 3 and the base one float
    into the allocation, so no row starts on a 16-byte boundary."""
    pad, offset = (0, 0) if layout == 'dense' else (3, 1)
    for rows in (1, 3, 257):
        z, y = T.make_logits(rows, classes, seed=rows + classes)
        order = np.argsort(-z, axis=1, kind='stable')
        for r in range(0, rows, 2):                     # every other label among the first seven of its row
            y[r] = order[r, (r // 2) % min(7, classes)]
        _check(z, y, pad, offset)


@pytest.mark.parametrize('classes,pad', [(5, 3), (6, 2), (63, 1), (1001, 3), (1025, 3), (21841, 3)])
def test_aligned_rows_whose_length_is_no_multiple_of_four(classes, pad):
    """16-byte loads with a last quad that is cut short: ld % 4 == 0 and an aligned base, classes % 4 != 0"""
    z, y = T.make_logits(9, classes, seed=classes)
    y[:4] = np.argsort(-z[:4], axis=1, kind='stable')[np.arange(4), np.arange(4) % classes]
    z[5, classes - 1], y[5] = 50.0, classes - 1         # the maximum and the label in the cut quad
    z[6, classes - 1] = 50.0
    _check(z, y, pad, 0)


def test_more_rows_than_one_trip_of_the_grid_stride_loop():
    rows = 2 * ROWS_PER_TRIP + 3
    z, y = T.make_logits(rows, 8, seed=1)
    _, r = _check(z, y)
    assert (r[ROWS_PER_TRIP:] == T.rank_ref(z, y)[ROWS_PER_TRIP:]).all() and len(set(r[ROWS_PER_TRIP:].tolist())) == 8


def test_ties_go_to_the_lower_class_index():
    classes = 70
    z = np.full((3, classes), 0.5, dtype=np.float32)                    # a constant row: the label's rank is its index
    y = np.array([0, 33, classes - 1])
    p, r = _check(z, y, ks=(1, 5, 34))
    assert r.tolist() == [0, 33, classes - 1] and p.tolist() == [0, 0, 0]
    # z_y tied across the boundary of k = 5: four values above, then a run of equal values at indices 10, 20, 30
    z = np.zeros((3, classes), dtype=np.float32)
    z[:, [1, 2, 3, 4]] = [9, 8, 7, 6]
    z[:, [10, 20, 30]] = 5
    hits = torch.zeros(2, dtype=torch.int64, device='cuda')
    p, r = _run(z, [10, 20, 30], hits=hits)
    assert r.tolist() == [4, 5, 6] and p.tolist() == [1, 1, 1]           # only the first of the run is inside the first five
    assert hits.tolist() == [0, 1]
    assert np.array_equal(r, T.rank_ref(z, [10, 20, 30]))


@pytest.mark.parametrize('classes,pad,offset', [(6, 0, 0), (200, 0, 0), (200, 3, 1), (1025, 0, 0)])
def test_special_values_and_labels_outside_the_classes(classes, pad, offset):
    z, y = T.make_logits(10, classes, seed=5)
    c = classes
    z[0, y[0]] = np.nan                                  # NaN at the label: a miss, and the prediction is the first NaN
    z[1, (y[1] + 1) % c] = np.nan                        # NaN elsewhere: never outranks
    z[2, [0, c - 1]] = np.nan
    y[2] = c // 2
    z[3, c - 1], y[3] = np.inf, c - 1                    # +inf at the label
    z[4, 0], z[4, c - 1], y[4] = np.inf, np.inf, c - 1   # ... tied with an earlier +inf
    z[5, y[5]] = -np.inf                                 # -inf at the label: last but for ties
    z[6], y[6] = -np.inf, c - 1                          # a row of -inf
    y[7], y[8] = -1, c                                   # labels outside [0, classes)
    z[9], y[9] = np.nan, 0                               # a row of NaN
    p, r = _check(z, y, pad, offset, ks=(1, 5, c, c + 1, 2 ** 31 - 1))
    assert r[0] == c and p[0] == y[0]
    assert r[1] < c and p[1] == (y[1] + 1) % c and p[2] == 0
    assert r[3] == 0 and r[4] == 1 and r[6] == c - 1 and p[6] == 0
    assert r[7] == c and r[8] == c and r[9] == c and p[9] == 0
    assert r[5] == int((z[5] > -np.inf).sum() + (z[5, :y[5]] == -np.inf).sum())


def test_hits_are_added_to_and_neighbouring_slots_stay():
    from robustart_amd.metrics import topk_score
    z, y = T.make_logits(257, 200, seed=9)
    y[::2] = np.argsort(-z[::2], axis=1, kind='stable')[np.arange(129), np.arange(129) % 7]
    h1, h5 = T.hits_ref(T.rank_ref(z, y), (1, 5), 200)
    assert 0 < h1 < h5 < 257
    zd, yd = torch.from_numpy(z).cuda(), torch.from_numpy(y).cuda()
    counters = torch.tensor([11, 12, 1000, 2000, 15, 16], dtype=torch.int64, device='cuda')
    topk_score(zd, yd, ks=(1, 5), hits=counters[2:], pred=False, rank=False)              # slot 1 of three
    assert counters.tolist() == [11, 12, 1000 + h1, 2000 + h5, 15, 16]
    topk_score(zd, yd, ks=(1, 5), hits=counters[2:], pred=False, rank=False)              # again: added, not overwritten
    assert counters.tolist() == [11, 12, 1000 + 2 * h1, 2000 + 2 * h5, 15, 16]
    topk_score(zd, yd, ks=(5,), hits=counters[5:])
    assert counters.tolist() == [11, 12, 1000 + 2 * h1, 2000 + 2 * h5, 15, 16 + h5]


@pytest.mark.parametrize('ks', [(1,), (1, 5), (1, 2, 3, 5, 10, 37, 38, 1000)])
def test_sets_of_k(ks):
    z, y = T.make_logits(257, 37, seed=13)                # 37 classes: 38 and 1000 lie above them
    y[250:] = [-1, 37, -5, 10 ** 12, 0, 1, 2]
    _check(z, y, ks=ks)
    want = T.hits_ref(T.rank_ref(z, y), ks, 37)
    assert want[-1] <= 257 - 4 if ks[-1] > 37 else True    # the four labels outside the classes miss even k > classes


def test_each_output_can_be_left_out():
    z, y = T.make_logits(67, 65, seed=2)
    want_r, want_p = T.rank_ref(z, y), T.pred_ref(z)
    hits = torch.zeros(2, dtype=torch.int64, device='cuda')
    p, r = _run(z, y, hits=hits, pred=False)
    assert p is None and np.array_equal(r, want_r) and hits.tolist() == T.hits_ref(want_r, (1, 5), 65)
    hits.zero_()
    p, r = _run(z, y, hits=hits, rank=False)
    assert r is None and np.array_equal(p, want_p) and hits.tolist() == T.hits_ref(want_r, (1, 5), 65)
    p, r = _run(z, y, hits=None)
    assert np.array_equal(p, want_p) and np.array_equal(r, want_r)
    hits.zero_()
    assert _run(z, y, hits=hits, pred=False, rank=False) == (None, None) and hits.tolist() == T.hits_ref(want_r, (1, 5), 65)
    p, r = _run(z, y, ks=(), hits=hits)                   # no k: nothing counted
    assert np.array_equal(r, want_r) and hits.tolist() == T.hits_ref(want_r, (1, 5), 65)


def test_a_rows_outputs_do_not_depend_on_the_other_rows():
    z, y = T.make_logits(300, 1000, seed=4)
    p0, r0 = _run(z, y)
    z2, y2 = T.make_logits(300, 1000, seed=99)
    keep = [0, 7, 128, 299]
    z2[keep], y2[keep] = z[keep], y[keep]
    p1, r1 = _run(z2, y2)
    assert np.array_equal(p0[keep], p1[keep]) and np.array_equal(r0[keep], r1[keep])
    p2, r2 = _run(z[keep], y[keep])                       # ... nor on the row's place in the launch
    assert np.array_equal(p0[keep], p2) and np.array_equal(r0[keep], r2)


def test_wrapper_checks():
    from robustart_amd.metrics import topk_score
    z = torch.zeros(4, 10, device='cuda')
    y = torch.zeros(4, dtype=torch.int64, device='cuda')
    with pytest.raises(ValueError):
        topk_score(z.half(), y)
    with pytest.raises(ValueError):
        topk_score(z.t(), y[:4])
    with pytest.raises(ValueError):
        topk_score(z, y.int())
    with pytest.raises(ValueError):
        topk_score(z, y, ks=(0,))
    with pytest.raises(ValueError):
        topk_score(z, y, ks=(1, 5), hits=torch.zeros(1, dtype=torch.int64, device='cuda'))
    p, r = topk_score(z[:0], y[:0])
    assert p.shape == (0,) and r.shape == (0,)
