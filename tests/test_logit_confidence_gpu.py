"""rart_logit_confidence_f32 against a numpy fp64 reference written from the entry's definition (include/robustart_hip.h):
prediction / confidence / correctness over a class subset of fp32 logits.

pred and correct must equal the reference exactly.  conf is compared by relative error against fp64; the bound is 4 x the worst
relative error of torch's own fp32 CPU softmax(z).max() on the same rows (computed here from the reference, never from the kernel),
floored at 1e-6 (about 16 fp32 ulp: ten tree levels for 1000 terms, plus expf and the division); the factor 4 covers a different
order of summation.  Every case prints its measured error beside the bound (run with -s to see the table)."""
import numpy as np
import pytest
import torch

from _confidence_ref import conf_bound, reference, torch_fp32_error

pytestmark = pytest.mark.gpu

ROWS = (1, 2, 63, 64, 65, 257)
NROWS = 257
GUARD = 8


def _subset(classes, k, include, seed):
    rs = np.random.RandomState(seed)
    rest = [c for c in range(classes) if c not in include]
    pick = rs.choice(rest, k - len(include), replace=False).tolist() if k > len(include) else []
    return sorted(pick + list(include))


# (name, classes, subset or None): the issue's shapes, then the two sides of the threshold between the register and the looped kernel
CONFIGS = [
    ('1000_k200', 1000, _subset(1000, 200, (0, 999), 1)),
    ('1000_all', 1000, None),
    ('1000_k1', 1000, [517]),
    ('1000_k64', 1000, _subset(1000, 64, (), 2)),
    ('1000_k65', 1000, _subset(1000, 65, (), 3)),
    ('10_k3', 10, [1, 4, 9]),
    ('1023_all', 1023, None),
    ('21841_all', 21841, None),
    ('21841_k200', 21841, _subset(21841, 200, (21840,), 4)),
    ('1024_all', 1024, None),
    ('1025_all', 1025, None),
]

FAMILIES = ('normal_x1', 'normal_x8', 'normal_x40', 'constant', 'tie_two', 'tie_all', 'max_outside', 'plus_minus_1e4', 'some_neg_inf',
            'all_neg_inf', 'nan_inside', 'nan_outside', 'pos_inf')


def make_logits(classes, subset, seed):
    """[257][classes] fp32: row r belongs to family r % 13 (the first rows of every launch size meet the plain families, the 63-row
    launches and larger meet every family several times).  Returns (logits, family index per row)."""
    rs = np.random.RandomState(seed)
    sel = np.arange(classes) if subset is None else np.asarray(subset)
    out = np.setdiff1d(np.arange(classes), sel)
    x = rs.standard_normal((NROWS, classes)).astype(np.float32)
    fam = np.arange(NROWS) % len(FAMILIES)
    for r in range(NROWS):
        f = FAMILIES[fam[r]]
        a, b = sel[rs.randint(len(sel))], sel[rs.randint(len(sel))]
        if f == 'normal_x8':
            x[r] *= 8
        elif f == 'normal_x40':
            x[r] *= 40
        elif f == 'constant':
            x[r] = np.float32(rs.standard_normal() * 3)
        elif f == 'tie_two':
            x[r, a] = x[r, b] = x[r].max() + np.float32(0.5)
        elif f == 'tie_all':
            x[r, sel] = np.float32(1.25)                  # the maximum at every selected position; the others stay random
        elif f == 'max_outside' and len(out):
            x[r, out[rs.randint(len(out))]] = 50.0
        elif f == 'plus_minus_1e4':
            x[r] = np.where(rs.rand(classes) < 0.5, np.float32(1e4), np.float32(-1e4))
        elif f == 'some_neg_inf':
            x[r, rs.rand(classes) < 0.3] = -np.inf
            x[r, a] = 1.0                                  # at least one finite selected entry
        elif f == 'all_neg_inf':
            x[r] = -np.inf
        elif f == 'nan_inside':
            x[r, a] = np.nan
            x[r, b] = np.nan
        elif f == 'nan_outside' and len(out):
            x[r, out[rs.randint(len(out))]] = np.nan
        elif f == 'pos_inf':
            x[r, a] = np.inf
    return x, fam


def make_labels(pred, k):
    """labels equal to pred, different from pred (inside [0, K) when K > 1), -1 and K, by row % 4"""
    lab = pred.astype(np.int64).copy()
    r = np.arange(len(pred))
    lab[r % 4 == 1] = (lab[r % 4 == 1] + 1) % k if k > 1 else -1
    lab[r % 4 == 2] = -1
    lab[r % 4 == 3] = k
    return lab


def launch(logits_dev, rows, classes, ld, subset_dev, labels_dev, first_row=0):
    """the raw entry on rows [first_row, first_row + rows) of a [*, ld] buffer, outputs inside guard bands that must stay untouched"""
    from robustart_amd import _lib
    lib = _lib.load()
    pred = torch.full((rows + 2 * GUARD,), -7, dtype=torch.int32, device='cuda')
    conf = torch.full((rows + 2 * GUARD,), -7.0, dtype=torch.float32, device='cuda')
    corr = torch.full((rows + 2 * GUARD,), 77, dtype=torch.uint8, device='cuda')
    n_sub = 0 if subset_dev is None else subset_dev.numel()
    _lib.check(lib.rart_logit_confidence_f32(logits_dev.data_ptr() + 4 * ld * first_row, rows, classes, ld, _lib.ptr(subset_dev), n_sub,
                                             None if labels_dev is None else labels_dev.data_ptr() + 8 * first_row,
                                             pred.data_ptr() + 4 * GUARD, conf.data_ptr() + 4 * GUARD, corr.data_ptr() + GUARD,
                                             _lib.stream_ptr()))
    pred, conf, corr = pred.cpu().numpy(), conf.cpu().numpy(), corr.cpu().numpy()
    for buf, fill in ((pred, -7), (conf, -7.0), (corr, 77)):
        assert (buf[:GUARD] == fill).all() and (buf[GUARD + rows:] == fill).all(), 'guard band written'
    return pred[GUARD:GUARD + rows], conf[GUARD:GUARD + rows], corr[GUARD:GUARD + rows]


def check(got, want_pred, want_conf, want_corr, ref_err, what):
    pred, conf, corr = got
    n = len(pred)
    assert np.array_equal(pred, want_pred[:n]), what
    assert np.array_equal(corr, want_corr[:n]), what
    fin = np.isfinite(want_conf[:n])
    assert np.array_equal(np.isnan(conf), ~fin), what                     # NaN exactly where the contract says so
    bound = conf_bound(ref_err[:n])
    err = float((np.abs(conf[fin].astype(np.float64) - want_conf[:n][fin]) / want_conf[:n][fin]).max()) if fin.any() else 0.0
    print('%-28s rows %3d  conf rel err %.3e  bound %.3e  (torch fp32 softmax %.3e)' % (what, n, err, bound, float(ref_err[:n].max())))
    assert err <= bound, (what, err, bound)
    return err


@pytest.mark.parametrize('name,classes,subset', CONFIGS, ids=[c[0] for c in CONFIGS])
def test_against_fp64(name, classes, subset):
    x, fam = make_logits(classes, subset, seed=classes + (0 if subset is None else len(subset)))
    k = classes if subset is None else len(subset)
    z = x if subset is None else x[:, subset]
    want_pred, want_conf = reference(z)
    ref_err = torch_fp32_error(z, want_conf)
    labels = make_labels(want_pred, k)
    want_corr = (labels == want_pred).astype(np.uint8)
    # what the families promise, stated on the reference so that a mistake in make_logits cannot hide
    for f, r in ((f, int(np.argmax(fam == FAMILIES.index(f)))) for f in FAMILIES):
        if f in ('constant', 'tie_all'):
            assert want_pred[r] == 0 and np.float32(want_conf[r]) == np.float32(1.0) / np.float32(k)
        if f in ('all_neg_inf', 'nan_inside', 'pos_inf'):
            assert np.isnan(want_conf[r])
        if f in ('nan_outside', 'max_outside', 'some_neg_inf', 'plus_minus_1e4'):
            assert np.isfinite(want_conf[r])
    sub_dev = None if subset is None else torch.tensor(subset, dtype=torch.int32, device='cuda')
    lab_dev = torch.from_numpy(labels).cuda()
    full = {}
    for ld in (classes, classes + 1, classes + 24):
        buf = torch.full((NROWS, ld), float('nan'), dtype=torch.float32, device='cuda')     # a NaN in the padding would show in conf
        buf[:, :classes] = torch.from_numpy(x).cuda()
        for rows in ROWS:
            got = launch(buf, rows, classes, ld, sub_dev, lab_dev)
            check(got, want_pred, want_conf, want_corr, ref_err, '%s ld=%d' % (name, ld))
            if rows == NROWS:
                full[ld] = got
        # constant rows give 1 / K rounded, exactly
        for f in ('constant', 'tie_all'):
            rr = np.where(fam == FAMILIES.index(f))[0]
            assert (full[ld][1][rr] == np.float32(1.0) / np.float32(k)).all() and (full[ld][0][rr] == 0).all()
    # the outputs do not depend on the row stride
    for ld in (classes + 1, classes + 24):
        for a, b in zip(full[classes], full[ld]):
            assert a.tobytes() == b.tobytes()
    # row r computed alone == row r of the 257-row launch, byte for byte (every family twice, and the last row)
    assert buf.shape[1] == classes + 24                    # the last buffer of the loop above
    for r in list(range(2 * len(FAMILIES))) + [NROWS - 1]:
        alone = launch(buf, 1, classes, classes + 24, sub_dev, lab_dev, first_row=r)
        for a, b in zip(alone, full[classes + 24]):
            assert a.tobytes() == b[r:r + 1].tobytes(), (name, r, FAMILIES[fam[r]])
    # no labels: correct is 0 everywhere, pred and conf unchanged
    got = launch(buf, NROWS, classes, classes + 24, sub_dev, None)
    assert not got[2].any() and got[0].tobytes() == full[classes][0].tobytes() and got[1].tobytes() == full[classes][1].tobytes()


def test_all_classes_spellings_agree():
    """NULL subset, n_subset == 0 with a pointer, and the identity subset select the same K values in the same order: same bytes"""
    from robustart_amd import _lib
    x, _ = make_logits(1000, None, seed=5)
    buf = torch.from_numpy(x).cuda()
    a = launch(buf, NROWS, 1000, 1000, None, None)
    ident = torch.arange(1000, dtype=torch.int32, device='cuda')
    b = launch(buf, NROWS, 1000, 1000, ident, None)
    lib = _lib.load()
    pred = torch.empty(NROWS, dtype=torch.int32, device='cuda')
    conf = torch.empty(NROWS, dtype=torch.float32, device='cuda')
    corr = torch.empty(NROWS, dtype=torch.uint8, device='cuda')
    _lib.check(lib.rart_logit_confidence_f32(buf.data_ptr(), NROWS, 1000, 1000, ident.data_ptr(), 0, None, pred.data_ptr(), conf.data_ptr(),
                                             corr.data_ptr(), _lib.stream_ptr()))
    for u, v, w in zip(a, b, (pred, conf, corr)):
        assert u.tobytes() == v.tobytes() == w.cpu().numpy().tobytes()


def test_more_rows_than_waves_in_the_grid():
    """the grid holds 2048 blocks of four waves: 8192 + 5 rows make the first waves take a second row"""
    rows, classes, subset = 8192 + 5, 10, [1, 4, 9]
    rs = np.random.RandomState(9)
    x = rs.standard_normal((rows, classes)).astype(np.float32) * 3
    want_pred, want_conf = reference(x[:, subset])
    labels = make_labels(want_pred, 3)
    got = launch(torch.from_numpy(x).cuda(), rows, classes, classes, torch.tensor(subset, dtype=torch.int32, device='cuda'),
                 torch.from_numpy(labels).cuda())
    check(got, want_pred, want_conf, (labels == want_pred).astype(np.uint8), torch_fp32_error(x[:, subset], want_conf), 'grid stride')


def test_python_wrapper_views_labels_and_sync_free():
    from robustart_amd.metrics import class_subset, subset_confidence
    subset = CONFIGS[0][2]
    x, _ = make_logits(1000, subset, seed=6)
    want_pred, want_conf = reference(x[:, subset])
    ref_err = torch_fp32_error(x[:, subset], want_conf)
    labels = make_labels(want_pred, len(subset))
    want_corr = (labels == want_pred).astype(np.uint8)
    wide = torch.full((NROWS + 6, 1031), float('nan'), dtype=torch.float32, device='cuda')
    view = wide[3:3 + NROWS, 5:1005]                       # a row-strided view that starts 20 bytes into a row: no alignment to rely on
    view.copy_(torch.from_numpy(x).cuda())
    assert not view.is_contiguous()
    sub = class_subset(subset, 1000, 'cuda')
    lab = torch.from_numpy(labels).cuda()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')                # a device-to-host read inside the call would raise
    try:
        pred, conf, corr = subset_confidence(view, sub, lab)
        p2, c2, k2 = subset_confidence(view, sub, None)
        p3, c3, k3 = subset_confidence(view[:1], None, None)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert (pred.dtype, conf.dtype, corr.dtype) == (torch.int32, torch.float32, torch.uint8)
    check((pred.cpu().numpy(), conf.cpu().numpy(), corr.cpu().numpy()), want_pred, want_conf, want_corr, ref_err, 'wrapper, strided view')
    assert torch.equal(p2, pred) and c2.cpu().numpy().tobytes() == conf.cpu().numpy().tobytes() and not k2.any()
    all_pred, all_conf = reference(x[:1])
    assert p3.tolist() == all_pred.tolist() and abs(float(c3[0]) - all_conf[0]) <= 1e-6 * all_conf[0] and k3.tolist() == [0]
    empty = subset_confidence(view[:0], sub, None)
    assert [t.numel() for t in empty] == [0, 0, 0]
    with pytest.raises(RuntimeError, match='CUDA'):
        subset_confidence(view.cpu(), None, None)
    with pytest.raises(ValueError):
        subset_confidence(view.double(), sub, None)
    with pytest.raises(ValueError):
        subset_confidence(wide[:, ::2], None, None)        # classes not contiguous
    with pytest.raises(ValueError):
        subset_confidence(view, sub.long(), None)
