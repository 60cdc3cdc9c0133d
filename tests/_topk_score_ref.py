"""The definition of rart_topk_score_f32 (include/robustart_hip.h) in numpy: the label's position in a stable descending argsort of
the row, numpy.argmax for the prediction, and the hit counts.  tests/test_topk_score_ref_cpu.py checks it against
metrics.evaluators._topk_acc and torch.topk; tests/test_topk_score_gpu.py compares the kernel with it exactly."""
import numpy as np


def rank_ref(z, labels):
    """z: fp32 [rows, classes], labels: ints [rows] -> int32 [rows].  np.argsort(-z, stable) orders a row by descending value with
    ties to the lower index and NaNs last, so a NaN never stands before the label; a label outside [0, classes) or a NaN at the
    label gives `classes`."""
    z = np.asarray(z, dtype=np.float32)
    labels = np.asarray(labels, dtype=np.int64).reshape(-1)
    rows, classes = z.shape
    out = np.full(rows, classes, dtype=np.int32)
    ok = (labels >= 0) & (labels < classes)
    if ok.any():
        zz, yy = z[ok], labels[ok]
        order = np.argsort(-zz, axis=1, kind='stable')
        pos = np.argmax(order == yy[:, None], axis=1).astype(np.int32)
        pos[np.isnan(zz[np.arange(len(yy)), yy])] = classes
        out[ok] = pos
    return out


def rank_by_counting(z, labels):
    """the same number by the two compares the header states: #{j : z_j > z_y} + #{j < y : z_j == z_y}"""
    z = np.asarray(z, dtype=np.float32)
    rows, classes = z.shape
    out = np.full(rows, classes, dtype=np.int32)
    with np.errstate(invalid='ignore'):
        for r, y in enumerate(np.asarray(labels, dtype=np.int64).reshape(-1)):
            if 0 <= y < classes and not np.isnan(z[r, y]):
                out[r] = int((z[r] > z[r, y]).sum() + (z[r, :y] == z[r, y]).sum())
    return out


def pred_ref(z):
    """the lowest index of the maximum, the first NaN if there is one: numpy.argmax"""
    return np.argmax(np.asarray(z, dtype=np.float32), axis=1).astype(np.int32)


def hits_ref(rank, ks, classes):
    """per k the number of rows with rank < k; rank == classes (no valid label) is a miss for every k, also for k > classes"""
    rank = np.asarray(rank)
    return [int(((rank < k) & (rank < classes)).sum()) for k in ks]


def make_logits(rows, classes, seed):
    """Rows of five kinds by r % 5: continuous normals; normals on a grid of 1/2 (many exact ties); two values only; a constant row;
    a single peak on a constant floor.  Labels uniform over the classes."""
    rs = np.random.RandomState(seed)
    z = rs.randn(rows, classes).astype(np.float32)
    kind = np.arange(rows) % 5
    z[kind == 1] = np.round(z[kind == 1] * 2) / 2
    z[kind == 2] = (z[kind == 2] > 0.3).astype(np.float32)
    z[kind == 3] = 1.25
    z[kind == 4] = -3.0
    for r in np.nonzero(kind == 4)[0]:
        z[r, rs.randint(classes)] = 2.0
    labels = rs.randint(0, classes, size=rows).astype(np.int64)
    return z, labels
