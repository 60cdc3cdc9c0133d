"""Calibration and out-of-distribution measures of the ImageNet-A / ImageNet-O evaluation, in numpy fp64.

A mirror of RobustART/metrics/calibration_tools.py:26-63 (calib_err, aurra) and :138-191 (fpr_and_fdr_at_recall, get_measures)
without its two imports that this path cannot satisfy: sklearn (roc_auc_score, average_precision_score) and the `prototype` logger,
which is not in the reference's tree.  The two sklearn quantities are written out from their definitions:
    AUPR   average precision: sum over the distinct score thresholds of (recall_k - recall_{k-1}) * precision_k, a step function
    AUROC  the trapezoid rule over the ROC points of the distinct thresholds (sklearn drops collinear points first, which can move
           the last bits)
Both work on distinct thresholds, so tied scores enter as one point: fp32 confidences saturate at exactly 1.0, and a run of ties
there is the common case, not a corner.
Out of scope: temperature tuning (tune_temp) and soft_f1.
"""
import numpy as np

recall_level_default = 0.95


def calib_err(confidence, correct, p='2', beta=100):
    """calibration_tools.py:26-56, as written: samples sorted by confidence, bins of `beta` samples (the last one takes the
    remainder), and the loop runs over `range(len(bins) - 1)`, so the LAST bin -- the most confident samples -- is left out of the
    error while the weights still divide by the total count.  With fewer than 2 * beta samples there is one bin and the result is 0.
    p: '2' (RMS), '1' (mean absolute), 'infty' / 'infinity' / 'max'.
    One departure: fewer samples than beta leaves no bin, an IndexError on `bins[-1]` in the reference; here a ValueError naming the
    two numbers."""
    confidence = np.asarray(confidence, dtype=np.float64).reshape(-1)
    correct = np.asarray(correct, dtype=np.float64).reshape(-1)
    if p not in ('1', '2', 'infty', 'infinity', 'max'):
        raise ValueError("calib_err: p must be '1', '2' or 'infty', got %r" % (p,))
    if len(confidence) < beta:
        raise ValueError('calib_err: %d samples are fewer than one bin of beta = %d' % (len(confidence), beta))
    idxs = np.argsort(confidence)
    confidence = confidence[idxs]
    correct = correct[idxs]
    bins = [[i * beta, (i + 1) * beta] for i in range(len(confidence) // beta)]
    bins[-1] = [bins[-1][0], len(confidence)]
    cerr = 0
    total_examples = len(confidence)
    for i in range(len(bins) - 1):
        bin_confidence = confidence[bins[i][0]:bins[i][1]]
        bin_correct = correct[bins[i][0]:bins[i][1]]
        num_examples_in_bin = len(bin_confidence)
        if num_examples_in_bin > 0:
            difference = np.abs(np.nanmean(bin_confidence) - np.nanmean(bin_correct))
            if p == '2':
                cerr += num_examples_in_bin / total_examples * np.square(difference)
            elif p == '1':
                cerr += num_examples_in_bin / total_examples * difference
            else:
                cerr = np.maximum(cerr, difference)
    if p == '2':
        cerr = np.sqrt(cerr)
    return float(cerr)


def aurra(confidence, correct):
    """calibration_tools.py:59-63: area under the response-rate / accuracy curve -- the mean over k of the accuracy of the k most
    confident samples."""
    confidence = np.asarray(confidence, dtype=np.float64).reshape(-1)
    conf_ranks = np.argsort(confidence)[::-1]
    rra_curve = np.cumsum(np.asarray(correct, dtype=np.float64).reshape(-1)[conf_ranks])
    rra_curve = rra_curve / np.arange(1, len(rra_curve) + 1)
    return float(np.mean(rra_curve))


def _clf_curve(y_true, y_score):
    """(fps, tps, thresholds) at the distinct score values, scores descending: the curve both sklearn measures start from."""
    y_true = np.asarray(y_true).reshape(-1) == 1
    y_score = np.asarray(y_score, dtype=np.float64).reshape(-1)
    order = np.argsort(y_score, kind='mergesort')[::-1]
    y_score, y_true = y_score[order], y_true[order]
    threshold_idxs = np.r_[np.where(np.diff(y_score))[0], y_true.size - 1]
    tps = np.cumsum(y_true, dtype=np.float64)[threshold_idxs]
    fps = 1 + threshold_idxs - tps
    return fps, tps, y_score[threshold_idxs]


def fpr_at_recall(y_true, y_score, recall_level=recall_level_default):
    """calibration_tools.py:138-178 (fpr_and_fdr_at_recall with pos_label = 1): the false-positive rate at the threshold whose
    recall is closest to recall_level."""
    fps, tps, thresholds = _clf_curve(y_true, y_score)
    n_neg = np.sum(np.logical_not(np.asarray(y_true).reshape(-1) == 1))
    recall = tps / tps[-1]
    last_ind = tps.searchsorted(tps[-1])
    sl = slice(last_ind, None, -1)
    recall, fps = np.r_[recall[sl], 1], np.r_[fps[sl], 0]
    cutoff = np.argmin(np.abs(recall - recall_level))
    return float(fps[cutoff] / n_neg)


def _auroc(fps, tps):
    fpr, tpr = np.r_[0.0, fps] / fps[-1], np.r_[0.0, tps] / tps[-1]
    return float(np.sum(np.diff(fpr) * (tpr[1:] + tpr[:-1]) / 2.0))


def _average_precision(fps, tps):
    precision = tps / (tps + fps)
    recall = tps / tps[-1]
    # sklearn's order of summation: the curve reversed, closed with (recall 0, precision 1)
    precision, recall = np.r_[precision[::-1], 1.0], np.r_[recall[::-1], 0.0]
    return float(-np.sum(np.diff(recall) * precision[:-1]))


def get_measures(_pos, _neg, recall_level=recall_level_default):
    """calibration_tools.py:180-191 -> (auroc, aupr, fpr): `_pos` are the scores of the positive class (label 1), `_neg` of the
    negative one; a higher score means "more positive"."""
    pos = np.asarray(_pos, dtype=np.float64).reshape(-1)
    neg = np.asarray(_neg, dtype=np.float64).reshape(-1)
    if len(pos) == 0 or len(neg) == 0:
        raise ValueError('get_measures: %d positive and %d negative scores: both classes are needed' % (len(pos), len(neg)))
    examples = np.concatenate([pos, neg])
    labels = np.zeros(len(examples), dtype=np.int32)
    labels[:len(pos)] += 1
    fps, tps, _ = _clf_curve(labels, examples)
    return _auroc(fps, tps), _average_precision(fps, tps), fpr_at_recall(labels, examples, recall_level)
