"""Evaluators over `results.txt.all` files (see package docstring for the reference anchors).

The natural-distribution evaluators at the end (ImageNet-A / -O / -P) read the lines ConfidenceWriter writes.  The reference's
`ImageNetAEvaluator` (RobustART/metrics/imageneta_evaluator.py) is a line-for-line copy of its ImageNet-P evaluator that keys its
result dict with a list: it raises TypeError and computes nothing about ImageNet-A.  The one here reports what the reference's
`calibration_tools.show_calibration_results` logs for that set -- accuracy, RMS calibration error, AURRA.
"""
import json

import numpy as np

from . import calibration


def parse_line(line):
    """First two `: value` fields of a result line, as strings (AR_evaluator.py:13-21: scan for ':' and cut the text
    from two characters later up to the next ',' or '}')."""
    res = []
    for i in range(len(line)):
        if line[i] == ':':
            for j in range(i + 2, len(line)):
                if line[j] == ',' or line[j] == '}':
                    res.append(line[i + 2:j])
                    break
    return res[0], res[1]


def _lines(path):
    with open(path) as f:
        return f.readlines()


class Metric(object):
    """RobustART/metrics/base_evaluator.py:7-24."""

    def __init__(self, metric_dict=None):
        self.metric = dict(metric_dict or {})
        self.cmp_key, self.v = None, None

    def __repr__(self):
        return 'metric=%s key=%s' % (self.metric, self.cmp_key)

    __str__ = __repr__

    def update(self, up_dict=None):
        self.metric.update(up_dict or {})

    def set_cmp_key(self, key):
        self.cmp_key = key
        self.v = self.metric[key]


def _load_res(res_file):
    res = {}
    for line in _lines(res_file):
        info = json.loads(line)
        for k, v in info.items():
            res.setdefault(k, []).append(v)
    return res


def _topk_acc(score, label, topk):
    """imagenetc_evaluator.py:55-66: torch.topk(maxk, largest, sorted) on the scores, compare with the label."""
    score = np.asarray(score, dtype=np.float64)
    label = np.asarray(label).reshape(-1)
    maxk = max(topk)
    # stable descending order (ties resolve to the lower class index, as torch.topk does for sorted output on CPU)
    order = np.argsort(-score, axis=1, kind='stable')[:, :maxk]
    correct = order == label[:, None]
    return {k: float(correct[:, :k].any(axis=1).sum() * (100.0 / len(label))) for k in topk}


class ImageNetCEvaluator(object):
    def __init__(self, topk=(1, 5)):
        self.topk = list(topk)

    def load_res(self, res_file):
        return _load_res(res_file)

    def eval(self, res_file):
        res = self.load_res(res_file)
        if 'rank' in res and 'score' not in res:
            # a RankWriter file: `rank` is the label's position in the order _topk_acc sorts the scores into, so the label is among
            # the first k exactly when rank < k -- top-k = 100 * mean(rank < k), summed the way _topk_acc sums
            rank = np.asarray(res['rank']).reshape(-1)
            acc = {k: float((rank < k).sum() * (100.0 / len(rank))) for k in self.topk}
        else:
            acc = _topk_acc(res['score'], res['label'], self.topk)
        metric = Metric({'top%d' % k: acc[k] for k in self.topk})
        metric.set_cmp_key('top%d' % self.topk[0])
        with open(res_file.replace('results.txt.all', 'metric'), 'w') as f:
            json.dump(metric.metric, f)
        return metric


class ImageNetSEvaluator(object):
    def __init__(self):
        self.metric = Metric()

    def load_res(self, res_file):
        return _load_res(res_file)

    def eval(self, res_file, decoder_type='pil', resize_type='pil-bilinear'):
        res = self.load_res(res_file)
        acc = _topk_acc(res['score'], res['label'], [1])[1]
        out = {(decoder_type, resize_type): acc}
        self.metric.update(out)
        return out

    def get_mean(self):
        return {'Mean': float(np.mean(list(self.metric.metric.values())))}

    def get_std(self):
        return {'Std.': float(np.std(list(self.metric.metric.values())))}

    def clear(self):
        self.metric.metric = {}


class AdvRobustEvaluator(object):
    parse_line = staticmethod(parse_line)

    def eval(self, clean_path, adv_path, num=None):
        lines_clean, lines_att = _lines(clean_path), _lines(adv_path)
        n = num if num is not None else len(lines_clean)
        before = after = 0
        for i in range(n):
            a, b = parse_line(lines_clean[i])
            if a == b:
                before += 1
                c, d = parse_line(lines_att[i])
                if c == d:
                    after += 1
        ar = after / before * 100
        print('Clean Acc: {}, Adversarial Robustness: {}'.format(before / n * 100, ar))
        return ar


class WorstCaseAdvRobustEvaluator(object):
    parse_line = staticmethod(parse_line)

    def eval(self, clean_path, multi_adv_result_paths, num=None):
        lines_clean = _lines(clean_path)
        atts = [_lines(p) for p in multi_adv_result_paths]
        n = num if num is not None else len(lines_clean)
        before = after = 0
        for i in range(n):
            a, b = parse_line(lines_clean[i])
            if a == b:
                before += 1
                ok = 1
                for la in atts:
                    c, d = parse_line(la[i])
                    if c != d:
                        ok = 0
                after += ok
        wcar = after / before * 100
        print('Worst-Case Adversarial Robustness: {}'.format(wcar))
        return wcar


def transfer_rate(src_clean_path, tgt_clean_path, transfer_path):
    """parse_transfer.py:33-42: among samples both the source and the target model classify correctly, the fraction
    the transferred adversarial examples make the TARGET model misclassify."""
    ls, lt, lx = _lines(src_clean_path), _lines(tgt_clean_path), _lines(transfer_path)
    if not (len(ls) == len(lt) == len(lx)):
        raise ValueError('transfer_rate: result files differ in length')
    before = after = 0
    for i in range(len(ls)):
        a, b = parse_line(ls[i])
        c, d = parse_line(lt[i])
        if a == b and c == d:
            before += 1
            e, f = parse_line(lx[i])
            if e != f:
                after += 1
    return after / before


def _load_confidence(res_file):
    """(confidence fp64 [n], correct fp64 [n], num_correct) of a ConfidenceWriter file, read as imageneto_evaluator.py:36-42 reads
    it: the `confidence` and `correct` lists of the lines concatenated, `num_correct` summed."""
    confidence, correct, num_correct = [], [], 0
    for line in _lines(res_file):
        obj = json.loads(line)
        confidence += obj['confidence']
        correct += obj['correct']
        num_correct += obj['num_correct']
    return np.array(confidence, dtype=np.float64), np.array(correct, dtype=np.float64), num_correct


class _MeanOfValues(object):
    """get_mean as ImageNetSEvaluator carries it: the reference iterates `for key, item in dict`, which unpacks the KEYS; here the
    mean runs over the values."""

    def get_mean(self):
        mean = float(np.mean([v for v in self.metric.metric.values() if v is not None]))
        return {'Mean': mean}

    def clear(self):
        self.metric.metric = {}


class ImageNetAEvaluator(_MeanOfValues):
    """ImageNet-A: {'top1', 'RMS_calib_error', 'AURRA'}, all in percent (calibration_tools.py:123-130 logs the last two as
    100 * calib_err(p='2') and 100 * aurra).  beta is calib_err's bin size.  A file of fewer than beta samples has no bin, hence no
    calibration error (calib_err raises ValueError, the reference IndexError): 'RMS_calib_error' is then None, and the other two
    numbers are still reported -- ImageNet-A itself has 7500 samples."""

    def __init__(self, beta=100):
        self.metric = Metric()
        self.beta = int(beta)

    def eval(self, res_file):
        confidence, correct, _ = _load_confidence(res_file)
        if len(confidence) == 0:
            raise ValueError('ImageNetAEvaluator: %s holds no samples' % res_file)
        result_dict = {'top1': 100 * float(np.mean(correct)),
                       'RMS_calib_error': (100 * calibration.calib_err(confidence, correct, p='2', beta=self.beta)
                                           if len(confidence) >= self.beta else None),
                       'AURRA': 100 * calibration.aurra(confidence, correct)}
        self.metric.update(result_dict)
        return result_dict


class ImageNetOEvaluator(_MeanOfValues):
    """imageneto_evaluator.py:27-63: the anomaly score of a sample is minus its confidence, the out-of-distribution samples are
    the positive class, and the reported number is 100 * AUPR.  AUROC and FPR95 of the same call stay on `last_measures`."""

    def __init__(self):
        self.metric = Metric()
        self.last_measures = None

    def eval(self, res_file_in=None, res_file_out=None):
        assert res_file_in is not None and res_file_out is not None
        confidence_in, _, _ = _load_confidence(res_file_in)
        confidence_out, _, _ = _load_confidence(res_file_out)
        in_score = -confidence_in
        out_score = -confidence_out
        auroc, aupr, fpr = calibration.get_measures(out_score, in_score)
        self.last_measures = {'AUROC': 100 * auroc, 'AUPR': 100 * aupr, 'FPR95': 100 * fpr}
        result_dict = {'AUPR': 100 * aupr}
        self.metric.update(result_dict)
        return result_dict

    def get_mean(self):
        out = super().get_mean()
        self.metric.update(out)               # imageneto_evaluator.py:73-74
        self.metric.set_cmp_key('Mean')
        return out


class ImageNetPEvaluator(_MeanOfValues):
    """imagenetp_evaluator.py:27-44: the flip rate of a perturbation -- per sequence the share of frames whose prediction differs
    from the previous frame's (from the FIRST frame's when 'noise' is in the perturbation's name), averaged over the sequences.
    Reads lines {"predictions": [...]}, one per sequence.  Only the evaluator is mirrored: decoding the sequences is out of scope."""

    def __init__(self):
        self.metric = Metric()

    def load_res(self, res_file):
        return [np.array(json.loads(line)['predictions']) for line in _lines(res_file)]

    def eval(self, res_file, perturbation=None):
        predictions = self.load_res(res_file)
        noise_perturbation = 'noise' in perturbation
        result = 0
        for vid_preds in predictions:
            result_for_vid = []
            prev_pred = vid_preds[0]
            for pred in vid_preds[1:]:
                result_for_vid.append(int(prev_pred != pred))
                if not noise_perturbation:
                    prev_pred = pred
            result += np.mean(result_for_vid) / len(predictions)
        result_dict = {perturbation: float(result)}
        self.metric.update(result_dict)
        return result_dict
