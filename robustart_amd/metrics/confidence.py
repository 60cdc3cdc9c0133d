"""Prediction, confidence and correctness over a class subset, on the GPU next to the engine that produced the logits.

ImageNet-A and ImageNet-O score a 1000-class model on 200 of its classes (imagenet-a_o-loop): per sample the evaluation needs the
prediction inside the subset, the largest soft-max probability over the subset and whether the prediction is right.
rart_logit_confidence_f32 (csrc/logit_confidence.hip) computes the three in one launch, so 9 bytes per sample reach the host instead
of the score vector.

The ImageNet-C loop scores the same model on all classes once per (corruption, severity): topk_score (rart_topk_score_f32,
csrc/topk_score.hip) gives the prediction and the label's rank per sample and adds the top-k hits to counters that stay on the device.
"""
import ctypes

import torch


def class_subset(indices, classes, device):
    """Validate a class subset on the host and upload it once -> int32 tensor on `device`.  The indices must be ints, strictly
    increasing and in [0, classes): the kernel does not range-check them (they index a row of logits), so this is where they are
    checked.  Strictly increasing is what an image-folder dataset produces (sorted class folders), and it makes the subset coordinate
    of a class its rank."""
    idx = list(indices)
    classes = int(classes)
    prev = -1
    for k, v in enumerate(idx):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError('class_subset: entry %d is %r, not an int' % (k, v))
        if v < 0 or v >= classes:
            raise ValueError('class_subset: entry %d is %d, outside [0, %d)' % (k, v, classes))
        if v <= prev:
            raise ValueError('class_subset: entry %d is %d after %d: the indices must be strictly increasing' % (k, v, prev))
        prev = v
    return torch.tensor(idx, dtype=torch.int32).to(device)


def subset_confidence(logits, subset=None, labels=None):
    """(pred int32 [b], conf fp32 [b], correct uint8 [b]) of fp32 CUDA logits [b, classes], which may be a row-strided view (unit
    stride along the classes).  subset: a tensor from class_subset (None: all classes).  labels: int64 CUDA tensor [b] in subset
    coordinates (None: correct is 0 everywhere, the out-of-distribution set).  The definition is rart_logit_confidence_f32's
    (include/robustart_hip.h).  No device-to-host read and no allocation beyond the three outputs; there is no CPU path."""
    from .. import _lib
    if not isinstance(logits, torch.Tensor) or logits.device.type != 'cuda':
        raise RuntimeError('subset_confidence: logits must be a CUDA tensor (the row reduction is a HIP kernel; there is no CPU fallback)')
    if logits.dtype != torch.float32 or logits.dim() != 2:
        raise ValueError('subset_confidence: logits must be fp32 [rows, classes], got %s %s' % (logits.dtype, tuple(logits.shape)))
    rows, classes = logits.shape
    if classes < 1:
        raise ValueError('subset_confidence: logits have no classes')
    if classes > 1 and logits.stride(1) != 1:
        raise ValueError('subset_confidence: the classes of a row must be contiguous (stride %d)' % logits.stride(1))
    ld = logits.stride(0) if rows > 1 else classes
    if ld < classes:
        raise ValueError('subset_confidence: row stride %d is shorter than the %d classes' % (ld, classes))
    n_sub = 0
    if subset is not None:
        if subset.dtype != torch.int32 or subset.dim() != 1 or subset.device != logits.device or not subset.is_contiguous():
            raise ValueError('subset_confidence: subset must be a contiguous int32 vector on the logits\' device (class_subset)')
        n_sub = subset.numel()
        if n_sub > classes:
            raise ValueError('subset_confidence: a subset of %d of %d classes' % (n_sub, classes))
    if labels is not None:
        if labels.dtype != torch.int64 or labels.shape != (rows,) or labels.device != logits.device or not labels.is_contiguous():
            raise ValueError('subset_confidence: labels must be a contiguous int64 vector [rows] on the logits\' device')
    dev = logits.device
    pred = torch.empty(rows, dtype=torch.int32, device=dev)
    conf = torch.empty(rows, dtype=torch.float32, device=dev)
    correct = torch.empty(rows, dtype=torch.uint8, device=dev)
    lib = _lib.load()
    with torch.cuda.device(dev):
        _lib.check(lib.rart_logit_confidence_f32(logits.data_ptr(), rows, classes, ld, _lib.ptr(subset if n_sub else None), n_sub,
                                                 _lib.ptr(labels), pred.data_ptr(), conf.data_ptr(), correct.data_ptr(),
                                                 _lib.stream_ptr()))
    return pred, conf, correct


def topk_score(logits, labels, ks=(1, 5), hits=None, pred=True, rank=True):
    """(pred int32 [b] or None, rank int32 [b] or None) of fp32 CUDA logits [b, classes], which may be a row-strided view (unit stride
    along the classes), and int64 CUDA labels [b].  rank is the label's position in a stable descending sort of the row (ties to the
    lower class index; `classes` for a label outside [0, classes) or a NaN at the label), pred the lowest index of the maximum: the
    definition is rart_topk_score_f32's (include/robustart_hip.h).  hits: None, or a contiguous int64 CUDA vector of at least
    len(ks) entries to which the number of rows with rank < ks[i] is ADDED (never cleared: pass counters[2 * slot:] to keep one pair
    per slot).  pred / rank False skips that output.  No device-to-host read and no allocation beyond the outputs asked for; there is
    no CPU path."""
    from .. import _lib
    if not isinstance(logits, torch.Tensor) or logits.device.type != 'cuda':
        raise RuntimeError('topk_score: logits must be a CUDA tensor (the row reduction is a HIP kernel; there is no CPU fallback)')
    if logits.dtype != torch.float32 or logits.dim() != 2:
        raise ValueError('topk_score: logits must be fp32 [rows, classes], got %s %s' % (logits.dtype, tuple(logits.shape)))
    rows, classes = logits.shape
    if classes < 1:
        raise ValueError('topk_score: logits have no classes')
    if classes > 1 and logits.stride(1) != 1:
        raise ValueError('topk_score: the classes of a row must be contiguous (stride %d)' % logits.stride(1))
    ld = logits.stride(0) if rows > 1 else classes
    if ld < classes:
        raise ValueError('topk_score: row stride %d is shorter than the %d classes' % (ld, classes))
    if not isinstance(labels, torch.Tensor) or labels.dtype != torch.int64 or labels.shape != (rows,) or labels.device != logits.device \
            or not labels.is_contiguous():
        raise ValueError('topk_score: labels must be a contiguous int64 vector [rows] on the logits\' device')
    ks = [int(k) for k in ks]
    if len(ks) > 8 or any(k < 1 for k in ks):
        raise ValueError('topk_score: at most 8 values of k, each at least 1, got %r' % (ks,))
    if hits is not None:
        if not isinstance(hits, torch.Tensor) or hits.dtype != torch.int64 or hits.dim() != 1 or hits.device != logits.device \
                or not hits.is_contiguous() or hits.numel() < len(ks):
            raise ValueError('topk_score: hits must be a contiguous int64 vector of at least %d entries on the logits\' device' % len(ks))
    dev = logits.device
    p = torch.empty(rows, dtype=torch.int32, device=dev) if pred else None
    r = torch.empty(rows, dtype=torch.int32, device=dev) if rank else None
    lib = _lib.load()
    with torch.cuda.device(dev):
        _lib.check(lib.rart_topk_score_f32(logits.data_ptr(), rows, classes, ld, _lib.ptr(labels), _lib.ptr(p), _lib.ptr(r),
                                           (ctypes.c_int * max(len(ks), 1))(*ks), len(ks) if hits is not None else 0, _lib.ptr(hits),
                                           _lib.stream_ptr()))
    return p, r
