"""The definition of rart_logit_confidence_f32 (include/robustart_hip.h) in numpy fp64, and the yardstick its confidence is measured
with: the error of torch's own fp32 CPU soft-max on the same rows.  Shared by the kernel test and the end-to-end evaluation test."""
import numpy as np
import torch


def reference(z32):
    """the definition, in fp64, on the K selected logits of each row in subset order"""
    z = z32.astype(np.float64)
    pred = np.argmax(z, axis=1)                            # the lowest position of the maximum; the first NaN if there is one
    m = z[np.arange(len(z)), pred]
    with np.errstate(invalid='ignore', over='ignore'):
        conf = 1.0 / np.exp(z - m[:, None]).sum(axis=1)    # inf - inf and -inf - -inf are NaN, a NaN maximum makes every term NaN
    return pred.astype(np.int32), conf


def torch_fp32_error(z32, conf64):
    """relative error per row of torch's fp32 CPU softmax(z).max() against the fp64 reference (NaN rows: 0)"""
    got = torch.softmax(torch.from_numpy(np.ascontiguousarray(z32)), 1).max(1).values.double().numpy()
    ok = np.isfinite(conf64)
    err = np.zeros(len(conf64))
    err[ok] = np.abs(got[ok] - conf64[ok]) / conf64[ok]
    return err


def conf_bound(ref_err):
    """4 x the worst relative error of torch's fp32 soft-max on these rows (another order of summation), floored at 1e-6 (about 16
    fp32 ulp: ten tree levels for 1000 terms, plus expf and the division)"""
    return max(1e-6, 4.0 * float(np.max(ref_err))) if len(ref_err) else 1e-6
