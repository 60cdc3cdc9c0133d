"""Result writer and robustness metrics: the step immediately after the hot path.

Mirrors RobustART/metrics/ (names, arguments, printed quantities):
    ImageNetCEvaluator   RobustART/metrics/imagenetc_evaluator.py:26-75    top-k from `score` / `label` lines
    ImageNetSEvaluator   RobustART/metrics/imagenets_evaluator.py:9-66     per (decoder, resize) top-1, mean / std
    AdvRobustEvaluator   RobustART/metrics/AR_evaluator.py:9-39            AR = survived / clean-correct * 100
    WorstCaseAdvRobustEvaluator  RobustART/metrics/WCAR_evaluator.py:9-44  WCAR = survived ALL attacks / clean-correct
    transfer_rate        exprs/nips_benchmark/batch_eval_transfer/parse_transfer.py:10-46
    ImageNetAEvaluator   RobustART/metrics/calibration_tools.py:123-130    top-1, RMS calibration error, AURRA from `confidence` /
                                                                           `correct` lines (the reference's class of this name is broken)
    ImageNetOEvaluator   RobustART/metrics/imageneto_evaluator.py:27-63    AUPR of out- vs in-distribution confidences
    ImageNetPEvaluator   RobustART/metrics/imagenetp_evaluator.py:27-44    flip rate over `predictions` sequences
    calib_err, aurra, fpr_at_recall, get_measures   RobustART/metrics/calibration_tools.py:26-63,138-191, numpy fp64, no sklearn
    class_subset, subset_confidence   prediction / confidence / correctness over a class subset on the GPU (metrics/confidence.py,
                                      rart_logit_confidence_f32); ConfidenceWriter writes them, 9 bytes per sample off the device
    topk_score           prediction, label rank and device-resident top-k counters of the ImageNet-C loop (rart_topk_score_f32);
                         RankWriter writes `rank` lines, 8 bytes per sample off the device, which ImageNetCEvaluator reads as well
and writes the JSON-lines `results.txt.all` files they read (one line per sample, `prediction` first, `label`
second: AR/WCAR/transfer parse the first two values of a line).

Departures from the reference as written (each one is a defect there):
  * AR / WCAR define `parse_line(line)` without `self` and call it as a method, so `eval` raises TypeError; here it
    is a staticmethod with the same parsing;
  * the sample count is hard-coded to 50000 there; here it is the length of the clean file (`num=` overrides);
  * ImageNetSEvaluator keys its result dict with a list (unhashable) and iterates `for key, item in dict`; here the
    key is the tuple (decoder_type, resize_type) and mean / std run over the values;
  * imageneta_evaluator.py is a line-for-line copy of the ImageNet-P evaluator that keys a dict with a list (TypeError) and computes
    nothing about ImageNet-A; here ImageNetAEvaluator reports what show_calibration_results logs.  The `get_mean` of the
    ImageNet-A / -O / -P evaluators has the same `for key, item in dict` defect and the same fix;
  * calibration_tools.py imports sklearn and a `prototype` logger that is not in the tree; calibration.py needs neither.  calib_err
    is mirrored as written, leaving out its last bin; fewer samples than beta is a ValueError (IndexError there).
Not mirrored: tune_temp, soft_f1, the decoding of ImageNet-P's sequences.
"""
from .calibration import aurra, calib_err, fpr_at_recall, get_measures                 # noqa: F401
from .confidence import class_subset, subset_confidence, topk_score                   # noqa: F401
from .evaluators import (AdvRobustEvaluator, ImageNetAEvaluator, ImageNetCEvaluator,   # noqa: F401
                         ImageNetOEvaluator, ImageNetPEvaluator, ImageNetSEvaluator,
                         WorstCaseAdvRobustEvaluator, parse_line, transfer_rate)
from .writer import ConfidenceWriter, RankWriter, ResultWriter, result_dir            # noqa: F401
