"""JSON-lines result files, one process per GPU.

Layout (exprs/nips_benchmark/batch_eval_transfer/parse_transfer.py:27-31, batch_eval_adv/eval.sh): a run writes
`<root>/<model>/<noise>_<eps>/results.txt.all` (clean: `none_0`; transfer: `<src>_To_<tgt>/<attack>_<eps>/...`).
Every rank appends its shard to `results.txt.rank<r>` as {"prediction": p, "label": y, "score": [...], "index": i};
rank 0 merges the shards ordered by the global sample index, so the file is identical for every world size.

ConfidenceWriter (the ImageNet-A / ImageNet-O evaluation) keeps the sharding and the merge and writes, per SAMPLE,
{"confidence": [c], "correct": [b], "num_correct": b, "prediction": p, "label": y, "index": i}: the key set the reference's
ImageNetOEvaluator reads (imageneto_evaluator.py:36-50 concatenates the `confidence` / `correct` lists of the lines and sums
`num_correct`, so it reads this file unchanged), one sample per line so that the file is the same for every batch size too.

RankWriter (the ImageNet-C loop) keeps the sharding and the merge too and writes {"prediction": p, "label": y, "rank": r, "index": i}:
the label's rank in the stable descending order of the scores instead of the scores, a few bytes per sample where a `score` line
of a 1000-class model is some 20 KB.  ImageNetCEvaluator reads either form.
"""
import json
import os


def result_dir(root, model_name, noise='none', eps='0', tgt_name=None):
    top = model_name if tgt_name is None else '%s_To_%s' % (model_name, tgt_name)
    return os.path.join(root, top, '%s_%s' % (noise, eps))


class ResultWriter(object):
    def __init__(self, save_dir, rank=0, world=1, with_score=True):
        self.dir, self.rank, self.world, self.with_score = save_dir, rank, world, with_score
        os.makedirs(save_dir, exist_ok=True)
        self.path = os.path.join(save_dir, 'results.txt.rank%d' % rank)
        self.f = open(self.path, 'w')

    def write_batch(self, logits, labels, indices):
        """logits: (b, classes) tensor on any device; labels: (b,) tensor; indices: global sample indices."""
        pred = logits.argmax(dim=1).tolist()
        lab = labels.tolist()
        sc = logits.float().cpu().tolist() if self.with_score else None
        for j in range(len(lab)):
            rec = {'prediction': int(pred[j]), 'label': int(lab[j])}
            if sc is not None:
                rec['score'] = sc[j]
            rec['index'] = int(indices[j])
            self.f.write(json.dumps(rec) + '\n')

    def close(self, barrier=None):
        """Flush this rank's shard; after `barrier()` rank 0 merges all shards into results.txt.all."""
        self.f.close()
        if barrier is not None:
            barrier()
        out = os.path.join(self.dir, 'results.txt.all')
        if self.rank == 0:
            recs = []
            for r in range(self.world):
                with open(os.path.join(self.dir, 'results.txt.rank%d' % r)) as f:
                    recs.extend(json.loads(ln) for ln in f)
            recs.sort(key=lambda x: x['index'])
            with open(out, 'w') as f:
                for rec in recs:
                    f.write(json.dumps(rec) + '\n')
        return out


class ConfidenceWriter(ResultWriter):
    """Result files of the subset evaluation (metrics/confidence.py): same shards, same merge by global index as ResultWriter."""

    def __init__(self, save_dir, rank=0, world=1):
        super().__init__(save_dir, rank, world, with_score=False)

    def write_batch(self, pred, conf, correct, labels, indices):
        """pred int32 / conf fp32 / correct uint8: the three outputs of subset_confidence, [b] on any device -- 9 bytes per sample
        cross to the host, not the score vectors.  labels: (b,) tensor or sequence in subset coordinates, None for a set without
        labels (written as -1).  indices: global sample indices.  The confidence is written as the double that equals the fp32
        value, so reading the file back loses nothing."""
        pred, conf, correct = pred.tolist(), conf.tolist(), correct.tolist()
        lab = [-1] * len(pred) if labels is None else (labels.tolist() if hasattr(labels, 'tolist') else list(labels))
        for j in range(len(pred)):
            b = int(correct[j])
            self.f.write(json.dumps({'confidence': [conf[j]], 'correct': [b], 'num_correct': b, 'prediction': int(pred[j]),
                                     'label': int(lab[j]), 'index': int(indices[j])}) + '\n')


class RankWriter(ResultWriter):
    """Compact result files of the ImageNet-C loop (metrics/confidence.py: topk_score): same shards, same merge by global index as
    ResultWriter."""

    def __init__(self, save_dir, rank=0, world=1):
        super().__init__(save_dir, rank, world, with_score=False)

    def write_batch(self, pred, rank, labels, indices):
        """pred / rank int32: the two outputs of topk_score, [b] on any device -- 8 bytes per sample cross to the host.  labels: (b,)
        tensor or sequence.  indices: global sample indices."""
        pred, rank = pred.tolist(), rank.tolist()
        lab = labels.tolist() if hasattr(labels, 'tolist') else list(labels)
        for j in range(len(pred)):
            self.f.write(json.dumps({'prediction': int(pred[j]), 'label': int(lab[j]), 'rank': int(rank[j]),
                                     'index': int(indices[j])}) + '\n')
