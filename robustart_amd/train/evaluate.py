"""The evaluation loops of cls_solver -- clean / corrupted / attacked, ImageNet-A/O, ImageNet-S and ImageNet-C -- on one scaffold
(EvalRun: the model, its HIP engine, logits of a uint8 batch, the result-path names, the barrier, this rank's batches)."""
import json
import os
import time

import torch
import torch.distributed as dist

from .checkpoint import build_model
from .data import IMAGENET_MEAN, IMAGENET_STD, FileImageNet, make_dataset, read_transforms, shard_indices, synthetic_size


def parse_eps(s):
    """'8/255' or '0.031' -> float (the launchers pass fractions, batch_eval_adv/eval.sh:9-10)."""
    if isinstance(s, (int, float)):
        return float(s)
    if '/' in s:
        a, b = s.split('/')
        return float(a) / float(b)
    return float(s)


def topk_correct(logits, labels, ks=(1, 5)):
    _, pred = logits.topk(max(ks), dim=1)
    hit = pred.eq(labels.view(-1, 1))
    return [int(hit[:, :k].any(1).sum()) for k in ks]


def all_reduce_counters(values, device):
    """The eval path's only collective: sum of a few int64 counters."""
    t = torch.tensor(values, dtype=torch.int64, device=device)
    if dist_up():
        dist.all_reduce(t)
    return [int(v) for v in t.tolist()]


def dist_up():                                                   # is the process group up?
    return dist.is_available() and dist.is_initialized()


class EvalRun:
    """What every evaluation loop needs, built once per evaluate* call after the loop's own checks: the model on the device in eval mode; on the HIP
    path its engine `f_model` at --precision / `engine_precision` (bf16, or 'fp32x': logits within 1e-4 of the fp32 network at ~3x the MFMA work)."""

    def __init__(self, cfg, args, device, model=None):
        self.cfg, self.args, self.device = cfg, args, device
        self.model = (model or build_model(cfg, args)).to(device).eval()
        self.use_hip = device.type == 'cuda' and args.engine == 'hip'
        self.f_model = None
        if self.use_hip:
            from ..model.engine import EngineModel
            self.f_model = EngineModel(self.model, takes_normalized=False, precision=getattr(args, 'precision', None) or cfg.get('engine_precision', 'bf16'))
        self.mean = torch.tensor(IMAGENET_MEAN, device=device).view(1, 3, 1, 1)
        self.std = torch.tensor(IMAGENET_STD, device=device).view(1, 3, 1, 1)
        self.save_dir = getattr(args, 'save_dir', None)
        self.barrier = dist.barrier if dist_up() else None

    @property
    def name(self):
        return getattr(self.args, 'src_name', None) or self.cfg['model']['type']

    def logits_u8(self, x):
        """uint8 NHWC batch -> logits: the engine's u8 entry (normalisation in its input kernel) or the torch module under no_grad"""
        if self.use_hip:
            return self.f_model.rart_engine.logits_from_u8(x, IMAGENET_MEAN, IMAGENET_STD)
        with torch.no_grad():
            return self.model((x.permute(0, 3, 1, 2).float() / 255.0 - self.mean) / self.std)

    def batches(self, ds, rank, world):
        """this rank's contiguous share of `ds`, one index list per batch"""
        idx, bs = shard_indices(len(ds), rank, world), int(self.cfg.get('data', {}).get('batch_size', 64))
        return (idx[s:s + bs] for s in range(0, len(idx), bs))


def natural_mode(dcfg):
    """`data.test.imagenet_a&o: True` (exp/imagenet-a_o-loop/config_vit_base.yaml:79-84): the ImageNet-A / ImageNet-O evaluation."""
    return bool(((dcfg or {}).get('test') or {}).get('imagenet_a&o', False))


def read_class_map(tcfg, num_classes):
    """The model's class index -> wnid: the lines of `data.test.class_index_file` (one wnid per line, the line number is the class
    index) or, without that key, the sorted sub-directory names of `imagenet_val_root_dir` (the order an image-folder training set
    gives its classes).  The count must equal the model's num_classes."""
    path = tcfg.get('class_index_file')
    if path:
        with open(path) as f:
            names = [ln.strip() for ln in f if ln.strip()]
        src = 'data.test.class_index_file %s' % path
    else:
        root = tcfg.get('imagenet_val_root_dir')
        if not root or not os.path.isdir(root):
            raise ValueError('data.test: imagenet_a&o needs class_index_file or a directory imagenet_val_root_dir with one folder per '
                             'class, got %r' % (root,))
        names = sorted(d for d in os.listdir(root) if os.path.isdir(os.path.join(root, d)))
        src = 'data.test.imagenet_val_root_dir %s' % root
    if len(names) != int(num_classes):
        raise ValueError('%s names %d classes, the model has num_classes = %d' % (src, len(names), int(num_classes)))
    if len(set(names)) != len(names):
        raise ValueError('%s names a class twice' % src)
    return names


def subset_of(folder_names, class_map, what):
    """class indices of a folder set's class names, in folder order -> list of ints; a name the map lacks is a ValueError"""
    pos = {w: i for i, w in enumerate(class_map)}
    for w in folder_names:
        if w not in pos:
            raise ValueError('%s: class folder %r is not in the class map' % (what, w))
    return [pos[w] for w in folder_names]


def natural_datasets(cfg):
    """The config side of the ImageNet-A / -O evaluation, all of it on the host: the class map, the three folder sets and the two
    class subsets -> {'a': (dataset, indices), 'o_in': (dataset, indices), 'o_out': (dataset, indices)}."""
    dcfg = cfg.get('data', {})
    tcfg = dcfg.get('test') or {}
    num_classes = int(((cfg.get('model') or {}).get('kwargs') or {}).get('num_classes', 1000))
    class_map = read_class_map(tcfg, num_classes)
    t = read_transforms(dcfg, 'test')
    size = int(dcfg.get('input_size', 224))
    sets = {}
    for key, name in (('a', 'imagenet_a_root_dir'), ('o_out', 'imagenet_o_root_dir'), ('o_in', 'imagenet_o_folder')):
        if not tcfg.get(name):
            raise ValueError('data.test: imagenet_a&o needs data.test.%s' % name)
        sets[key] = FileImageNet.from_folder(tcfg[name], size, t['test_resize'], t['type'], (tcfg.get('image_reader') or {}).get('type', 'pil'),
                                             dcfg.get('limit_samples'), int(dcfg.get('seed', 0)), num_workers=int(dcfg.get('num_workers') or 8),
                                             entropy=(tcfg.get('image_reader') or {}).get('entropy', 'host'))
    if sets['o_in'].classes != sets['o_out'].classes:
        raise ValueError('data.test.imagenet_o_folder must hold exactly the class folders of imagenet_o_root_dir: %d vs %d folders, '
                         'differing in %s' % (len(sets['o_in'].classes), len(sets['o_out'].classes),
                                              sorted(set(sets['o_in'].classes) ^ set(sets['o_out'].classes))[:5]))
    sub_a = subset_of(sets['a'].classes, class_map, 'data.test.imagenet_a_root_dir')
    sub_o = subset_of(sets['o_out'].classes, class_map, 'data.test.imagenet_o_root_dir')
    for sub, name in ((sub_a, 'imagenet_a_root_dir'), (sub_o, 'imagenet_o_root_dir')):
        if sub != sorted(sub):
            # the label of a folder sample is the folder's position, the prediction the class's rank in the subset: they are the same
            # coordinate only when the class map orders the folders as their names do
            raise ValueError('data.test.%s: the class map does not keep the order of the class folders\' names' % name)
    return {'a': (sets['a'], sub_a), 'o_in': (sets['o_in'], sub_o), 'o_out': (sets['o_out'], sub_o)}


def evaluate_natural(cfg, args, rank, world, device, model=None):
    """`data.test.imagenet_a&o`: three passes over sharded indices -- ImageNet-A, the in-distribution set of ImageNet-O's classes, and
    ImageNet-O (out of distribution, no labels).  Per batch: engine logits -> rart_logit_confidence_f32 over the set's class subset ->
    ConfidenceWriter.  After the barrier rank 0 computes the metrics from the merged files, as the reference does."""
    if not getattr(args, 'save_dir', None):
        raise ValueError('data.test.imagenet_a&o needs --save-dir: the metrics are computed from the merged result files')
    if (getattr(args, 'attack', None) and args.attack != 'none') or getattr(args, 'corruption', None):
        raise ValueError('data.test.imagenet_a&o cannot be combined with --attack / --corruption: no config of imagenet-a_o-loop has noise')
    plan = natural_datasets(cfg)
    if device.type != 'cuda':
        raise RuntimeError('data.test.imagenet_a&o runs on the GPU (the resize and the subset confidence are HIP kernels; no CPU fallback)')
    from ..metrics import (ConfidenceWriter, ImageNetAEvaluator, ImageNetOEvaluator, class_subset, result_dir, subset_confidence)
    run = EvalRun(cfg, args, device, model)
    num_classes = int(((cfg.get('model') or {}).get('kwargs') or {}).get('num_classes', 1000))
    t0 = time.time()
    paths, counts, subsets = {}, {}, {}
    for key, noise_name, labelled in (('a', 'imagenet_a', True), ('o_in', 'imagenet_o_in', True), ('o_out', 'imagenet_o_out', False)):
        ds, sub = plan[key]
        if tuple(sub) not in subsets:
            subsets[tuple(sub)] = class_subset(sub, num_classes, device)         # validated on the host, uploaded once
        sub_dev = subsets[tuple(sub)]
        writer = ConfidenceWriter(result_dir(run.save_dir, run.name, noise_name, '0'), rank, world)
        for items in run.batches(ds, rank, world):
            imgs, labels = ds.batch(items, device)
            logits = run.logits_u8(imgs)
            if logits.shape[1] != num_classes:
                raise ValueError('the model returns %d logits, model.kwargs.num_classes says %d' % (logits.shape[1], num_classes))
            pred, conf, correct = subset_confidence(logits.float(), sub_dev, labels if labelled else None)
            writer.write_batch(pred, conf, correct, [ds.items[i][1] for i in items] if labelled else None, items)
        paths[key] = writer.close(barrier=run.barrier)
        counts[key] = len(ds)
    res = None
    if rank == 0:
        ev_a, ev_o = ImageNetAEvaluator(), ImageNetOEvaluator()
        a = ev_a.eval(paths['a'])
        o = ev_o.eval(paths['o_in'], paths['o_out'])
        res = {'imagenet_a': dict(a, count=counts['a']),
               'imagenet_o': {'AUPR': o['AUPR'], 'AUROC': ev_o.last_measures['AUROC'], 'FPR95': ev_o.last_measures['FPR95'],
                              'count_in': counts['o_in'], 'count_out': counts['o_out']},
               'world_size': world, 'seconds': time.time() - t0}
        print(json.dumps(res))
    return res


def imagenet_s_ops(spec=None):
    """`--imagenet-s-ops a,b,...` -> the resize operators of the ImageNet-S loop, in order; None / '' -> the eleven names of
    PIL_FILTERS then CV_MODES.  An unknown or repeated name is a ValueError."""
    from ..noise.imagenet_s import CV_MODES, PIL_FILTERS
    known = list(PIL_FILTERS) + list(CV_MODES)
    if spec is None or not str(spec).strip():
        return known
    ops = [t.strip() for t in str(spec).split(',') if t.strip()]
    for t in ops:
        if t not in known:
            raise ValueError('--imagenet-s-ops: unknown resize operator %r (%s)' % (t, ', '.join(known)))
    if len(set(ops)) != len(ops) or not ops:
        raise ValueError('--imagenet-s-ops: every operator once, got %r' % (spec,))
    return ops


def evaluate_imagenet_s(cfg, args, rank, world, device, model=None):
    """`--evaluate --imagenet-s`: the loop of exp/imagenet_s_loop (eval.sh:23, multi_eval_decoder_resize_solver): one model scored on
    the test set once per (decoder, resize operator) pair; the accuracies, their mean and their spread.  Per batch of sharded
    indices the files are decoded ONCE (data.test.image_reader.type pil | hip) and every operator runs on the decoded batch through
    image_transfer_batch(transform_type='val', resize=data.input_size): the operator under test replaces the config's Resize, so
    only input_size is taken from the transform list (which still has to parse).  The decoder is 'pil' (the others are not in this
    build).  `data.test.save_acc_var_neg` (with --save-dir) also writes <save_dir>/<model>/imagenet_s_summary.json; the reference
    solver that defines this key is absent from the reference tree, so the summary's form is unpinned."""
    ops = imagenet_s_ops(getattr(args, 'imagenet_s_ops', None))
    dcfg = cfg.get('data', {})
    if (getattr(args, 'attack', None) and args.attack != 'none') or getattr(args, 'corruption', None) or natural_mode(dcfg):
        raise ValueError('--imagenet-s cannot be combined with --attack, --corruption or data.test.imagenet_a&o: no config of '
                         'imagenet_s_loop has another noise')
    if device.type != 'cuda':
        raise RuntimeError('--imagenet-s runs on the GPU (the resize operators are HIP kernels; no CPU fallback)')
    from ..metrics import ImageNetSEvaluator, ResultWriter, result_dir
    from ..noise import imagenet_s as NS
    size = int(dcfg.get('input_size', 224))
    ds = make_dataset(dcfg, synthetic_size(dcfg), size, 'test')    # parses the transforms
    if not isinstance(ds, FileImageNet):
        raise ValueError('--imagenet-s needs data.read_from: fs (the loop is about decoding and resizing files)')
    run = EvalRun(cfg, args, device, model)
    name, save_dir = run.name, run.save_dir
    writers = {op: ResultWriter(result_dir(save_dir, name, 'imagenet_s', 'pil_%s' % op), rank, world) for op in ops} if save_dir else {}
    counters = {op: [0, 0] for op in ops}
    cnt = 0
    t0 = time.time()
    for items in run.batches(ds, rank, world):
        decoded = ds.decode_indices(items, device)                 # once per batch, whatever the number of operators
        labels = torch.tensor([ds.items[i][1] for i in items], dtype=torch.int64, device=device)
        cnt += len(items)
        for op in ops:
            imgs = NS.image_transfer_batch(None, 'pil', op, 'val', size, ds.num_workers, decoded=decoded)
            logits = run.logits_u8(imgs)
            a, b = topk_correct(logits.float(), labels)
            counters[op][0] += a
            counters[op][1] += b
            if writers:
                writers[op].write_batch(logits, labels, items)
    paths = {op: writers[op].close(barrier=run.barrier) for op in ops} if writers else {}
    flat = all_reduce_counters([v for op in ops for v in counters[op]] + [cnt], device)
    cnt = flat[-1]
    res = None
    if rank == 0:
        ev = ImageNetSEvaluator()
        for k, op in enumerate(ops):
            if paths:
                ev.eval(paths[op], 'pil', op)
            else:
                ev.metric.update({('pil', op): 100.0 * flat[2 * k] / max(cnt, 1)})
        acc = {'%s/%s' % k: v for k, v in ev.metric.metric.items()}
        res = {'imagenet_s': acc, 'Mean': ev.get_mean()['Mean'], 'Std.': ev.get_std()['Std.'], 'count': cnt, 'world_size': world,
               'seconds': time.time() - t0}
        if save_dir and bool((dcfg.get('test') or {}).get('save_acc_var_neg', False)):
            import numpy as np
            vals = list(acc.values())
            with open(os.path.join(save_dir, name, 'imagenet_s_summary.json'), 'w') as f:
                json.dump({'acc': acc, 'mean': res['Mean'], 'var': float(np.var(vals)), 'neg_std': -res['Std.']}, f)
        print(json.dumps(res))
    return res


def _once_each(spec, what):
    toks = [t.strip() for t in str(spec).split(',') if t.strip()]
    if not toks:
        raise ValueError('%s: an empty list' % what)
    if len(set(toks)) != len(toks):
        raise ValueError('%s: every entry once, got %r' % (what, spec))
    return toks


def imagenet_c_names(spec=None):
    """`--imagenet-c-names a,b,...` -> (corruption names in order, named explicitly?).  None: the 15 standard corruptions,
    CORRUPTION_NAMES[:15]; 'all': these and the four extras; both name frost only implicitly.  An unknown or repeated name or an empty
    list is a ValueError."""
    from ..noise.imagenet_c import CORRUPTION_NAMES
    if spec is None:
        return list(CORRUPTION_NAMES[:15]), False
    if str(spec).strip() == 'all':
        return list(CORRUPTION_NAMES), False
    names = _once_each(spec, '--imagenet-c-names')
    for t in names:
        if t not in CORRUPTION_NAMES:
            raise ValueError('--imagenet-c-names: unknown corruption %r (%s)' % (t, ', '.join(CORRUPTION_NAMES)))
    return names, True


def imagenet_c_severities(spec=None):
    """`--imagenet-c-severities 1,2,...` -> severities in order; None: 1..5.  Anything outside 1..5, a repeat or an empty list is a
    ValueError."""
    if spec is None:
        return [1, 2, 3, 4, 5]
    out = []
    for t in _once_each(spec, '--imagenet-c-severities'):
        if t not in ('1', '2', '3', '4', '5'):
            raise ValueError('--imagenet-c-severities: %r is not a severity (1..5)' % (t,))
        out.append(int(t))
    return out


def read_frost_textures(path):
    """The photographs of a folder as uint8 HxWx3 arrays, read with Pillow in sorted file order (the order decides which photograph
    a sample draws)."""
    import numpy as np
    from PIL import Image
    if not os.path.isdir(path):
        raise ValueError('the frost folder %r is not a directory' % (path,))
    out = []
    for fn in sorted(os.listdir(path)):
        p = os.path.join(path, fn)
        if os.path.isfile(p):
            with Image.open(p) as im:
                out.append(np.array(im.convert('RGB')))
    if not out:
        raise ValueError('the frost folder %r holds no photographs' % (path,))
    return out


def imagenet_c_plan(cfg, args):
    """Everything `--imagenet-c` decides from the arguments and the config alone, before a model, a dataset or the device is
    looked at -> {'names', 'severities', 'skipped', 'frost_dir'}.  Frost needs photographs (--imagenet-c-frost-dir, the key
    data.test.imagenet_c_frost_dir, or an earlier set_frost_textures): without them a frost that only the default list or 'all'
    names is left out and listed under 'skipped'; a frost named explicitly is a ValueError."""
    from ..noise import imagenet_c as C
    names, explicit = imagenet_c_names(getattr(args, 'imagenet_c_names', None))
    sevs = imagenet_c_severities(getattr(args, 'imagenet_c_severities', None))
    dcfg = cfg.get('data', {}) or {}
    if (getattr(args, 'attack', None) and args.attack != 'none') or getattr(args, 'corruption', None) or getattr(args, 'imagenet_s', False) \
            or natural_mode(dcfg):
        raise ValueError('--imagenet-c cannot be combined with --attack, --corruption, --imagenet-s or data.test.imagenet_a&o: the loop '
                         'applies every corruption itself and no config of imagenet_c_loop_mini has another noise')
    if getattr(args, 'imagenet_c_scores', False) and not getattr(args, 'save_dir', None):
        raise ValueError('--imagenet-c-scores writes the full result files: it needs --save-dir')
    frost_dir = getattr(args, 'imagenet_c_frost_dir', None) or (dcfg.get('test') or {}).get('imagenet_c_frost_dir')
    skipped = []
    if 'frost' in names and not frost_dir and not C._frost_textures:
        if explicit:
            raise ValueError('--imagenet-c-names names frost, which needs photographs: pass --imagenet-c-frost-dir (or '
                             'data.test.imagenet_c_frost_dir)')
        names = [t for t in names if t != 'frost']
        skipped = ['frost']
    return {'names': names, 'severities': sevs, 'skipped': skipped, 'frost_dir': frost_dir}


def evaluate_imagenet_c(cfg, args, rank, world, device, model=None):
    """`--evaluate --imagenet-c`: the loop of exp/imagenet_c_loop_mini: one model scored on every (corruption, severity) pair in one
    pass over the test set.  Per batch of sharded indices the dataset is read ONCE (any data.read_from); every pair corrupts that
    batch into one scratch buffer (the source batch is never written), the engine turns it into logits and rart_topk_score_f32 adds
    the top-1 / top-5 hits to the pair's two counters, which stay on the device: nothing is read on the host inside the loop, and
    one all_reduce and one read end it.  gaussian_noise and speckle_noise run all their severities in one noise_severities_ launch
    (bit-identical to the per-severity calls).  Seed and sample offset are those of a single `--corruption NAME --severity S` run,
    so a pair's inputs, logits and result directory <save_dir>/<model>/<corruption>_<severity>/ are that run's.  With --save-dir a
    pair's file holds RankWriter lines (prediction, label, rank: 8 bytes per sample off the device), or the full ResultWriter lines
    under --imagenet-c-scores; rank 0 evaluates every file with ImageNetCEvaluator.  Accuracies are percentages, as the evaluator's.
    The reference's multi_eval_solver, which defines this loop's summary, is absent from the reference tree: the form of the
    printed line ('imagenet_c' per pair, 'error' = mean top-1 error per corruption over the severities run, 'Mean' of those, 'skipped')
    is unpinned."""
    plan = imagenet_c_plan(cfg, args)
    if device.type != 'cuda':
        raise RuntimeError('--imagenet-c runs on the GPU (the corruptions and the scorer are HIP kernels; no CPU fallback)')
    from ..metrics import ImageNetCEvaluator, RankWriter, ResultWriter, result_dir, topk_score
    from ..noise import imagenet_c as C
    if plan['frost_dir'] and 'frost' in plan['names']:
        C.set_frost_textures(read_frost_textures(plan['frost_dir']))
    names, sevs = plan['names'], plan['severities']
    dcfg = cfg.get('data', {})
    ds = make_dataset(dcfg, synthetic_size(dcfg), int(dcfg.get('input_size', 224)), 'test')
    run = EvalRun(cfg, args, device, model)
    name, save_dir = run.name, run.save_dir
    full = bool(getattr(args, 'imagenet_c_scores', False))
    pairs = [(c, s) for c in names for s in sevs]
    slot = {p: k for k, p in enumerate(pairs)}
    writers = {}
    if save_dir:
        writers = {p: (ResultWriter if full else RankWriter)(result_dir(save_dir, name, p[0], '%d' % p[1]), rank, world) for p in pairs}
    counters = torch.zeros(2 * len(pairs) + 1, dtype=torch.int64, device=device)      # (top-1, top-5) per pair, then the sample count
    fused = [c for c in ('gaussian_noise', 'speckle_noise') if c in names and len(sevs) > 1]
    scratch = []
    cnt = 0
    t0 = time.time()

    def score(x, pair, labels, lab_host, items):
        logits = run.logits_u8(x)
        w = writers.get(pair)
        keep = w is not None and not full
        p, r = topk_score(logits.float(), labels, ks=(1, 5), hits=counters[2 * slot[pair]:], pred=keep, rank=keep)
        if keep:
            w.write_batch(p, r, lab_host, items)
        elif w is not None:
            w.write_batch(logits, labels, items)

    for items in run.batches(ds, rank, world):
        imgs, labels = ds.batch(items, device)                    # once per batch, whatever the number of pairs
        first = items[0]                                          # global index of the batch's first sample
        cnt += len(items)
        lab_host = labels.tolist() if writers and not full else None
        if not scratch or scratch[0].shape != imgs.shape:
            scratch = [torch.empty_like(imgs) for _ in range(len(sevs) if fused else 1)]
        for c in names:
            cid = C.CORRUPTION_NAMES.index(c)
            if c in fused:
                C.noise_severities_(imgs, scratch, sevs, seeds=[args.seed] * len(sevs), sample_offset=first, corruption_id=cid)
                for k, sv in enumerate(sevs):
                    score(scratch[k], (c, sv), labels, lab_host, items)
            else:
                for sv in sevs:
                    C.corrupt_batch_(imgs, cid, sv, seed=args.seed, sample_offset=first, out=scratch[0])
                    score(scratch[0], (c, sv), labels, lab_host, items)
    paths = {}
    if writers:
        for w in writers.values():
            w.f.close()
        if run.barrier is not None:
            run.barrier()                                         # one for all the files: every shard is on disk before rank 0 merges
        paths = {p: writers[p].close() for p in pairs}
    counters[-1] = cnt
    if dist_up():
        dist.all_reduce(counters)
    flat = counters.tolist()                                      # the loop's only read of a counter
    cnt = int(flat[-1])
    res = None
    if rank == 0:
        ev = ImageNetCEvaluator(topk=(1, 5))
        acc = {}
        for k, p in enumerate(pairs):
            if paths:
                m = ev.eval(paths[p]).metric
                acc['%s/%d' % p] = {'top1': m['top1'], 'top5': m['top5']}
            else:
                acc['%s/%d' % p] = {'top1': float(flat[2 * k] * (100.0 / max(cnt, 1))), 'top5': float(flat[2 * k + 1] * (100.0 / max(cnt, 1)))}
        error = {c: 100.0 - sum(acc['%s/%d' % (c, sv)]['top1'] for sv in sevs) / len(sevs) for c in names}
        res = {'imagenet_c': acc, 'error': error, 'Mean': sum(error.values()) / len(error) if error else None,
               'skipped': plan['skipped'], 'count': cnt, 'world_size': world, 'seconds': time.time() - t0}
        print(json.dumps(res))
    return res


def evaluate(cfg, args, rank, world, device, model=None):
    """Clean / corrupted / attacked evaluation over the sharded dataset; returns the reduced metrics dict."""
    dcfg = cfg.get('data', {})
    if getattr(args, 'imagenet_c', False):
        return evaluate_imagenet_c(cfg, args, rank, world, device, model)
    if getattr(args, 'imagenet_s', False):
        return evaluate_imagenet_s(cfg, args, rank, world, device, model)
    if natural_mode(dcfg):
        return evaluate_natural(cfg, args, rank, world, device, model)
    ds = make_dataset(dcfg, synthetic_size(dcfg), int(dcfg.get('input_size', 224)), 'test')      # a file-backed set brings its own length
    run = EvalRun(cfg, args, device, model)
    use_hip, f_model, mean, std = run.use_hip, run.f_model, run.mean, run.std
    noise = None
    if use_hip:
        from ..model.engine import EngineModel
        n_model = EngineModel(None, takes_normalized=True, engine=f_model.rart_engine)
    if args.corruption:
        from ..noise import AddNoise
        noise = AddNoise('imagenet-c')
        noise.config.update(corruption_name=args.corruption, severity=args.severity)
    attack = None
    if args.attack and args.attack != 'none':
        from ..noise import AddNoise
        attack = AddNoise(args.attack)
        key = 'f_model' if 'f_model' in attack.config else 'model'
        if not use_hip:
            raise RuntimeError('attacks need the GPU path (no CPU fallback)')
        attack.config[key] = f_model if key == 'f_model' else n_model      # ResNet-50 and ViT-B/16: HIP forward + backward
        attack.config['eps'] = parse_eps(args.eps)
        if 'steps' in attack.config and args.steps:
            attack.config['steps'] = args.steps
    # transfer harness: adversarial examples crafted on cfg.model, scored on the target model
    tgt_model = None
    if getattr(args, 'tgt_type', None):
        from ..model import get_model
        tgt = get_model({'type': args.tgt_type}).to(device).eval()
        tgt_model = lambda z, _t=tgt: _t((z - mean) / std)       # noqa: E731
        if use_hip:
            try:
                tgt_model = EngineModel(tgt, takes_normalized=False)
            except Exception:                                   # no HIP engine for this architecture: the torch module stays
                pass
    writer = None
    if run.save_dir:
        from ..metrics import ResultWriter, result_dir
        noise_name = args.corruption or (args.attack if args.attack and args.attack != 'none' else 'none')
        eps_name = ('%d' % args.severity) if args.corruption else (('%.3f' % parse_eps(args.eps)) if noise_name != 'none' else '0')
        writer = ResultWriter(result_dir(run.save_dir, run.name, noise_name, eps_name, tgt_name=getattr(args, 'tgt_name', None)), rank, world)
    c1 = c5 = cnt = 0
    t0 = time.time()
    for items in run.batches(ds, rank, world):
        imgs, labels = ds.batch(items, device)
        first = items[0]                                       # global index of the batch's first sample
        if noise is not None:
            from ..noise import imagenet_c as C
            C.corrupt_batch_(imgs, C.CORRUPTION_NAMES.index(args.corruption), args.severity, seed=args.seed, sample_offset=first)
        if attack is not None:
            # the attack's random starts are a function of (seed, dataset index): set the process-wide counter to the
            # batch's first global index, which every attack reads when no explicit sample_offset is passed
            from ..noise import rng
            rng.manual_seed(args.seed, first)
            x01 = imgs.permute(0, 3, 1, 2).float().div(255.0).contiguous()
            adv_x = attack.add_noise(x01, labels)
            with torch.no_grad():
                logits = (tgt_model or f_model)(adv_x)
        else:
            logits = run.logits_u8(imgs)
        a, b = topk_correct(logits.float(), labels)
        c1, c5, cnt = c1 + a, c5 + b, cnt + len(items)
        if writer is not None:
            writer.write_batch(logits, labels, items)
    if writer is not None:
        writer.close(barrier=run.barrier)
    c1, c5, cnt = all_reduce_counters([c1, c5, cnt], device)
    res = {'top1': c1 / max(cnt, 1), 'top5': c5 / max(cnt, 1), 'count': cnt, 'world_size': world,
           'noise': args.corruption or args.attack or 'none', 'seconds': time.time() - t0}
    if rank == 0:
        print(json.dumps(res))
    return res
