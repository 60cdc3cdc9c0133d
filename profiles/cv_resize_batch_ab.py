"""The ImageNet-S loop with the batched OpenCV resize against the parent commit's per-image cv_resize loop -- the numbers of DESIGN.md
4.9 -- and the identity of the result files of a `--imagenet-s` run between the two trees.

    python profiles/cv_resize_batch_ab.py --parent DIR [--images 256] [--alternations 3] [--out profiles/cv_resize_batch_ab.json]

DIR holds the parent commit's tree with its library built (`git archive HEAD^ | tar -x -C DIR`, then DIR/robustart_amd/csrc/build.py).
The measurement is the `loop` of profiles/resize_batch_ab.py, unchanged: the 256 files of 375 x 500 of profiles/jpeg_reader_ab.py, the
'hip' reader with 8 workers, ResNet-50 on the bf16 engine, decode once, then the eleven operators through image_transfer_batch and the
eleven forwards, each part followed by a synchronize, the second pass of two.  Each tree runs in a worker process of its own; the
driver asks parent and this tree in turn, --alternations times, on one box.  Then `cls_solver --evaluate --imagenet-s --save-dir` runs
once per tree on the first --files files with the same weights, and every file under the two save directories is compared (sha256)."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CV_OPS = ['opencv-nearest', 'opencv-bilinear', 'opencv-cubic', 'opencv-area', 'opencv-lanczos']


def result_files(tree, folder, files, work, name):
    """one `--imagenet-s` run of `tree` in a process of its own -> {relative path: sha256} of everything it saved"""
    meta, cfg, save = os.path.join(work, 'meta.txt'), os.path.join(work, 'cfg_%s.yaml' % name), os.path.join(work, 'save_' + name)
    with open(meta, 'w') as f:
        f.write(''.join(json.dumps({'filename': os.path.join('c0', 'img%04d.jpg' % k), 'label': (37 * k + 11) % 1000}) + '\n'
                        for k in range(files)))
    with open(cfg, 'w') as f:                  # JSON is YAML
        json.dump({'model': {'type': 'resnet50_official', 'kwargs': {'num_classes': 1000}},
                   'data': {'type': 'imagenet', 'read_from': 'fs', 'batch_size': 16, 'input_size': 224, 'test_resize': 256, 'num_workers': 8,
                            'test': {'save_acc_var_neg': True, 'root_dir': folder, 'meta_file': meta, 'image_reader': {'type': 'hip'},
                                     'sampler': {'type': 'distributed'},
                                     'transforms': [{'type': 'Resize', 'kwargs': {'size': [256, 256]}},
                                                    {'type': 'CenterCrop', 'kwargs': {'size': [224, 224]}}, {'type': 'ToTensor'},
                                                    {'type': 'Normalize', 'kwargs': {'mean': [0.485, 0.456, 0.406],
                                                                                     'std': [0.229, 0.224, 0.225]}}]}},
                   'saver': {'pretrain': {'path': os.path.join(work, 'weights.pth')}}}, f)
    code = ('import sys; sys.path.insert(0, %r); from robustart_amd.train import cls_solver as S; '
            'S.main(["--config", %r, "--evaluate", "--imagenet-s", "--save-dir", %r])' % (tree, cfg, save))
    subprocess.run([sys.executable, '-c', code], check=True, cwd=tree, stdout=subprocess.DEVNULL, timeout=600)
    out = {}
    for d, _, names in os.walk(save):
        for n in names:
            with open(os.path.join(d, n), 'rb') as f:
                out[os.path.relpath(os.path.join(d, n), save)] = hashlib.sha256(f.read()).hexdigest()
    return out


def spread(values):
    return {'min': min(values), 'max': max(values), 'all': values}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', required=True)
    ap.add_argument('--images', type=int, default=256)
    ap.add_argument('--alternations', type=int, default=3)
    ap.add_argument('--files', type=int, default=48)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert os.path.isdir(a.parent), '--parent: the directory of the parent commit\'s tree'
    sys.path.insert(0, ROOT)
    from profiles.jpeg_reader_ab import write_files
    from profiles.resize_batch_ab import Worker
    parent = os.path.abspath(a.parent)
    res = {'images': a.images, 'image_hw': [375, 500], 'alternations': a.alternations, 'cpus_available': len(os.sched_getaffinity(0))}
    with tempfile.TemporaryDirectory() as folder, tempfile.TemporaryDirectory() as work:
        write_files(folder, a.images)
        trees = {'parent': Worker(parent, folder, a.images), 'this': Worker(ROOT, folder, a.images)}
        try:
            loops = {k: [] for k in trees}
            for _ in range(a.alternations):
                for k, w in trees.items():                 # parent, then this tree
                    loops[k].append(w.ask('loop'))
        finally:
            for w in trees.values():
                w.close()
        res['loops'] = loops
        summary = {}
        for key in ['resize_opencv_ms', 'resize_pil_ms', 'decode_ms', 'forward_total_ms', 'total_ms']:
            summary[key] = {k: spread([r[key] for r in loops[k]]) for k in trees}
        for op in CV_OPS:
            summary[op] = {k: spread([r['resize_ms'][op] for r in loops[k]]) for k in trees}
        # accepted: in every alternation this tree is below the parent by more than the spread between repeats on one build
        for key, s in summary.items():
            if key.startswith('opencv') or key in ('resize_opencv_ms', 'total_ms'):
                noise = max(s['parent']['max'] - s['parent']['min'], s['this']['max'] - s['this']['min'])
                s['gain_every_alternation_ms'] = [p - t for p, t in zip(s['parent']['all'], s['this']['all'])]
                s['repeat_spread_ms'] = noise
                s['below_parent_beyond_spread'] = all(g > noise for g in s['gain_every_alternation_ms'])
        res['summary'] = summary
        # the result files of one --imagenet-s run per tree, same weights
        import torch
        sys.path.insert(0, ROOT)
        from robustart_amd.model import get_model
        from robustart_amd.model.resnet_torch import randomize_bn_stats
        torch.manual_seed(5)
        torch.save({'model': randomize_bn_stats(get_model({'type': 'resnet50_official'}), 5).eval().state_dict()},
                   os.path.join(work, 'weights.pth'))
        files = {k: result_files(t, folder, min(a.files, a.images), work, k) for k, t in (('parent', parent), ('this', ROOT))}
        res['result_files'] = {'count': len(files['this']), 'files_per_run': min(a.files, a.images),
                               'byte_identical': files['parent'] == files['this'] and len(files['this']) > 0,
                               'differing': sorted(n for n in set(files['parent']) | set(files['this'])
                                                   if files['parent'].get(n) != files['this'].get(n))}
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
