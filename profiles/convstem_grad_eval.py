"""Gradient evaluation (forward + backward-to-input) of the ConvStem models next to their base models, the measurement DESIGN.md 4.6.4
asks for: CUDA events, 3 warm-up runs, median of 11.  DESIGN.md 4.6.4 says whether its numbers have been taken.

    python profiles/convstem_grad_eval.py [--batch 256] [--out result.json] [--types convnext_base,convnext_base_cvst,...]
    python profiles/convstem_grad_eval.py --steps-only 1 --types convnext_base_cvst --precision bf16

Prints one JSON object: per (type, precision) the median time of `forward_backward` and images / s, and for the ConvStem types the time
of the stem chain alone (its forward and its backward on a random output gradient) with its share of the gradient evaluation.
--steps-only N runs two warm-up evaluations, then N evaluations of ONE (type, precision) and nothing else: the command to put under
`rocprofv3 --kernel-trace --stats` (the per-kernel CSV then holds N + 2 calls of every launch)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
TYPES = 'convnext_base,convnext_base_cvst,vit_base,vit_base_cvst'


def timed(torch, fn, n=11, warm=3):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return statistics.median(out)


def stem_alone(torch, eng, x01, B):
    """-> a callable that runs the stem chain's forward and backward on buffers of its own"""
    if hasattr(eng, 'dims'):                       # ConvNeXt: the dense stage-0 input
        out = eng._act('prof_out', (B * 56 * 56, eng.dims[0]))
        g = eng._act('prof_g', (B * 56 * 56, eng.dims[0]))
        slot_f, slot_b = {}, {}
    else:                                          # ViT: the patch rows of the token matrix
        P, T = 196, 197
        out = eng._act('prof_out', (B, T, eng.D))
        g = eng._act('prof_g', (B, T, eng.D))
        slot_f = dict(rows_per_image=P, dst_rows_per_image=T, dst_row_off=1)
        slot_b = dict(rows_per_image=P, src_rows_per_image=T, src_row_off=1)
    g.copy_((0.01 * torch.randn(g.shape, device='cuda')).to(g.dtype))

    def run():
        eng.cvst.forward(x01, False, MEAN, STD, B, 224, 224, out, **slot_f)
        eng.cvst.backward(g, STD, **slot_b)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--out', default=None)
    ap.add_argument('--types', default=TYPES)
    ap.add_argument('--precision', default='bf16,fp32x')
    ap.add_argument('--steps-only', type=int, default=0)
    a = ap.parse_args()
    import torch
    from robustart_amd.model import get_model
    from robustart_amd.model.engine import make_engine
    assert torch.cuda.is_available(), 'this measurement needs the GPU'
    B = a.batch
    torch.manual_seed(0)
    x01 = torch.rand(B, 3, 224, 224, device='cuda')
    y = torch.randint(0, 1000, (B,), device='cuda')
    res = {'batch': B}
    for t in a.types.split(','):
        model = get_model({'type': t}).cuda().eval()
        for prec in a.precision.split(','):
            eng = make_engine(model, 'cuda', prec)
            if a.steps_only:
                for _ in range(2 + a.steps_only):
                    eng.forward_backward(x01, MEAN, STD, y, 0)
                torch.cuda.synchronize()
                return
            r = {'grad_eval_ms': timed(torch, lambda: eng.forward_backward(x01, MEAN, STD, y, 0))}
            r['images_per_s'] = 1e3 * B / r['grad_eval_ms']
            if getattr(eng, 'cvst', None) is not None:
                r['stem_fwd_bwd_ms'] = timed(torch, stem_alone(torch, eng, x01, B))
                r['stem_share'] = r['stem_fwd_bwd_ms'] / r['grad_eval_ms']
            res['%s/%s' % (t, prec)] = r
            print(json.dumps({'%s/%s' % (t, prec): r}), flush=True)
            eng._buf.clear()
            del eng
            torch.cuda.empty_cache()
        del model
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
