"""Streaming fused attention (csrc/vit_stream.hip) timed on one GPU, through ViTEngine's own attention calls.

    python profiles/att_stream_ab.py [--out profiles/att_stream_ab.json] [--reps 30]

bf16: the streaming entries against the unfused decomposition (batched GEMMs + soft-max rows on score-sized temporaries), forward and
backward, at B = 32, H = 12, T = 577 and B = 64, H = 16, T = 257.  Pairs: no other path exists above 256 keys, so time and issued-MFMA
TFLOP/s of the streaming entries at the same shapes.  Both precisions at T = 224 (B = 64, H = 12): the streaming entries beside the
resident kernels, for the record.  The variants of a shape alternate in one process on random data; every call is timed with device
events; median and minimum over the repetitions."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MFMA_FLOP = 2 * 32 * 32 * 16
# MFMA instructions per (32-row tile, 32-row tile) of a product chain, one plane; pairs issue three times as many
FWD_MFMA, BWD_MFMA = 8, 32            # forward: S 4 + PV 4; backward: query side S 4 (sweep 1) + S 4 + dP 4 + dQ 4, key side S 4 + dP 4 + dV 4 + dK 4


def issued_flop(B, H, T, per_tile_pair, pair):
    tiles, streamed = (T + 31) // 32, 2 * ((T + 63) // 64)      # a wave's tile meets every 32-row tile of every 64-row chunk
    return B * H * tiles * streamed * per_tile_pair * (3 if pair else 1) * MFMA_FLOP


def engine(H, precision):
    """a ViTEngine of H heads of 64: its attention calls take the token count as an argument, so the module behind it is a small one"""
    from robustart_amd.model.vit_engine import ViTEngine
    from robustart_amd.model.vit_torch import VisionTransformer
    torch.manual_seed(0)
    m = VisionTransformer(img_size=32, num_classes=8, embed_dim=64 * H, depth=1, num_heads=H).eval()
    return ViTEngine(m, 'cuda', precision=precision)


def operands(B, H, T, pair):
    D, rows = 64 * H, B * T
    g = torch.Generator(device='cuda').manual_seed(T)
    r = lambda *s: torch.randn(*s, device='cuda', generator=g)

    def store(t, slack=0):
        if pair:
            hi = t.to(torch.bfloat16)
            return torch.stack([hi, (t - hi.float()).to(torch.bfloat16)]).contiguous()
        return torch.cat([t.to(torch.bfloat16), torch.zeros(slack, t.shape[1], dtype=torch.bfloat16, device='cuda')]).contiguous()
    qkv = store(r(rows, 3 * D) * 0.7, 256)
    datt = store(r(rows, D))
    att = store(torch.zeros(rows, D, device='cuda'))
    dqkv = store(torch.zeros(rows, 3 * D, device='cuda'))
    return qkv, att, datt, dqkv


def time_variants(variants, reps, warmup=3):
    """variants: {name: callable}; they alternate, each call between two device events -> {name: (median us, min us)}"""
    times = {k: [] for k in variants}
    for i in range(warmup + reps):
        for name, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if i >= warmup:
                times[name].append(a.elapsed_time(b) * 1e3)
    return {k: (statistics.median(v), min(v)) for k, v in times.items()}


def shape_report(B, H, T, precision, other, reps):
    """the streaming route and `other` ('unfused' | 'resident' | None) at one shape"""
    pair = precision != 'bf16'
    eng = engine(H, precision)
    qkv, att, datt, dqkv = operands(B, H, T, pair)

    def route(stream, fused):
        def set_():
            eng.stream_attention, eng.fused_attention, eng.fused_attention_bwd = stream, fused, fused
        return set_
    routes = {'stream': route(True, True)}
    if other == 'unfused':
        routes['unfused'] = route(None, False)
    if other == 'resident':
        routes['resident'] = route(False, True)
    variants, outs = {}, {}
    for name, set_ in routes.items():
        def fwd(set_=set_):
            set_()
            eng._attention(qkv, att, B, T)

        def bwd(set_=set_):
            set_()
            eng._attention_bwd(qkv, att, datt, dqkv, B, T)
        variants[name + '_fwd'], variants[name + '_bwd'] = fwd, bwd
        fwd()
        bwd()
        outs[name] = (att.clone(), dqkv.clone())
    rep = dict(B=B, H=H, T=T, precision=precision, reps=reps)
    if other:                                   # the two routes compute the same thing at the timed size
        val = (lambda t: t[0].double() + t[1].double()) if pair else (lambda t: t[:B * T].double())
        for i, part in enumerate(('att', 'dqkv')):
            a, b = val(outs['stream'][i]).flatten(), val(outs[other][i]).flatten()
            rep['%s_stream_vs_%s_rel_l2' % (part, other)] = ((a - b).norm() / b.norm()).item()
    for name, (med, mn) in time_variants(variants, reps).items():
        rep[name + '_us'] = dict(median=round(med, 1), min=round(mn, 1))
    for d, per in (('fwd', FWD_MFMA), ('bwd', BWD_MFMA)):
        rep['stream_%s_issued_mfma_tflops' % d] = round(issued_flop(B, H, T, per, pair) / rep['stream_%s_us' % d]['median'] / 1e6, 1)
    return rep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), 'att_stream_ab.json'))
    ap.add_argument('--reps', type=int, default=30)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'this measurement needs the GPU'
    res = dict(device=torch.cuda.get_device_name(0), protocol='variants of a shape alternate in one process, random data, one pair of '
               'device events per call, median and min over the repetitions; issued-MFMA TFLOP/s counts every MFMA instruction the '
               'streaming kernels issue (padded tiles included) over the median', shapes=[])
    for B, H, T in ((32, 12, 577), (64, 16, 257)):
        res['shapes'].append(shape_report(B, H, T, 'bf16', 'unfused', a.reps))
        res['shapes'].append(shape_report(B, H, T, 'fp32x', None, a.reps))
    for precision in ('bf16', 'fp32x'):
        res['shapes'].append(shape_report(64, 12, 224, precision, 'resident', a.reps))
    for s in res['shapes']:
        print(json.dumps(s))
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
