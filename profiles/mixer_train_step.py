"""MLP-Mixer-B/16 training step on the GPU, the numbers of DESIGN.md 4.7 (training): CUDA events, median of 5 after warm-up.

    python profiles/mixer_train_step.py [--batch 256] [--out result.json] [--steps-only N]

Prints one JSON object: train-mode forward + backward next to the gradient evaluation (forward + backward-to-input), the two
token-weight-gradient launches (median us, TFLOP/s) against torch.einsum on the same bf16 operands, the share of the step the
token-parameter launches take, a whole training step (forward, loss, backward, AdamW + EMA, repack) against torch autograd of
model/mixer_torch.py in fp32 and under bf16 autocast with torch.optim.AdamW, and peak memory.
--steps-only N runs N plain engine steps and nothing else (the command to put under `rocprofv3 --kernel-trace --stats`)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def timed(torch, fn, n=5, warm=2):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--out', default=None)
    ap.add_argument('--steps-only', type=int, default=0)
    ap.add_argument('--skip-torch', action='store_true')
    a = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from robustart_amd.model import get_model
    from robustart_amd.model.engine_base import EngineBase, wgrad_split_tokens
    from robustart_amd.model.mixer_train_engine import MixerTrainEngine
    from robustart_amd.train.arena import HipOptimizer, ParamArena, label_smooth_ce
    assert torch.cuda.is_available(), 'this measurement needs the GPU'
    B = a.batch
    torch.manual_seed(0)
    model = get_model({'type': 'mixer_b16_224', 'kwargs': {'drop_path': 0.0, 'drop_path_rate': 0.0}}).cuda().train()
    arena = ParamArena(model)
    opt = HipOptimizer(arena, kind='AdamW', lr=1e-5, weight_decay=0.05, betas=(0.9, 0.999), eps=1e-8, ema_decay=0.9999)
    eng = MixerTrainEngine(model, 'cuda', on_grad_ready=arena.grad_ready)
    x01 = torch.rand(B, 3, 224, 224, device='cuda')
    y = torch.randint(0, 1000, (B,), device='cuda')

    def fwd_bwd():
        logits = eng.forward(x01, False, MEAN, STD)
        eng.backward(label_smooth_ce(logits, y, 0.1, 1.0 / B)[1])

    def step():
        fwd_bwd()
        arena.finish_grad_exchange()
        opt.step(grad_scale=1.0)
        eng.repack()

    if a.steps_only:
        for _ in range(a.steps_only):
            fwd_bwd()
        torch.cuda.synchronize()
        return
    res = {'batch': B}
    torch.cuda.reset_peak_memory_stats()
    res['train_fwd_bwd_ms'] = timed(torch, fwd_bwd)
    res['peak_memory_GiB'] = torch.cuda.max_memory_allocated() / 2 ** 30
    res['grad_eval_ms'] = timed(torch, lambda: eng.forward_backward(x01, MEAN, STD, y, 0))
    res['train_step_ms'] = timed(torch, step)
    res['train_step_images_per_s'] = 1e3 * B / res['train_step_ms']
    # per-launch times of the token-parameter kernels inside a step
    fwd_bwd()
    eng.profile = []
    fwd_bwd()
    torch.cuda.synchronize()
    kinds = {}
    for rec in eng.profile:
        kinds.setdefault(rec[3], []).append((rec[1].elapsed_time(rec[2]) * 1e3, rec[0]))
    eng.profile = None
    tok_us = 0.0
    for k in ('tok_wgrad', 'tok_wgrad_reduce', 'tok_rowsum'):
        us = [u for u, _ in kinds.get(k, [])]
        tok_us += sum(us)
        res[k + '_median_us'] = statistics.median(us)
        res[k + '_launches'] = len(us)
    res['tok_wgrad_event_TFLOPs'] = statistics.median(f / u * 1e-6 for u, f in kinds['tok_wgrad'])
    res['token_parameter_share_of_fwd_bwd'] = tok_us * 1e-3 / res['train_fwd_bwd_ms']
    # the two launches alone (back to back, no events between the kernel and its fold) against torch.einsum
    T, Ht, D = eng.T, eng.layers[0]['tok_hidden'], eng.D
    g = torch.Generator(device='cuda').manual_seed(1)
    ln = torch.randn(B, T, D, device='cuda', generator=g).to(torch.bfloat16)
    du = torch.randn(B, Ht, D, device='cuda', generator=g).to(torch.bfloat16)
    grad = torch.empty(Ht, T, device='cuda')
    flops = 2.0 * B * Ht * T * D
    res['split_rule'] = wgrad_split_tokens(B, Ht, T, EngineBase.wgrad_target_wgs)
    for target in (256, 512, 1024, 2048):
        eng.wgrad_target_wgs = target
        ms = timed(torch, lambda: eng._tok_wgrad(du, ln, Ht, T, B, grad), n=9, warm=3)
        res['tok_wgrad_dW1_target%d' % target] = {'us': ms * 1e3, 'TFLOPs': flops / ms * 1e-9,
                                                  'splits': wgrad_split_tokens(B, Ht, T, target)[0]}
    eng.wgrad_target_wgs = EngineBase.wgrad_target_wgs
    grad2 = torch.empty(T, Ht, device='cuda')
    ms = timed(torch, lambda: eng._tok_wgrad(ln, du, T, Ht, B, grad2), n=9, warm=3)
    res['tok_wgrad_dW2'] = {'us': ms * 1e3, 'TFLOPs': flops / ms * 1e-9}
    ms = timed(torch, lambda: torch.einsum('bhd,btd->ht', du, ln), n=9, warm=3)
    res['torch_einsum_bhd_btd_ht'] = {'us': ms * 1e3, 'TFLOPs': flops / ms * 1e-9}
    ms = timed(torch, lambda: torch.einsum('btd,bhd->th', ln, du), n=9, warm=3)
    res['torch_einsum_btd_bhd_th'] = {'us': ms * 1e3, 'TFLOPs': flops / ms * 1e-9}
    ref = torch.einsum('bhd,btd->ht', du.double(), ln.double())
    eng._tok_wgrad(du, ln, Ht, T, B, grad)
    res['tok_wgrad_vs_fp64_rel'] = ((grad.double() - ref).norm() / ref.norm()).item()
    bias = torch.empty(Ht, device='cuda')
    res['tok_rowsum_Ht_us'] = 1e3 * timed(torch, lambda: eng._tok_rowsum(du, Ht, B, bias), n=9, warm=3)
    lib, L = eng.lib, __import__('robustart_amd._lib', fromlist=['x'])
    out = torch.empty_like(du)
    res['gelu_recompute_htok_us'] = 1e3 * timed(
        torch, lambda: L.check(lib.rart_gelu_bf16(L.ptr(du), L.ptr(out), du.numel(), L.stream_ptr())), n=9, warm=3)
    print(json.dumps(res), flush=True)
    if not a.skip_torch:
        # what the reference runs: torch autograd of the same module, fp32 and bf16 autocast, with torch.optim.AdamW
        del eng, opt, arena
        torch.cuda.empty_cache()
        mean = torch.tensor(MEAN, device='cuda').view(1, 3, 1, 1)
        std = torch.tensor(STD, device='cuda').view(1, 3, 1, 1)
        for name, amp in (('torch_bf16_autocast', True), ('torch_fp32', False)):
            m = get_model({'type': 'mixer_b16_224'}).cuda().train()
            topt = torch.optim.AdamW(m.parameters(), lr=1e-5, weight_decay=0.05)

            def tstep(with_opt=True):
                topt.zero_grad(set_to_none=True)
                with torch.autocast('cuda', dtype=torch.bfloat16, enabled=amp):
                    o = m((x01 - mean) / std)
                F.cross_entropy(o.float(), y, label_smoothing=0.1).backward()
                if with_opt:
                    topt.step()
            res[name + '_fwd_bwd_ms'] = timed(torch, lambda: tstep(False), n=3, warm=2)
            res[name + '_step_ms'] = timed(torch, tstep, n=3, warm=1)
            res[name + '_step_images_per_s'] = 1e3 * B / res[name + '_step_ms']
            del m, topt
            torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
