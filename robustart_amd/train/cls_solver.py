"""cls_solver-shaped train / eval entry for the hot path.

Reference: RobustART/train/__init__.py:1 re-exports `prototype.prototype.solver.cls_solver`, whose source is
absent; behaviour is taken from the YAML schema (exprs/nips_benchmark/pgd_adv_train/resnet50/config.yaml:1-61),
the launchers (`python -m ...solver.X --config cfg [--evaluate] [--attack NAME --eps E]`,
exprs/nips_benchmark/batch_eval_adv/eval.sh:43) and the only readable instance of the loop,
cifar10/code/train.py:96-127.

    python -m robustart_amd.train.cls_solver --config cfg.yaml --evaluate [--attack pgd_linf --eps 2/255]
    python -m torch.distributed.run --nproc-per-node 8 -m robustart_amd.train.cls_solver --config cfg.yaml

One process per GPU.  Evaluation: samples shard over ranks (distributed, non-repeating sampler), noise comes from
AddNoise (HIP kernels), the forward from the HIP engine, and the ONLY collective is one all-reduce of the
(top-1, top-5, count) counters.  Adversarial training (PGD-k inner loop, BN in eval mode during the attack,
cifar10/code/train.py:105-111): the attack runs on the HIP engine with the current weights re-folded; the
train-mode forward/backward of ResNet-50 runs on the HIP train engine (model/train_engine.py: igemm contractions,
batch-statistics BatchNorm kernels, split-K weight gradients; other architectures use torch autograd as scaffold); the
loss + its gradient (label-smoothed CE), the optimizer (SGD-Nesterov / AdamW), the EMA and the gradient reset are HIP
kernels over flat parameter arenas (train/arena.py), and the gradient exchange is a few large all-reduces on arena
slices over RCCL/xGMI, overlapped with backward unless `dist.sync: True`.
"""
import argparse
import json
import math
import os
import sys

import torch
import torch.distributed as dist
import torch.nn.functional as F

# the solver's parts live in their own modules; every name that was importable from here still is
from .checkpoint import build_model, build_model_and_resume, load_checkpoint_file, load_pretrain, save_checkpoint  # noqa: F401
from .data import (IMAGENET_MEAN, IMAGENET_STD, EpochSampler, FakeImageNet, FileImageNet, StructuredFakeImageNet, _entry, _LIST_TYPES,  # noqa: F401
                   _square, _TransformName, make_dataset, read_meta_file, read_transforms, shard_indices)
from .evaluate import (_once_each, all_reduce_counters, evaluate, evaluate_imagenet_c, evaluate_imagenet_s, evaluate_natural,  # noqa: F401
                       imagenet_c_names, imagenet_c_plan, imagenet_c_severities, imagenet_s_ops, natural_datasets, natural_mode, parse_eps,
                       read_class_map, read_frost_textures, subset_of, topk_correct)


def load_config(path):
    import yaml
    with open(path) as f:
        return yaml.safe_load(f)


def resolve_schedule(cfg, n_train, batch_size, world, default_max_iter=20):
    """-> (max_iter, warmup_steps) from the reference's key set (pgd_adv_train/resnet50/config.yaml:18-29): the
    iteration keys `lr_scheduler.kwargs.{max_iter, warmup_steps}` when present, else the epoch keys `max_epoch` /
    `warmup_epoch` times the iterations of one epoch of the distributed_iteration sampler,
    ceil(len(train set) / (batch_size * world_size)).  A top-level `max_iter` (this build's own shortcut, used by the
    tests) wins over both."""
    lk = (cfg.get('lr_scheduler') or {}).get('kwargs') or {}
    per_epoch = max(1, -(-int(n_train) // (int(batch_size) * int(world))))
    if cfg.get('max_iter') is not None:
        max_iter = int(cfg['max_iter'])
    elif lk.get('max_iter') is not None:
        max_iter = int(lk['max_iter'])
    elif lk.get('max_epoch') is not None:
        max_iter = int(round(float(lk['max_epoch']) * per_epoch))
    else:
        max_iter = int(default_max_iter)
    if lk.get('warmup_steps') is not None:
        warm = int(lk['warmup_steps'])
    elif lk.get('warmup_epoch') is not None:
        warm = int(round(float(lk['warmup_epoch']) * per_epoch))
    else:
        warm = max(max_iter // 20, 1)
    return max_iter, min(warm, max_iter)


def cosine_lr(step, total, base_lr, warmup_lr, warmup_steps, min_lr=0.0):
    """lr_scheduler.type CosineEpoch with linear warm-up (config.yaml:21-29)."""
    if step < warmup_steps:
        return base_lr + (warmup_lr - base_lr) * step / max(warmup_steps, 1)
    t = (step - warmup_steps) / max(total - warmup_steps, 1)
    return min_lr + 0.5 * (warmup_lr - min_lr) * (1 + math.cos(math.pi * t))


def init_dist():
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local = int(os.environ.get('LOCAL_RANK', '0'))
    use_cuda = torch.cuda.is_available()
    if use_cuda:
        torch.cuda.set_device(local)
    # RART_FORCE_DIST=1: join the process group even as a single rank (a one-GPU box then creates the RCCL communicator and runs
    # the same collectives the 8-GPU launch does)
    if (world > 1 or os.environ.get('RART_FORCE_DIST') == '1') and not dist.is_initialized():
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('MASTER_PORT', '29511')
        dist.init_process_group('nccl' if use_cuda else 'gloo')       # "nccl" == RCCL on ROCm
    return rank, world, torch.device('cuda', local) if use_cuda else torch.device('cpu')


def train(cfg, args, rank, world, device):
    """(Adversarial) training loop; returns the last loss (float) for tests."""
    dcfg = cfg.get('data', {})
    n = int(dcfg.get('fake_size', 512))
    bs = int(dcfg.get('batch_size', 32))
    size = int(dcfg.get('input_size', 224))
    # `mixup` / `cutmix` (augmentation/resnet50/config.yaml:30-31): the Beta parameters of the batch mixing, None = off (train/mixing.py)
    from . import mixing
    mixup_alpha, cutmix_alpha = mixing.mix_alphas(cfg)
    mix_on = mixup_alpha is not None or cutmix_alpha is not None
    if mix_on and cfg.get('adv_train', None):  # before the model is built or reaches the device: no reference config combines the two
        raise ValueError('adv_train together with an active %s key: mixing under adversarial training is not defined here (no reference '
                         'config combines them); drop one of the two' % ' / '.join(k for k, v in (('mixup', mixup_alpha), ('cutmix', cutmix_alpha)) if v is not None))
    ds = make_dataset(dcfg, n, size, 'train')
    n = len(ds)
    max_iter, warmup_steps = resolve_schedule(cfg, n, bs, world, getattr(args, 'max_iter', 20))
    model, resume = build_model_and_resume(cfg, args)
    from ..model.convstem_torch import convstem_of
    if convstem_of(model) is not None:         # before the model reaches the device: every reference config of these types evaluates
        raise NotImplementedError('training %r: the ConvStem models are evaluation only (forward and backward-to-input on the HIP '
                                  'engines; there is no train engine for the stem)' % (cfg['model']['type'],))
    from ..model.resnet_torch import FAMILY as resnet_family
    if cfg['model']['type'] in resnet_family:  # likewise: ResNet-101/152, Wide-ResNet and ResNeXt are evaluated, attacked and corrupted
        raise NotImplementedError('training %r: this member of the ResNet family is evaluation only (forward and backward-to-input on '
                                  'the HIP engine; ResNetTrainEngine is built and measured for resnet50_official alone)' % (cfg['model']['type'],))
    from ..model.densenet_torch import FAMILY as densenet_family
    if cfg['model']['type'] in densenet_family:  # likewise: DenseNet-121/169/201 are evaluated, attacked and corrupted
        raise NotImplementedError('training %r: the DenseNet models are evaluation only (forward and backward-to-input on the HIP '
                                  'engine; there is no train engine for them)' % (cfg['model']['type'],))
    from ..model.resnet_basic_torch import BasicResNet
    if isinstance(model, BasicResNet):           # likewise: ResNet-18/34 are evaluated, attacked and corrupted
        raise NotImplementedError('training %r: the BasicBlock ResNets are evaluation only (forward and backward-to-input on the HIP '
                                  'engine; there is no train engine for them)' % (cfg['model']['type'],))
    model = model.to(device)
    from ..model.convnext_torch import ConvNeXt, ConvNeXtV2
    from ..model.mixer_torch import MlpMixer
    on_hip = device.type == 'cuda' and args.engine == 'hip' and getattr(args, 'train_engine', 'hip') == 'hip'
    if isinstance(model, MlpMixer) and not on_hip:
        raise NotImplementedError('training %r on %s with --engine %s --train-engine %s: MLP-Mixer trains only on MixerTrainEngine, '
                                  'on the GPU with --engine hip --train-engine hip (there is no CPU or torch-engine path)'
                                  % (cfg['model']['type'], device.type, args.engine, getattr(args, 'train_engine', 'hip')))
    if isinstance(model, ConvNeXtV2) and not on_hip:
        raise NotImplementedError('training %r on %s with --engine %s --train-engine %s: ConvNeXt-V2 trains only on ConvNeXtTrainEngine, '
                                  'on the GPU with --engine hip --train-engine hip (there is no CPU or torch-engine path)'
                                  % (cfg['model']['type'], device.type, args.engine, getattr(args, 'train_engine', 'hip')))
    if isinstance(model, ConvNeXt) and not on_hip:
        raise NotImplementedError('training %r on %s with --engine %s --train-engine %s: there is no ConvNeXt train engine on this path; '
                                  'ConvNeXtTrainEngine runs on the GPU with --engine hip --train-engine hip'
                                  % (cfg['model']['type'], device.type, args.engine, getattr(args, 'train_engine', 'hip')))
    ocfg = cfg.get('optimizer', {'type': 'SGD', 'kwargs': {'nesterov': True, 'momentum': 0.9, 'weight_decay': 1e-4}})
    okw = dict(ocfg.get('kwargs', {}))
    lcfg = cfg.get('lr_scheduler', {}).get('kwargs', {})
    base_lr, warmup_lr = float(lcfg.get('base_lr', 0.1)), float(lcfg.get('warmup_lr', 0.4))
    min_lr = float(lcfg.get('min_lr', 0.0))
    kind = ocfg.get('type', 'SGD')
    # flat arenas: parameters / gradients are views; the exchange is a few large all-reduces on arena slices,
    # overlapped with backward unless the config asks for `dist.sync: True`
    from .arena import HipOptimizer, ParamArena, label_smooth_ce, label_smooth_ce_mix
    no_wd = ocfg.get('no_wd', {}) or {}
    norm_names, fc_bias_names = set(), set()
    for mn, mod in model.named_modules():
        if isinstance(mod, (torch.nn.modules.batchnorm._BatchNorm, torch.nn.LayerNorm, torch.nn.GroupNorm)):
            norm_names.update(mn + '.' + pn for pn, _ in mod.named_parameters(recurse=False))
        if isinstance(mod, torch.nn.Linear) and mod.bias is not None:
            fc_bias_names.add(mn + '.bias')

    def no_decay(name, p):
        return (bool(no_wd.get('norm', False)) and name in norm_names) or \
               (bool(no_wd.get('fc', False)) and name in fc_bias_names)

    arena = ParamArena(model, bucket_bytes=int(cfg.get('dist', {}).get('bucket_mb', 48)) << 20, no_decay=no_decay,
                       overlap=not bool(cfg.get('dist', {}).get('sync', False)))
    ema_on = bool(cfg.get('ema', {}).get('enable', False))
    decay = float(cfg.get('ema', {}).get('kwargs', {}).get('decay', 0.9999))
    use_hip_opt = device.type == 'cuda' and args.engine == 'hip'
    ema = None
    if use_hip_opt:
        # SGD-Nesterov / AdamW + EMA + gradient reset: one HIP launch over the arena (rart_sgd_step_f32 / rart_adamw_step_f32)
        opt = HipOptimizer(arena, kind=kind, lr=base_lr, momentum=float(okw.get('momentum', 0.9)),
                           nesterov=bool(okw.get('nesterov', False)), weight_decay=float(okw.get('weight_decay', 0.0)),
                           betas=tuple(okw.get('betas', (0.9, 0.999))), eps=float(okw.get('eps', 1e-8)),
                           ema_decay=decay if ema_on else None)
    else:
        # CPU scaffold for the multi-process tests (gloo): torch's optimizer on the same arena views
        groups = [{'params': [p for n, p in zip(arena.names, arena.params) if not no_decay(n, p)]},
                  {'params': [p for n, p in zip(arena.names, arena.params) if no_decay(n, p)], 'weight_decay': 0.0}]
        groups = [g for g in groups if g['params']]
        opt = torch.optim.AdamW(groups, lr=base_lr, **okw) if kind == 'AdamW' else torch.optim.SGD(groups, lr=base_lr, **okw)
        if ema_on:
            ema = arena.flat_p.clone()
    ema_buffers = {k: v.detach().clone() for k, v in model.named_buffers() if v.dtype.is_floating_point} if ema_on else {}
    train_engine = None
    if use_hip_opt and getattr(args, 'train_engine', 'hip') == 'hip':
        from ..model.resnet_torch import ResNet
        from ..model.vit_torch import VisionTransformer
        model.train()
        if isinstance(model, ResNet) and size % 32 == 0:
            from ..model.train_engine import ResNet50TrainEngine
            train_engine = ResNet50TrainEngine(model, device, on_grad_ready=arena.grad_ready)
        elif isinstance(model, VisionTransformer):
            from ..model.vit_train_engine import ViTTrainEngine
            train_engine = ViTTrainEngine(model, device, on_grad_ready=arena.grad_ready)
        elif isinstance(model, ConvNeXt):
            from ..model.convnext_train_engine import ConvNeXtTrainEngine
            train_engine = ConvNeXtTrainEngine(model, device, on_grad_ready=arena.grad_ready)
        elif isinstance(model, MlpMixer):
            from ..model.mixer_train_engine import MixerTrainEngine
            train_engine = MixerTrainEngine(model, device, on_grad_ready=arena.grad_ready)
    ls = float(cfg.get('label_smooth', 0.0))
    adv = cfg.get('adv_train', None)                        # {'eps': '4/255', 'steps': 3, 'rel_stepsize': 0.4}
    mean = torch.tensor(IMAGENET_MEAN, device=device).view(1, 3, 1, 1)
    std = torch.tensor(IMAGENET_STD, device=device).view(1, 3, 1, 1)
    use_amp = device.type == 'cuda' and cfg.get('bf16', True)
    sampler = EpochSampler(n, bs, rank, world, int(dcfg.get('seed', 0)), bool(dcfg.get('shuffle', True)))
    loss_v = float('nan')
    attack_model = None
    scfg = cfg.get('saver', {}) or {}
    save_dir = scfg.get('save_dir') or getattr(args, 'ckpt_dir', None)
    save_freq = int(scfg.get('save_freq', scfg.get('val_freq', 0)) or 0)     # the reference solver saves at val_freq
    # ---- resume (--recover / saver.pretrain.path with 'optimizer' + 'last_iter' in the file and not ignored): the
    # momentum / Adam moments, the EMA (parameters and buffers) and the schedule position continue where they stopped
    start_iter = 0
    if resume.get('last_iter') is not None and resume.get('optimizer') is not None:
        start_iter = min(int(resume['last_iter']), max_iter)
        ost = resume['optimizer']
        # the two optimizer paths keep different state (flat arenas of the HIP step vs torch.optim's per-parameter
        # dicts): resuming across them would either fail deep inside load_state_dict or silently restart the moments
        # while the schedule continues -- refuse with a message that says so
        is_torch_state = isinstance(ost, dict) and ost.get('torch') is not None
        if use_hip_opt:
            if is_torch_state or not isinstance(ost, dict) or 'kind' not in ost:
                raise RuntimeError("checkpoint's optimizer state was written by the torch scaffold (--engine torch); it cannot "
                                   "resume the HIP optimizer. Resume with --engine torch, or drop it with "
                                   "saver.pretrain.ignore.key: ['optimizer', 'last_iter'] to fine-tune from the weights")
            if ost.get('kind') != kind:
                raise RuntimeError('checkpoint optimizer kind %r != configured optimizer %r' % (ost.get('kind'), kind))
            opt.load_state_dict(ost)
        else:
            if not is_torch_state:
                raise RuntimeError("checkpoint's optimizer state was written by the HIP optimizer; it cannot resume the torch "
                                   "scaffold (--engine torch / CPU). Resume on the GPU with --engine hip, or ignore "
                                   "['optimizer', 'last_iter'] to fine-tune from the weights")
            opt.load_state_dict(ost['torch'])
        if ema_on and resume.get('ema') is not None:
            esd = {(k[7:] if k.startswith('module.') else k): v for k, v in resume['ema'].items()}
            from ..model.vit_torch import VisionTransformer, legacy_vit_keys
            if isinstance(model, VisionTransformer):
                # a ViT checkpoint written by rounds 1-4 names patch_embed.{weight,bias} and blocks.N.fc{1,2}.*: load_pretrain renames the
                # MODEL's dict only, so without this the 50 renamed tensors kept the freshly loaded live weights as their average while the
                # moments and last_iter continued
                esd = legacy_vit_keys(esd)
            absent = [nm for nm in arena.names if nm not in esd]
            if absent:
                raise RuntimeError("resume: the checkpoint's 'ema' dict lacks %d of the model's %d parameters (first: %s); the average of "
                                   "those tensors cannot continue -- drop it with saver.pretrain.ignore.key: ['ema'] to restart the average "
                                   "from the loaded weights" % (len(absent), len(arena.names), absent[:3]))
            for nm, p_, o in zip(arena.names, arena.params, arena.offsets):
                tgt = opt.ema if use_hip_opt else ema
                tgt[o:o + p_.numel()].copy_(esd[nm].reshape(-1).to(tgt.device))
            for k in ema_buffers:
                if k in esd:
                    ema_buffers[k].copy_(esd[k].to(ema_buffers[k].device))
        if train_engine is not None:
            train_engine.repack()
    train.start_iter = start_iter

    def ema_state():
        sd = None
        if ema_on:
            if use_hip_opt:
                sd = opt.ema_state_dict(model)
            elif ema is not None:
                sd = {nm: ema[o:o + p_.numel()].view_as(p_).clone() for nm, p_, o in zip(arena.names, arena.params, arena.offsets)}
            if sd is not None:
                sd.update({k: v.clone() for k, v in ema_buffers.items()})
                for k, v in model.named_buffers():              # integer buffers (num_batches_tracked) are not averaged
                    if k not in sd:
                        sd[k] = v.detach().clone()
        return sd

    def save(step):
        if save_dir and rank == 0:
            ost = opt.state_dict() if use_hip_opt else {'torch': opt.state_dict()}
            name = 'ckpt_%d.pth.tar' % step if scfg.get('save_many', False) and step != max_iter else 'ckpt.pth.tar'
            save_checkpoint(os.path.join(save_dir, name), model, ema_state(), ost, step,
                            legacy_vit_keys=bool(scfg.get('legacy_vit_keys', False)))

    for it in range(start_iter, max_iter):
        lr = cosine_lr(it, max_iter, base_lr, warmup_lr, warmup_steps, min_lr)
        sel, epoch = sampler.batch(it)
        items = sel
        imgs, labels = ds.batch(sel, device, epoch) if isinstance(ds, FileImageNet) else ds.batch(sel, device)
        plan = mixing.draw_mix(mixup_alpha, cutmix_alpha, int(dcfg.get('seed', 0)), it, rank, len(sel), imgs.shape[1], imgs.shape[2]) \
            if mix_on else None
        if plan is None:
            x01 = imgs.permute(0, 3, 1, 2).float().div(255.0)
        else:
            # Mixup or CutMix of the batch with its permuted self (one of the two per iteration): on the HIP path one launch that fuses the
            # u8 -> [0, 1] hand-over, in torch on the scaffold; the partner labels follow the same permutation, uploaded once
            mix_lam = plan[1]
            perm_dev = mixing.upload_perm(plan, len(sel), device)
            x01 = mixing.apply_mix(imgs, plan, device, perm_dev=perm_dev) if use_hip_opt else mixing.apply_mix_torch(imgs, plan)
            labels_b = labels[perm_dev.long()]
        if adv and device.type == 'cuda':
            # inner maximisation on the HIP eval engine with the CURRENT weights, BN in inference mode: the engine is
            # built once and re-folded on the GPU from the live parameters / running statistics every iteration
            from ..model.engine import EngineModel
            from ..noise import adv as A
            if attack_model is None:
                model.eval()
                attack_model = EngineModel(model, takes_normalized=False)
            else:
                attack_model.rart_refold(model)
            x01 = A.pgd_linf(x01.contiguous(), labels, attack_model, parse_eps(adv['eps']),
                             float(adv.get('rel_stepsize', 3 / 40)), int(adv.get('steps', 3)), seed=it,
                             # every row draws its random start at ITS dataset index (sel is a strided slice of the epoch's
                             # permutation, not a contiguous range): no two images of an iteration share a field, and the
                             # draws do not depend on the world size
                             sample_offset=sampler.batch_rows(it, device))
        model.train()
        if train_engine is not None:
            # train-mode forward (batch statistics), label-smoothed CE, backward to every parameter: all HIP
            logits = train_engine.forward(x01.contiguous(), False, IMAGENET_MEAN, IMAGENET_STD)
            if plan is None:
                loss_rows, dlogits = label_smooth_ce(logits, labels, ls, 1.0 / len(items))
            else:
                loss_rows, dlogits = label_smooth_ce_mix(logits, labels, labels_b, mix_lam, ls, 1.0 / len(items))
            train_engine.backward(dlogits)                  # gradients land in the arena; buckets reduce as they fill
            loss = loss_rows.mean()
        else:
            xin = ((x01 - mean) / std).contiguous(memory_format=torch.channels_last)
            with torch.autocast('cuda', dtype=torch.bfloat16, enabled=use_amp):
                out = model(xin)
            if use_hip_opt:
                # label-smoothed CE and its gradient in one HIP kernel; autograd continues from dlogits
                if plan is None:
                    loss_rows, dlogits = label_smooth_ce(out, labels, ls, 1.0 / len(items))
                else:
                    loss_rows, dlogits = label_smooth_ce_mix(out, labels, labels_b, mix_lam, ls, 1.0 / len(items))
                out.backward(dlogits.to(out.dtype))         # bucket all-reduces start from the grad hooks
                loss = loss_rows.mean()
            elif plan is None:
                loss = F.cross_entropy(out.float(), labels, label_smoothing=ls)
                loss.backward()
            else:
                loss = mix_lam * F.cross_entropy(out.float(), labels, label_smoothing=ls) + \
                    (1.0 - mix_lam) * F.cross_entropy(out.float(), labels_b, label_smoothing=ls)
                loss.backward()
        scale = arena.finish_grad_exchange()                # waits for the buckets; returns 1 / world_size
        if use_hip_opt:
            opt.lr = lr
            opt.step(grad_scale=scale)                      # update + EMA + grad reset, one launch per decay range
            if train_engine is not None:
                train_engine.repack()                       # fp32 master weights -> bf16 igemm tables
        else:
            for gp in opt.param_groups:
                gp['lr'] = lr
            if scale != 1.0:
                arena.flat_g.mul_(scale)
            opt.step()
            arena.flat_g.zero_()
            if ema is not None:
                ema.mul_(decay).add_(arena.flat_p, alpha=1 - decay)
        if ema_buffers:
            with torch.no_grad():
                for k, v in model.named_buffers():
                    if k in ema_buffers:
                        ema_buffers[k].mul_(decay).add_(v.detach(), alpha=1 - decay)
        loss_v = float(loss.detach())
        if it % int(scfg.get('print_freq', 10)) == 0 or it == max_iter - 1:
            xs = arena.exchange_stats()
            if xs is not None:
                # every rank, on stderr: the gradient exchange of this step -- buckets, bytes, how many all-reduces started during backward,
                # and how long the compute stream stalled behind them (a first N-rank run is debugged from these lines)
                print('[cls_solver rank %d] %s' % (rank, json.dumps(dict(iter=it, grad_exchange=xs))), file=sys.stderr, flush=True)
            if rank == 0:
                rec = {'iter': it, 'loss': loss_v, 'lr': lr}
                if plan is not None:
                    rec['mix'] = {'kind': plan[0], 'lam': mix_lam}
                if xs is not None:
                    rec['grad_exchange'] = {k: xs[k] for k in ('buckets', 'bytes', 'launched_during_backward', 'stream_wait_s', 'host_wait_s') if k in xs}
                print(json.dumps(rec))
        if save_freq and (it + 1) % save_freq == 0 and it + 1 < max_iter:
            save(it + 1)                                     # an interrupted run resumes from here with --recover
    # checkpoint (rank 0): model, EMA (parameters from the optimizer's arena + the EMA'd buffers), optimizer, last iteration
    train.last_ema_state = ema_state()
    save(max_iter)
    return loss_v, model


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', required=True)
    ap.add_argument('--evaluate', action='store_true')
    ap.add_argument('--attack', default=None)
    ap.add_argument('--eps', default='8/255')
    ap.add_argument('--steps', type=int, default=0)
    ap.add_argument('--corruption', default=None)
    ap.add_argument('--severity', type=int, default=3)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--engine', choices=['hip', 'torch'], default='hip')
    ap.add_argument('--precision', choices=['bf16', 'bf16x3', 'fp32x'], default=None,
                    help="evaluation engine arithmetic: bf16 (default) or the reference-precision mode 'fp32x' (= 'bf16x3')")
    ap.add_argument('--max-iter', type=int, default=20)
    ap.add_argument('--train-engine', choices=['hip', 'torch'], default='hip', dest='train_engine',
                    help='train-mode forward/backward: hip = the HIP train engine of the model (ResNet50TrainEngine, ViTTrainEngine, '
                         'ConvNeXtTrainEngine, MixerTrainEngine), torch = autograd scaffold (ResNet-50 / ViT only)')
    ap.add_argument('--recover', default=None, help='checkpoint to start from (overrides saver.pretrain.path)')
    ap.add_argument('--ckpt-dir', default=None, dest='ckpt_dir', help='write <dir>/ckpt.pth.tar at the end of training')
    ap.add_argument('--save-dir', default=None, help='root of <model>/<noise>_<eps>/results.txt.all (robustart_amd.metrics)')
    ap.add_argument('--src_name', default=None, help='name of the attacked (source) model in the result path')
    ap.add_argument('--tgt_name', default=None, help='transfer: name of the target model (new_transfer/eval.sh:42-44)')
    ap.add_argument('--tgt-type', default=None, help='transfer: model.type of the target model; adversarial examples '
                    'are crafted on cfg.model and scored on this one')
    ap.add_argument('--imagenet-s', action='store_true', dest='imagenet_s',
                    help='with --evaluate: the ImageNet-S loop (exp/imagenet_s_loop): one pass per (decoder, resize operator) pair')
    ap.add_argument('--imagenet-s-ops', default=None, dest='imagenet_s_ops',
                    help='comma-separated resize operators of --imagenet-s (default: the six pil-* then the five opencv-*)')
    ap.add_argument('--imagenet-c', action='store_true', dest='imagenet_c',
                    help='with --evaluate: the ImageNet-C loop (exp/imagenet_c_loop_mini): every corruption at every severity in one '
                         'pass over the test set')
    ap.add_argument('--imagenet-c-names', default=None, dest='imagenet_c_names',
                    help="comma-separated corruptions of --imagenet-c (default: the 15 standard ones; 'all' adds the four extras)")
    ap.add_argument('--imagenet-c-severities', default=None, dest='imagenet_c_severities',
                    help='comma-separated severities of --imagenet-c (default: 1,2,3,4,5)')
    ap.add_argument('--imagenet-c-frost-dir', default=None, dest='imagenet_c_frost_dir',
                    help='folder of frost photographs, read in sorted order (also data.test.imagenet_c_frost_dir); without it the '
                         'default list leaves frost out')
    ap.add_argument('--imagenet-c-scores', action='store_true', dest='imagenet_c_scores',
                    help='with --imagenet-c and --save-dir: write the full score lines instead of the compact rank lines')
    args = ap.parse_args(argv)
    if args.imagenet_c:
        if not args.evaluate:
            raise ValueError('--imagenet-c is an evaluation loop: pass --evaluate')
        imagenet_c_names(args.imagenet_c_names)       # an unknown name or severity fails before the config is read
        imagenet_c_severities(args.imagenet_c_severities)
    if args.imagenet_s:
        imagenet_s_ops(args.imagenet_s_ops)           # an unknown name fails before anything is built
        if not args.evaluate:
            raise ValueError('--imagenet-s is an evaluation loop: pass --evaluate')
    cfg = load_config(args.config)
    rank, world, device = init_dist()
    try:
        if args.evaluate:
            return evaluate(cfg, args, rank, world, device)
        return train(cfg, args, rank, world, device)[0]
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


if __name__ == '__main__':
    main()
