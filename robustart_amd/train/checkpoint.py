"""Checkpoints of cls_solver: reading, writing, and building the model a run starts from together with the state a resumed run continues."""
import os

import torch


def load_checkpoint_file(path):
    """torch.load restricted to tensors / containers / numbers (weights_only=True): a checkpoint is data, and a pickle from
    an untrusted source would execute code.  Checkpoints of this solver and plain state dicts load this way; a legacy
    reference checkpoint that pickles other objects needs the explicit opt-in RART_ALLOW_PICKLE_CHECKPOINT=1."""
    import pickle
    try:
        return torch.load(path, map_location='cpu', weights_only=True)
    except (pickle.UnpicklingError, RuntimeError) as e:      # a missing / unreadable file (OSError) propagates as itself
        if os.environ.get('RART_ALLOW_PICKLE_CHECKPOINT') == '1':
            return torch.load(path, map_location='cpu', weights_only=False)
        raise RuntimeError('%s does not load with weights_only=True (%s); set RART_ALLOW_PICKLE_CHECKPOINT=1 to unpickle a '
                           'TRUSTED legacy checkpoint' % (path, e)) from e


def load_pretrain(model, path, prefer='model', strict=True, ignore_model=()):
    """`saver.pretrain.path` / --recover: load a checkpoint written by this solver or by the reference's
    (torch.save of {'model': state_dict, 'ema': {...}, ...} or a bare state_dict such as timm's
    jx_vit_base_p16_224-80ecf9dd.pth, exprs/nips_benchmark/new_adv_train/vit_base/config.yaml:78-79; DistributedDataParallel's
    'module.' prefix stripped).  prefer = 'ema' picks the EMA weights when the file has them.
    `ignore_model` = `saver.pretrain.ignore.model` (same file :80-87, exp/imagenet_c_loop_mini/config_vit_base.yaml:106-118): keys
    (with or without 'module.') popped from the checkpoint before loading -- fine-tuning with another number of classes; the
    model keeps its own initialisation for them and every OTHER key still has to match when strict.
    A ViT checkpoint in the key layout rounds 1-4 of this repository wrote (`patch_embed.weight`, `blocks.N.fc1.*`) is renamed to
    timm's layout, which the module tree now carries.  So is a ConvNeXt-V2 checkpoint in its authors' layout
    (convnextv2_base_1k_224_ema.pt: `downsample_layers.*`, `pwconv1`, `grn.gamma`, ...); `ignore_model` keys may then be given in
    either layout.  For EVERY model type, a leading `module.`, `model.` or `base_model.` that every key of the file carries is
    stripped, repeatedly (wrappers nest); no module of this package has a top-level attribute of those names.  That is what lets the
    ConvStem checkpoints convnext_b_cvst_robust.pt / vit_b_cvst_robust.pt load strictly into `convnext_base_cvst` / `vit_base_cvst`."""
    ck = load_checkpoint_file(path)
    sd = ck
    if isinstance(ck, dict):
        for key in ((prefer, 'model', 'state_dict', 'ema') if prefer else ('model', 'state_dict')):
            if key in ck and isinstance(ck[key], dict):
                sd = ck[key]
                break
    if isinstance(sd, dict) and 'ema_state_dict' in sd:          # reference EMA wrapper
        sd = sd['ema_state_dict']
    strip = lambda k: k[7:] if k.startswith('module.') else k    # noqa: E731
    sd = {strip(k): v for k, v in sd.items()}
    # a wrapper's prefix that EVERY key carries (any model type; the published ConvStem checkpoints: `module.`, `model.`, `base_model.`)
    wrapped = True
    while wrapped and sd:
        wrapped = False
        for pre in ('module.', 'model.', 'base_model.'):
            if all(k.startswith(pre) for k in sd):
                sd, wrapped = {k[len(pre):]: v for k, v in sd.items()}, True
    from ..model.vit_torch import VisionTransformer, legacy_vit_keys
    from ..model.convnext_torch import ConvNeXtV2, official_v2_key, official_v2_state_dict
    if isinstance(model, VisionTransformer):
        sd = legacy_vit_keys(sd)
    if isinstance(model, ConvNeXtV2):
        sd = official_v2_state_dict(sd)
    dropped = []
    for k in ignore_model or ():
        k = strip(str(k))
        if isinstance(model, VisionTransformer):
            k = next(iter(legacy_vit_keys({k: None})))
        if isinstance(model, ConvNeXtV2) and k not in sd:
            k = official_v2_key(k)
        if k in sd:
            del sd[k]
            dropped.append(k)
        else:
            raise KeyError('saver.pretrain.ignore.model: %r is not a key of %s' % (k, path))
    missing, unexpected = model.load_state_dict(sd, strict=False)
    missing = [k for k in missing if k not in dropped]
    if strict and (missing or unexpected):
        raise RuntimeError('load_pretrain(%s): missing keys %s, unexpected keys %s' % (path, list(missing), list(unexpected)))
    if missing or unexpected:
        import warnings
        warnings.warn('load_pretrain(%s): missing keys %s, unexpected keys %s' % (path, list(missing), list(unexpected)),
                      RuntimeWarning)
    load_pretrain.last_ignored = dropped
    return ck if isinstance(ck, dict) else {}


def save_checkpoint(path, model, ema_state=None, optimizer_state=None, step=0, extra=None, legacy_vit_keys=False):
    """The reference solver's checkpoint shape: {'model', 'ema', 'optimizer', 'last_iter'} (state dicts on the CPU).
    legacy_vit_keys (`saver.legacy_vit_keys: True`): write a ViT's parameters under the names rounds 1-4 of this repository used
    instead of timm's (for tools that read those files)."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    ren = (lambda d: d)
    if legacy_vit_keys:
        from ..model.vit_torch import timm_to_legacy_keys as ren
    ck = {'model': ren({k: v.detach().cpu() for k, v in model.state_dict().items()}), 'last_iter': int(step)}
    if ema_state is not None:
        ck['ema'] = ren({k: v.detach().cpu() for k, v in ema_state.items()})
    if optimizer_state is not None:
        ck['optimizer'] = optimizer_state
    if extra:
        ck.update(extra)
    torch.save(ck, path)
    return path


def build_model_and_resume(cfg, args=None):
    """get_model + `saver.pretrain.path` (or --recover) -> (the model with the weights an evaluation / fine-tuning run starts from, the resume
    state: the checkpoint's other entries -- 'optimizer', 'last_iter', 'ema', ... -- that the config does not ignore; {} without a file)."""
    from ..model import get_model
    model = get_model(cfg['model'])
    pre = (cfg.get('saver', {}) or {}).get('pretrain', {}) or {}
    path = getattr(args, 'recover', None) or pre.get('path')
    resume = {}
    if path:
        ck = load_pretrain(model, path, prefer='ema' if pre.get('use_ema', False) else 'model',
                           ignore_model=((pre.get('ignore') or {}).get('model')) or ())
        # `saver.pretrain.ignore.key: [optimizer, last_iter]` (pgd_adv_train/resnet50/config.yaml:67-70): fine-tuning from a
        # checkpoint instead of resuming it
        drop = set(((pre.get('ignore') or {}).get('key')) or [])
        resume = {k: v for k, v in ck.items() if k not in drop and k != 'model'}
    return model, resume


def build_model(cfg, args=None):
    """build_model_and_resume for the callers that only want the model."""
    return build_model_and_resume(cfg, args)[0]
