"""Model zoo entry point -- mirrors RobustART/model/__init__.py:1 (`get_model`).

Five architectures and two stem variants: `resnet50_official` (forward + backward-to-input HIP engine: engine.py), `vit_base` / `vit_b16_224`
(forward + backward-to-input HIP engine: vit_engine.py), `convnext_base` (forward + backward-to-input HIP engine:
convnext_engine.py; train engine: convnext_train_engine.py, drop_path_rate 0 only) and `convnextv2_base` (ConvNeXt-V2-B: forward +
backward-to-input on the same engine with the GRN kernels; train engine: the same ConvNeXtTrainEngine, bf16, drop_path_rate 0 only)
and `mixer_b16_224` (MLP-Mixer-B/16: forward + backward-to-input HIP engine: mixer_engine.py; train engine: MixerTrainEngine,
mixer_train_engine.py, bf16, drop rates 0 only).
`convnext_base_cvst` and `vit_base_cvst` / `vit_b16_224_cvst` are the ConvStem variants of ConvNeXt-B and ViT-B/16 (convstem_torch.py:
the stem / patch embedding is a chain of 3x3 stride-2 convolutions, each followed by LayerNorm and GELU): forward + backward-to-input on
the same two engines, the stem on the chain of convstem_engine.py; evaluation only, `cls_solver` refuses to train them.
The Bottleneck family of `resnet50_official` runs on the same engine (engine.py, one launch chain): `resnet101_official`,
`resnet152_official`, `wide_resnet50_2`, `wide_resnet101_2` (ungrouped: the fused kernels that accept their shapes, else the generic
launches) and `resnext50_32x4d`, `resnext101_32x8d` (conv2 is a grouped 3x3: csrc/conv_grouped.hip); evaluation only, `cls_solver`
refuses to train them.
`densenet121`, `densenet169`, `densenet201` (densenet_torch.py: the public torchvision definition) run on DenseNetEngine
(densenet_engine.py: the pre-activation and dense-concatenation kernels of csrc/densenet.hip around the shared GEMM entries), forward +
backward-to-input in both precisions; evaluation only, `cls_solver` refuses to train them.
`resnet18_official`, `resnet34_official` (resnet_basic_torch.py: the BasicBlock members of the ResNet family, torchvision's keys) run on
BasicResNetEngine (basic_resnet_engine.py: ResNet-50's stem, head and convolution launchers; in bf16 an identity block of layer1 /
layer2 is one launch of csrc/basic_block.hip where `basic_block_widths` lists its width), forward + backward-to-input in both
precisions; evaluation only, `cls_solver` refuses to train them.  The bare names `resnet18` / `resnet34` are not registered.
kwargs `num_classes` and `drop_path_rate` are accepted (drop path is identity in eval)."""
from .resnet_torch import resnet50, FAMILY as _RESNET_FAMILY
from .vit_torch import vit_base
from .convnext_torch import convnext_base, convnextv2_base
from .mixer_torch import mixer_b16_224
from .convstem_torch import convnext_base_cvst, vit_base_cvst
from .densenet_torch import FAMILY as _DENSENET_FAMILY
from .resnet_basic_torch import BASIC_FAMILY as _BASIC_FAMILY

_REGISTRY = {'resnet50_official': resnet50, 'resnet50': resnet50, 'vit_base': vit_base, 'vit_b16_224': vit_base,
             'vit_base_patch16_224': vit_base, 'convnext_base': convnext_base,
             'convnextv2_base': convnextv2_base, 'mixer_b16_224': mixer_b16_224, 'convnext_base_cvst': convnext_base_cvst,
             'vit_base_cvst': vit_base_cvst, 'vit_b16_224_cvst': vit_base_cvst}
_REGISTRY.update(_RESNET_FAMILY)
_REGISTRY.update(_DENSENET_FAMILY)
_REGISTRY.update(_BASIC_FAMILY)          # (the bare names `resnet18` / `resnet34` stay unregistered)


def get_model(config):
    """config: mapping with `type` and optional `kwargs` (the YAML `model:` block,
    exprs/nips_benchmark/pgd_adv_train/resnet50/config.yaml:1-6)."""
    mtype = config['type'] if isinstance(config, dict) else config.type
    kwargs = dict((config.get('kwargs') if isinstance(config, dict) else getattr(config, 'kwargs', None)) or {})
    kwargs.pop('bn', None)          # {use_sync_bn: False}: BN statistics are local
    if mtype not in _REGISTRY:
        raise NotImplementedError('model type %r is outside the hot-path scope (the ResNet Bottleneck family / ViT-B/16 / ConvNeXt-B / ConvNeXt-V2-B / MLP-Mixer-B/16 / DenseNet-121/169/201 / ResNet-18/34 as resnet18_official, resnet34_official only)' % mtype)
    return _REGISTRY[mtype](**kwargs)
