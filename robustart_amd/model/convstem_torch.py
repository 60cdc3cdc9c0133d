"""The ConvStem ("CvSt") variants of ConvNeXt-B and ViT-B/16 from "Revisiting Adversarial Training for ImageNet" (Singh, Croce, Hein) as
plain torch modules (parameter containers + fp32 reference for the HIP engines; the stem chain: convstem_engine.py).

Reference: config types `convnext_base_cvst` and `vit_base_cvst` (exprs/exp/{imagenet_c_loop_mini,imagenet_s_loop,imagenet-p-loop-mini,
imagenet-a_o-loop}/config_{convnext,vit}_base_cvst.yaml; the model lists of exprs/nips_benchmark/{adv_eval,new_adv_eval,batch_eval_adv}/
eval.sh), evaluated on the published robust checkpoints convnext_b_cvst_robust.pt and vit_b_cvst_robust.pt.  Every reference config of
these types is evaluation only.

Both networks differ from `convnext_base` / `vit_base` in the stem alone.  The common unit CS(cin, cout) is
    Conv2d(cin, cout, 3, stride=2, padding=1, bias=True) -> LayerNorm over the channels of each pixel (eps 1e-6, affine) -> exact GELU.
  * ConvNeXt-B + ConvStem: the whole timm stem (4x4 stride-4 conv + LayerNorm) becomes CS(3, 64), CS(64, 128): 224 -> 112 -> 56, with no
    further LayerNorm before stage 0.  Parameters `stem.stem.{0,1,3,4}.*` (conv 1, LayerNorm 1, conv 2, LayerNorm 2; indices 2 and 5
    are the parameter-free GELUs); everything else carries timm's names as `convnext_base` does.
  * ViT-B/16 + ConvStem: `patch_embed.proj` becomes CS(3, 48), CS(48, 96), CS(96, 192), CS(192, 384), Conv2d(384, 768, 1): 224 -> 14,
    196 tokens.  Parameters `patch_embed.proj.stem.{0,1,3,4,6,7,9,10,12}.*`, 12 being the 1x1 projection; class token, position
    embedding, blocks and head are `vit_base`'s.

These widths and names are restated from the published code from memory.  The checkpoints are not on this machine.  If a real
checkpoint disagrees, only the constructor defaults below change: the engines read every dimension from the module."""
import torch.nn as nn

from .convnext_torch import ConvNeXt, LayerNorm2d
from .vit_torch import VisionTransformer


class ConvStem(nn.Module):
    """CS(in_chans, widths[0]), CS(widths[0], widths[1]), ... and, with `embed_dim`, a closing Conv2d(widths[-1], embed_dim, 1).  The
    layers sit in `self.stem`, an nn.Sequential (conv, norm, GELU per unit), which gives the checkpoints' parameter names."""

    def __init__(self, in_chans, widths, embed_dim=None):
        super().__init__()
        layers, cin = [], in_chans
        for c in widths:
            layers += [nn.Conv2d(cin, c, 3, stride=2, padding=1, bias=True), LayerNorm2d(c, eps=1e-6), nn.GELU()]
            cin = c
        if embed_dim is not None:
            layers.append(nn.Conv2d(cin, embed_dim, 1))
        self.stem = nn.Sequential(*layers)
        self.widths, self.embed_dim = tuple(widths), embed_dim

    @property
    def units(self):
        """[(conv, norm)] of the CS units, in order"""
        return [(self.stem[3 * i], self.stem[3 * i + 1]) for i in range(len(self.widths))]

    @property
    def proj(self):
        """the closing 1x1 convolution, or None"""
        return self.stem[3 * len(self.widths)] if self.embed_dim is not None else None

    def forward(self, x):
        return self.stem(x)


class ConvNeXtCvSt(ConvNeXt):
    """ConvNeXt with the ConvStem; `stem_widths[-1]` is the width of stage 0."""

    def __init__(self, stem_widths=(64, 128), **kw):
        super().__init__(**kw)
        if stem_widths[-1] != self.dims[0]:
            raise ValueError('the last ConvStem width %d must equal the width of stage 0, %d' % (stem_widths[-1], self.dims[0]))
        if len(stem_widths) != 2:
            raise ValueError('ConvNeXt stages start at 1/4 of the image: the ConvStem has two stride-2 units, got %d' % len(stem_widths))
        self.stem = ConvStem(3, stem_widths)
        for conv, _ in self.stem.units:
            nn.init.trunc_normal_(conv.weight, std=.02)
            nn.init.zeros_(conv.bias)


class VisionTransformerCvSt(VisionTransformer):
    """ViT whose patch embedding is a ConvStem: len(stem_widths) stride-2 units (2 ** len == patch_size) and a 1x1 projection."""

    def __init__(self, stem_widths=(48, 96, 192, 384), **kw):
        super().__init__(**kw)
        if 2 ** len(stem_widths) != self.patch_size:
            raise ValueError('%d stride-2 units do not make a patch of %d pixels' % (len(stem_widths), self.patch_size))
        self.patch_embed.proj = ConvStem(3, stem_widths, self.embed_dim)


def convnext_base_cvst(num_classes=1000, drop_path_rate=0.0, **kw):
    kw.pop('drop_path', None)
    kw.pop('pretrained', None)
    return ConvNeXtCvSt(num_classes=num_classes, drop_path_rate=drop_path_rate, **kw)


def vit_base_cvst(num_classes=1000, **kw):
    kw.pop('drop_path_rate', None)
    kw.pop('drop_path', None)
    kw.pop('pretrained', None)
    return VisionTransformerCvSt(num_classes=num_classes, **kw)


def convstem_of(model):
    """the ConvStem of a ConvNeXt / ViT module, or None"""
    stem = model.stem if isinstance(model, ConvNeXt) else getattr(getattr(model, 'patch_embed', None), 'proj', None)
    return stem if isinstance(stem, ConvStem) else None
