"""ConvNeXt-B and ConvNeXt-V2-B as plain torch modules (parameter container + fp32 reference for the HIP engine, convnext_engine.py).

Reference: config type `convnext_base` (exprs/exp/imagenet_c_loop_mini/config_convnext_base.yaml,
exprs/nips_benchmark/{new,pgd}_adv_train/convnext_base/config.yaml) loads timm's convnext_base: depths [3, 3, 27, 3], widths
[128, 256, 512, 1024]; stem = 4x4 stride-4 conv + channels-last LayerNorm; before stages 1-3 a LayerNorm then a 2x2 stride-2 conv;
block = 7x7 depthwise conv (bias, padding 3) -> LayerNorm (eps 1e-6) -> fc1 (C -> 4C) -> exact GELU -> fc2 (4C -> C) -> layer scale
`gamma` -> residual add; head = global average pool -> LayerNorm -> fc.  timm is not imported; the architecture is restated.
ConvNeXt-V2 (`convnextv2_base`, class ConvNeXtV2 at the end of this file) differs in the block only.

The module tree carries timm's parameter NAMES (`stem.{0,1}.*`, `stages.i.downsample.{0,1}.*`, `stages.i.blocks.j.{conv_dw, norm,
mlp.fc1, mlp.fc2}.*`, `stages.i.blocks.j.gamma`, `head.{norm,fc}.*`), so a timm checkpoint loads with strict=True."""
import re

import torch
import torch.nn as nn
import torch.nn.functional as F


class LayerNorm2d(nn.LayerNorm):
    """LayerNorm over the channels of an NCHW tensor (timm's LayerNorm2d)"""

    def forward(self, x):
        return F.layer_norm(x.permute(0, 2, 3, 1), self.normalized_shape, self.weight, self.bias, self.eps).permute(0, 3, 1, 2)


class Mlp(nn.Module):
    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden)
        self.fc2 = nn.Linear(hidden, dim)

    def forward(self, x):
        return self.fc2(F.gelu(self.fc1(x)))


class Block(nn.Module):
    def __init__(self, dim, drop_path=0.0, ls_init_value=1e-6):
        super().__init__()
        self.conv_dw = nn.Conv2d(dim, dim, 7, padding=3, groups=dim)
        self.norm = nn.LayerNorm(dim, eps=1e-6)
        self.mlp = Mlp(dim, 4 * dim)
        self.gamma = nn.Parameter(ls_init_value * torch.ones(dim))
        self.drop_path = drop_path

    def forward(self, x):
        y = self.conv_dw(x).permute(0, 2, 3, 1)
        y = self.mlp(self.norm(y)) * self.gamma
        y = y.permute(0, 3, 1, 2)
        if self.training and self.drop_path > 0.0:          # stochastic depth; identity in eval
            keep = 1.0 - self.drop_path
            y = y * x.new_empty(x.shape[0], 1, 1, 1).bernoulli_(keep) / keep
        return x + y


class Stage(nn.Module):
    def __init__(self, cin, cout, depth, dpr, block=Block):
        super().__init__()
        self.downsample = nn.Sequential(LayerNorm2d(cin, eps=1e-6), nn.Conv2d(cin, cout, 2, stride=2)) if cin != cout else nn.Identity()
        self.blocks = nn.Sequential(*[block(cout, dpr[j]) for j in range(depth)])

    def forward(self, x):
        return self.blocks(self.downsample(x))


class Head(nn.Module):
    def __init__(self, dim, num_classes):
        super().__init__()
        self.norm = nn.LayerNorm(dim, eps=1e-6)
        self.fc = nn.Linear(dim, num_classes)

    def forward(self, x):
        return self.fc(self.norm(x.mean((2, 3))))


class ConvNeXt(nn.Module):
    block = Block

    def __init__(self, depths=(3, 3, 27, 3), dims=(128, 256, 512, 1024), num_classes=1000, drop_path_rate=0.0, **_):
        super().__init__()
        self.depths, self.dims = tuple(depths), tuple(dims)
        self.stem = nn.Sequential(nn.Conv2d(3, dims[0], 4, stride=4), LayerNorm2d(dims[0], eps=1e-6))
        total = sum(depths)
        rates = [drop_path_rate * i / max(total - 1, 1) for i in range(total)]
        stages, k, cin = [], 0, dims[0]
        for d, c in zip(depths, dims):
            stages.append(Stage(cin, c, d, rates[k:k + d], self.block))
            k += d
            cin = c
        self.stages = nn.Sequential(*stages)
        self.head = Head(dims[-1], num_classes)
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.Linear)):
                nn.init.trunc_normal_(m.weight, std=.02)
                nn.init.zeros_(m.bias)

    def forward(self, x):
        return self.head(self.stages(self.stem(x)))


def convnext_base(num_classes=1000, drop_path_rate=0.0, **kw):
    kw.pop('drop_path', None)
    kw.pop('pretrained', None)
    return ConvNeXt(num_classes=num_classes, drop_path_rate=drop_path_rate, **kw)


# ---------------------------------------------------------------------------------------------------------------- ConvNeXt-V2
# timm's convnextv2_base: ConvNeXt(depths=(3, 3, 27, 3), dims=(128, 256, 512, 1024), use_grn=True, ls_init_value=None) -- the V1 network
# with two changes inside the block: a Global Response Norm between the GELU and fc2 (GlobalResponseNormMlp: `mlp.fc1`, `mlp.grn`,
# `mlp.fc2`), and no layer scale (no `gamma`).  Reference configs: exprs/exp/{imagenet_c_loop_mini,imagenet-p-loop-mini,imagenet_s_loop,
# imagenet-a_o-loop}/config_convnextv2_base.yaml, exprs/nips_benchmark/{pgd_adv_train,new_adv_train}/convnextv2/config.yaml.

class GlobalResponseNorm(nn.Module):
    """GRN over a channels-last [n][h][w][c] tensor: G = ||x||_2 over (h, w), N = G / (mean_c G + eps), x + (b + w * (x * N)).
    timm initialises weight and bias to zero (GRN is then the identity)."""

    def __init__(self, dim, eps=1e-6):
        super().__init__()
        self.eps = eps
        self.weight = nn.Parameter(torch.zeros(dim))
        self.bias = nn.Parameter(torch.zeros(dim))

    def forward(self, x):
        g = x.norm(p=2, dim=(1, 2), keepdim=True)
        n = g / (g.mean(dim=-1, keepdim=True) + self.eps)
        return x + torch.addcmul(self.bias, self.weight, x * n)


class GrnMlp(nn.Module):
    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden)
        self.grn = GlobalResponseNorm(hidden)
        self.fc2 = nn.Linear(hidden, dim)

    def forward(self, x):
        return self.fc2(self.grn(F.gelu(self.fc1(x))))


class BlockV2(nn.Module):
    def __init__(self, dim, drop_path=0.0):
        super().__init__()
        self.conv_dw = nn.Conv2d(dim, dim, 7, padding=3, groups=dim)
        self.norm = nn.LayerNorm(dim, eps=1e-6)
        self.mlp = GrnMlp(dim, 4 * dim)
        self.drop_path = drop_path

    def forward(self, x):
        y = self.mlp(self.norm(self.conv_dw(x).permute(0, 2, 3, 1))).permute(0, 3, 1, 2)
        if self.training and self.drop_path > 0.0:          # stochastic depth; identity in eval
            keep = 1.0 - self.drop_path
            y = y * x.new_empty(x.shape[0], 1, 1, 1).bernoulli_(keep) / keep
        return x + y


class ConvNeXtV2(ConvNeXt):
    """ConvNeXt-V2.  A subclass of ConvNeXt: stem, downsamples and head are V1's; `use_grn` tells the HIP engine the block kind."""
    block = BlockV2
    use_grn = True


def convnextv2_base(num_classes=1000, drop_path_rate=0.0, **kw):
    kw.pop('drop_path', None)
    kw.pop('pretrained', None)
    return ConvNeXtV2(num_classes=num_classes, drop_path_rate=drop_path_rate, **kw)


_V2_BLOCK_KEYS = (('dwconv.', 'conv_dw.'), ('pwconv1.', 'mlp.fc1.'), ('pwconv2.', 'mlp.fc2.'), ('grn.gamma', 'mlp.grn.weight'),
                  ('grn.beta', 'mlp.grn.bias'))


def official_v2_key(k):
    """one key of the ConvNeXt-V2 authors' checkpoint layout (convnextv2_base_1k_224_ema.pt: `downsample_layers.*`,
    `stages.i.j.{dwconv,norm,pwconv1,grn,pwconv2}`, top-level `norm`, `head`) -> timm's; a timm key is returned unchanged"""
    m = re.match(r'downsample_layers\.(\d+)\.(\d+)\.(.*)$', k)
    if m:
        i, j, rest = m.groups()
        return ('stem.%s.%s' % (j, rest)) if i == '0' else ('stages.%s.downsample.%s.%s' % (i, j, rest))
    m = re.match(r'stages\.(\d+)\.(\d+)\.(.*)$', k)
    if m:
        i, j, rest = m.groups()
        for a, b in _V2_BLOCK_KEYS:
            if rest.startswith(a):
                rest = b + rest[len(a):]
                break
        return 'stages.%s.blocks.%s.%s' % (i, j, rest)
    if k.startswith('norm.'):
        return 'head.' + k
    if k.startswith('head.') and not k.startswith(('head.fc.', 'head.norm.')):
        return 'head.fc.' + k[5:]
    return k


def official_v2_state_dict(sd):
    """a whole state dict in the authors' layout -> timm's; GRN's (1, 1, 1, C) gamma / beta become (C,).  A dict already in timm's
    layout (no `downsample_layers.` key) is returned as it is."""
    if not any(k.startswith('downsample_layers.') for k in sd):
        return sd
    out = {}
    for k, v in sd.items():
        t = official_v2_key(k)
        out[t] = v.reshape(v.shape[-1]) if '.grn.' in t and hasattr(v, 'reshape') else v
    return out
