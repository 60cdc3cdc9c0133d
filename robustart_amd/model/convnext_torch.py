"""ConvNeXt-B as a plain torch module (parameter container + fp32 reference for the HIP engine, convnext_engine.py).

Reference: config type `convnext_base` (exprs/exp/imagenet_c_loop_mini/config_convnext_base.yaml,
exprs/nips_benchmark/{new,pgd}_adv_train/convnext_base/config.yaml) loads timm's convnext_base: depths [3, 3, 27, 3], widths
[128, 256, 512, 1024]; stem = 4x4 stride-4 conv + channels-last LayerNorm; before stages 1-3 a LayerNorm then a 2x2 stride-2 conv;
block = 7x7 depthwise conv (bias, padding 3) -> LayerNorm (eps 1e-6) -> fc1 (C -> 4C) -> exact GELU -> fc2 (4C -> C) -> layer scale
`gamma` -> residual add; head = global average pool -> LayerNorm -> fc.  timm is not imported; the architecture is restated.

The module tree carries timm's parameter NAMES (`stem.{0,1}.*`, `stages.i.downsample.{0,1}.*`, `stages.i.blocks.j.{conv_dw, norm,
mlp.fc1, mlp.fc2}.*`, `stages.i.blocks.j.gamma`, `head.{norm,fc}.*`), so a timm checkpoint loads with strict=True."""
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
    def __init__(self, cin, cout, depth, dpr):
        super().__init__()
        self.downsample = nn.Sequential(LayerNorm2d(cin, eps=1e-6), nn.Conv2d(cin, cout, 2, stride=2)) if cin != cout else nn.Identity()
        self.blocks = nn.Sequential(*[Block(cout, dpr[j]) for j in range(depth)])

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
    def __init__(self, depths=(3, 3, 27, 3), dims=(128, 256, 512, 1024), num_classes=1000, drop_path_rate=0.0, **_):
        super().__init__()
        self.depths, self.dims = tuple(depths), tuple(dims)
        self.stem = nn.Sequential(nn.Conv2d(3, dims[0], 4, stride=4), LayerNorm2d(dims[0], eps=1e-6))
        total = sum(depths)
        rates = [drop_path_rate * i / max(total - 1, 1) for i in range(total)]
        stages, k, cin = [], 0, dims[0]
        for d, c in zip(depths, dims):
            stages.append(Stage(cin, c, d, rates[k:k + d]))
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
