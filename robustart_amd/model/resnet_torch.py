"""ResNet-50 (v1.5: stride on the 3x3) and the rest of its Bottleneck family (ResNet-101/152, Wide-ResNet-50/101-2,
ResNeXt-50 32x4d / -101 32x8d: `groups`, `width_per_group`) as a plain torch module.

Role: (1) the parameter container `get_model` returns (reference: RobustART/model/__init__.py:1 ->
prototype.model.get_model, whose source is absent; `resnet50_official` == the public torchvision
ResNet-50 v1.5 definition), (2) the plain-PyTorch fp32 reference the hand-written HIP
engine (robustart_amd/model/engine.py) is tested against, (3) the train-mode forward/backward
scaffold for cls_solver until the HIP wgrad kernels land.  torchvision is not installed here, so
the architecture is restated from its public description.
"""
import torch
import torch.nn as nn


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None, groups=1, width_per_group=64):
        super().__init__()
        mid = int(planes * width_per_group / 64) * groups       # ResNeXt / Wide-ResNet: the width of conv1's output and of the 3x3
        self.conv1 = nn.Conv2d(inplanes, mid, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(mid)
        self.conv2 = nn.Conv2d(mid, mid, 3, stride=stride, padding=1, groups=groups, bias=False)
        self.bn2 = nn.BatchNorm2d(mid)
        self.conv3 = nn.Conv2d(mid, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample

    def forward(self, x):
        identity = x
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        if self.downsample is not None:
            identity = self.downsample(x)
        return self.relu(out + identity)


class ResNet(nn.Module):
    def __init__(self, layers=(3, 4, 6, 3), num_classes=1000, width=64, groups=1, width_per_group=64):
        super().__init__()
        self.inplanes = width
        self.groups, self.width_per_group = groups, width_per_group
        self.conv1 = nn.Conv2d(3, width, 7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(width)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, stride=2, padding=1)
        self.layer1 = self._make_layer(width, layers[0])
        self.layer2 = self._make_layer(width * 2, layers[1], stride=2)
        self.layer3 = self._make_layer(width * 4, layers[2], stride=2)
        self.layer4 = self._make_layer(width * 8, layers[3], stride=2)
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.fc = nn.Linear(width * 8 * 4, num_classes)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.ones_(m.weight)
                nn.init.zeros_(m.bias)

    def _make_layer(self, planes, blocks, stride=1):
        downsample = None
        if stride != 1 or self.inplanes != planes * 4:
            downsample = nn.Sequential(nn.Conv2d(self.inplanes, planes * 4, 1, stride=stride, bias=False),
                                       nn.BatchNorm2d(planes * 4))
        kw = dict(groups=self.groups, width_per_group=self.width_per_group)
        layers = [Bottleneck(self.inplanes, planes, stride, downsample, **kw)]
        self.inplanes = planes * 4
        for _ in range(1, blocks):
            layers.append(Bottleneck(self.inplanes, planes, **kw))
        return nn.Sequential(*layers)

    def forward(self, x):
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        return self.fc(torch.flatten(self.avgpool(x), 1))


def resnet50(num_classes=1000, **_):
    return ResNet((3, 4, 6, 3), num_classes)


def _family(layers, groups=1, width_per_group=64):
    def make(num_classes=1000, **_):
        return ResNet(layers, num_classes, groups=groups, width_per_group=width_per_group)
    return make


# the other members of the Bottleneck family (public torchvision definitions: same module tree and state-dict keys as ResNet-50)
FAMILY = {'resnet101_official': _family((3, 4, 23, 3)), 'resnet152_official': _family((3, 8, 36, 3)),
          'wide_resnet50_2': _family((3, 4, 6, 3), 1, 128), 'wide_resnet101_2': _family((3, 4, 23, 3), 1, 128),
          'resnext50_32x4d': _family((3, 4, 6, 3), 32, 4), 'resnext101_32x8d': _family((3, 4, 23, 3), 32, 8)}


def randomize_bn_stats(model, seed=0):
    """Give eval-mode BN non-trivial running statistics / affine terms (random-init checkpoints have
    mean 0 / var 1, which would hide BN-folding bugs in the parity tests)."""
    g = torch.Generator().manual_seed(seed)
    for m in model.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.1)
            m.running_var.copy_(torch.rand(m.num_features, generator=g) * 0.5 + 0.75)
            m.weight.data.copy_(torch.rand(m.num_features, generator=g) * 0.5 + 0.75)
            m.bias.data.copy_(torch.randn(m.num_features, generator=g) * 0.1)
    return model
