"""ResNet-18 and ResNet-34 (the BasicBlock members of the ResNet family) as a plain torch module.

Role: the parameter container `get_model` returns for `resnet18_official` / `resnet34_official` (reference:
exprs/robust_baseline_exp/resnet/resnet18, .../resnet34, exprs/robust_baseline_exp/Test/resnet18; the model sources are absent, the
names mean the public torchvision definitions) and the plain-PyTorch reference BasicResNetEngine (basic_resnet_engine.py) is tested
against.  Module tree and state-dict keys are torchvision's: conv1, bn1, layerL.B.{conv1, bn1, conv2, bn2, downsample.0, downsample.1},
fc (512 -> classes).  Deliberately NOT a subclass of resnet_torch.ResNet: cls_solver picks the ResNet-50 train engine by
isinstance(model, ResNet), and these types are evaluation only.
"""
import torch
import torch.nn as nn


class BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 3, stride=stride, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(planes, planes, 3, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.downsample = downsample

    def forward(self, x):
        identity = x
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out))
        if self.downsample is not None:
            identity = self.downsample(x)
        return self.relu(out + identity)


class BasicResNet(nn.Module):
    def __init__(self, layers=(2, 2, 2, 2), num_classes=1000, width=64):
        super().__init__()
        self.inplanes = width
        self.conv1 = nn.Conv2d(3, width, 7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(width)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, stride=2, padding=1)
        self.layer1 = self._make_layer(width, layers[0])
        self.layer2 = self._make_layer(width * 2, layers[1], stride=2)
        self.layer3 = self._make_layer(width * 4, layers[2], stride=2)
        self.layer4 = self._make_layer(width * 8, layers[3], stride=2)
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.fc = nn.Linear(width * 8, num_classes)
        for m in self.modules():          # the initialisation of resnet_torch.ResNet
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.ones_(m.weight)
                nn.init.zeros_(m.bias)

    def _make_layer(self, planes, blocks, stride=1):
        downsample = None
        if stride != 1 or self.inplanes != planes:
            downsample = nn.Sequential(nn.Conv2d(self.inplanes, planes, 1, stride=stride, bias=False), nn.BatchNorm2d(planes))
        layers = [BasicBlock(self.inplanes, planes, stride, downsample)]
        self.inplanes = planes
        for _ in range(1, blocks):
            layers.append(BasicBlock(self.inplanes, planes))
        return nn.Sequential(*layers)

    def forward(self, x):
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        return self.fc(torch.flatten(self.avgpool(x), 1))


def _family(layers):
    def make(num_classes=1000, **_):
        return BasicResNet(layers, num_classes)
    return make


BASIC_LAYERS = {'resnet18_official': (2, 2, 2, 2), 'resnet34_official': (3, 4, 6, 3)}
# constructors that take num_classes and swallow other kwargs
BASIC_FAMILY = {name: _family(layers) for name, layers in BASIC_LAYERS.items()}
