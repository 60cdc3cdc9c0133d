"""MLP-Mixer-B/16 as a plain torch module (parameter container + fp32 reference for the HIP engine).

Reference: config type `mixer_b16_224` (exprs/nips_benchmark/{pgd_adv_train,ema,augmentation,label_smooth}/mlp_mixer,
robust_baseline_exp/mlp_mixer) builds timm's `mixer_b16_224`: patch 16, width 768, 12 blocks, token-mixing MLP 196 -> 384 -> 196
and channel MLP 768 -> 3072 -> 768 (mlp_ratio (0.5, 4.0)), LayerNorm eps 1e-6, exact GELU, head on the token mean of the final
norm.  timm is not imported; the architecture is restated with timm's parameter NAMES (`stem.proj.*`,
`blocks.N.{norm1,mlp_tokens.fc1,mlp_tokens.fc2,norm2,mlp_channels.fc1,mlp_channels.fc2}.*`, `norm.*`, `head.*`: 150 keys,
59 880 472 parameters for B/16), so a timm checkpoint loads with strict=True.  Drop path is the identity in eval; the reference's
configs pass drop rates of 0."""
import torch.nn as nn
import torch.nn.functional as F


class Mlp(nn.Module):
    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden)
        self.fc2 = nn.Linear(hidden, dim)

    def forward(self, x):
        return self.fc2(F.gelu(self.fc1(x)))


class PatchEmbed(nn.Module):
    def __init__(self, in_chans, embed_dim, patch_size):
        super().__init__()
        self.proj = nn.Conv2d(in_chans, embed_dim, patch_size, stride=patch_size)

    def forward(self, x):
        return self.proj(x).flatten(2).transpose(1, 2)          # [B][tokens][D]


class MixerBlock(nn.Module):
    def __init__(self, dim, tokens, mlp_ratio=(0.5, 4.0)):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim, eps=1e-6)
        self.mlp_tokens = Mlp(tokens, int(mlp_ratio[0] * dim))
        self.norm2 = nn.LayerNorm(dim, eps=1e-6)
        self.mlp_channels = Mlp(dim, int(mlp_ratio[1] * dim))

    def forward(self, x):
        x = x + self.mlp_tokens(self.norm1(x).transpose(1, 2)).transpose(1, 2)
        return x + self.mlp_channels(self.norm2(x))


class MlpMixer(nn.Module):
    def __init__(self, num_classes=1000, img_size=224, patch_size=16, embed_dim=768, depth=12, mlp_ratio=(0.5, 4.0), **_):
        super().__init__()
        self.patch_size, self.embed_dim = patch_size, embed_dim
        self.num_tokens = (img_size // patch_size) ** 2
        self.stem = PatchEmbed(3, embed_dim, patch_size)
        self.blocks = nn.ModuleList([MixerBlock(embed_dim, self.num_tokens, mlp_ratio) for _ in range(depth)])
        self.norm = nn.LayerNorm(embed_dim, eps=1e-6)
        self.head = nn.Linear(embed_dim, num_classes)
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.xavier_uniform_(m.weight)
                nn.init.normal_(m.bias, std=1e-6)

    def forward(self, x):
        x = self.stem(x)
        for blk in self.blocks:
            x = blk(x)
        return self.head(self.norm(x).mean(1))


def mixer_b16_224(num_classes=1000, **kw):
    kw.pop('drop_path_rate', None)
    kw.pop('drop_path', None)
    return MlpMixer(num_classes=num_classes, **kw)
