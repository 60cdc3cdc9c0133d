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
import time

import torch
import torch.distributed as dist
import torch.nn.functional as F

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


def parse_eps(s):
    """'8/255' or '0.031' -> float (the launchers pass fractions, batch_eval_adv/eval.sh:9-10)."""
    if isinstance(s, (int, float)):
        return float(s)
    if '/' in s:
        a, b = s.split('/')
        return float(a) / float(b)
    return float(s)


def load_config(path):
    import yaml
    with open(path) as f:
        return yaml.safe_load(f)


class FakeImageNet(torch.utils.data.Dataset):
    """`data.read_from: fake` (pgd_adv_train/resnet50/config.yaml:37): synthetic uint8 NHWC images whose content
    is a pure function of the global index, so every world size sees the same dataset."""

    def __init__(self, n, size=224, classes=1000):
        self.n, self.size, self.classes = n, size, classes

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        img, lab = self.batch([i], 'cpu')
        return img[0], int(lab[0]), i

    def batch(self, indices, device):
        """(uint8 [b, size, size, 3], int64 [b]) generated ON `device` from the global indices alone: an integer
        hash of (index, element), identical on CPU and GPU and for every world size (no host loop, no H2D copy)."""
        idx = torch.as_tensor(list(indices), dtype=torch.int64, device=device).view(-1, 1)
        e = torch.arange(self.size * self.size * 3, dtype=torch.int64, device=device).view(1, -1)
        h = (idx * 1000003 + e) * 2654435761 % 4294967296
        h = (h ^ (h >> 15)) * 2246822519 % 4294967296
        h = h ^ (h >> 13)
        img = (h & 255).to(torch.uint8).view(-1, self.size, self.size, 3)
        lab = ((idx.view(-1) * 2654435761 % 4294967296) >> 7) % self.classes
        return img, lab


class StructuredFakeImageNet(FakeImageNet):
    """`data.read_from: structured`: a LEARNABLE synthetic set (still a pure function of the global index): class c of
    `classes` (default 16) owns a fixed +-1 pattern on an 8 x 8 x 3 grid; an image is 128 + contrast * pattern(upsampled)
    + the hash noise of FakeImageNet scaled to +-noise.  A network fitted to it has real decision margins, which is what
    the bf16-engine-vs-fp32 attack-outcome test needs (random-pixel images with hash labels can only be memorised)."""

    def __init__(self, n, size=224, classes=16, contrast=48.0, noise=40.0):
        super().__init__(n, size, classes)
        self.contrast, self.noise = float(contrast), float(noise)

    def batch(self, indices, device):
        raw, _ = super().batch(indices, device)
        idx = torch.as_tensor(list(indices), dtype=torch.int64, device=device)
        lab = ((idx * 2654435761 % 4294967296) >> 7) % self.classes
        cell = torch.arange(self.size, device=device) * 8 // self.size                      # pixel -> grid cell
        cy, cx, ch = cell.view(1, -1, 1, 1), cell.view(1, 1, -1, 1), torch.arange(3, device=device).view(1, 1, 1, 3)
        h = (lab.view(-1, 1, 1, 1) * 7919 + cy * 131 + cx * 17 + ch) * 2654435761 % 4294967296
        sign = (((h ^ (h >> 13)) >> 5) & 1).float() * 2.0 - 1.0
        img = 128.0 + self.contrast * sign + (raw.float() - 127.5) * (self.noise / 127.5)
        return img.clamp_(0, 255).to(torch.uint8), lab


def read_meta_file(path):
    """`data.{train,test}.meta_file`: one sample per line, either "relative/path.JPEG label" (the ImageNet lists of the
    reference configs, pgd_adv_train/resnet50/config.yaml:45,55) or a JSON object {"filename": ..., "label": ...} (the
    imagenet-c / imagenet-s lists, exp/imagenet_c_loop_mini/config_vit_base.yaml:82).  -> [(relpath, label)]"""
    out = []
    with open(path) as f:
        for ln in f:
            ln = ln.strip()
            if not ln:
                continue
            if ln.startswith('{'):
                o = json.loads(ln)
                out.append((o['filename'], int(o['label'])))
            else:
                name, lab = ln.rsplit(None, 1)
                out.append((name, int(lab)))
    return out


class _TransformName(str):
    """FileImageNet.transform: the transform's name ('ONECROP' / 'STANDARD', what configs and callers compare it with) that can also be
    called as the transform step, transform(decoded, indices, epoch) = FileImageNet.transform_batch."""

    def __new__(cls, name, owner):
        self = super().__new__(cls, name)
        self.owner = owner
        return self

    def __call__(self, decoded, indices, epoch=0):
        return self.owner.transform_batch(decoded, indices, epoch)


class FileImageNet(torch.utils.data.Dataset):
    """`data.read_from: fs` with `data.<split>.{root_dir, meta_file, image_reader.type: pil | hip, transforms}`
    (exp/imagenet_c_loop_mini/config_vit_base.yaml:80-104; `transforms` as the mapping {type: ...} or as a list of torchvision entries,
    read_transforms): files are decoded on the host by PIL (the reference's 'pil'
    reader) and the transform's arithmetic runs on the GPU:
      ONECROP  = Resize([test_resize, test_resize]) (PIL bilinear, what torchvision applies to a PIL image) + CenterCrop(
                 input_size) -> rart_resize_batch_u8 with the fused centre crop, bit-exact with Pillow;
      STANDARD = RandomResizedCrop(input_size) + RandomHorizontalFlip: the crop box / flip are drawn on the host from
                 (seed, global index) (a pure function of the sample, like every draw of this path), the resize runs in
                 the same kernel.  `flip=False` (a transform list without RandomHorizontalFlip) never flips.  `jitter` (the ranges of
                 a list's ColorJitter entry, train/jitter.py) is applied to the finished uint8 batch after the resize and the flip,
                 one rart_color_jitter_u8 call for the whole batch, bit-exact with Pillow; the mapping form carries no jitter.
    Output is the uint8 NHWC batch the corruption kernels and the engines' u8 entry consume; normalisation happens in
    the engine's input kernel.
    reader='hip' (`image_reader.type: hip`, opt-in) decodes a batch's baseline JPEGs through noise.imagenet_s.decode_batch_gpu --
    Huffman decoding on `num_workers` host threads, IDCT / upsampling / colour conversion on the GPU, bit-identical to the 'pil'
    reader -- and hands every other file to PIL as 'pil' does; `decode_stats` counts the files that took each path.
    entropy='gpu' (`image_reader.entropy: gpu`, opt-in, with reader='hip') moves the Huffman decoding to the GPU as well
    (decode_batch_gpu(entropy='gpu')): the same images, the same `decode_stats`.
    batch() = decode_indices() then transform(): a caller that scores one decoded batch under several transforms (the ImageNet-S loop)
    calls the two steps itself."""

    def __init__(self, root_dir, meta_file, size=224, test_resize=256, transform='ONECROP', reader='pil', limit=None, seed=0,
                 jitter=None, flip=True, num_workers=8, entropy='host'):
        if reader not in ('pil', 'hip'):
            raise NotImplementedError("image_reader.type %r: 'pil' and 'hip' are available in this build" % (reader,))
        if entropy not in ('host', 'gpu'):
            raise ValueError("image_reader.entropy %r: 'host' and 'gpu' are available" % (entropy,))
        self.reader, self.num_workers, self.entropy = reader, int(num_workers), entropy
        self.decode_stats = {'gpu': 0, 'fallback': 0}          # reader='hip': files decoded on the GPU / by PIL
        if transform not in ('ONECROP', 'STANDARD'):
            raise NotImplementedError('transforms.type %r (ONECROP / STANDARD)' % (transform,))
        self.root, self.items = root_dir, (read_meta_file(meta_file) if meta_file is not None else [])
        self.classes = None                 # from_folder: the sorted class-folder names, label = position
        if limit:
            self.items = self.items[:int(limit)]
        self.size, self.test_resize, self.transform, self.seed = int(size), int(test_resize), _TransformName(transform, self), int(seed)
        self.n = len(self.items)
        self.jitter, self.flip = jitter, bool(flip)

    @classmethod
    def from_folder(cls, root_dir, size=224, test_resize=256, transform='ONECROP', reader='pil', limit=None, seed=0, num_workers=8,
                    entropy='host'):
        """An image-folder set `<root>/<class folder>/<file>` (imagenet-a, imagenet-o and the in-distribution folder of
        exp/imagenet-a_o-loop): class folders sorted by name, files sorted by name inside each, label = the position of the folder --
        torchvision's ImageFolder order.  `classes` keeps the folder names.  Entries of the root that are not directories (ImageNet-A
        ships a README.txt) are skipped; decode, ONECROP and the resize are FileImageNet's."""
        if not os.path.isdir(root_dir):
            raise ValueError('image folder %r is not a directory' % (root_dir,))
        self = cls(root_dir, None, size, test_resize, transform, reader, None, seed, num_workers=num_workers, entropy=entropy)
        self.classes = sorted(d for d in os.listdir(root_dir) if os.path.isdir(os.path.join(root_dir, d)))
        for lab, d in enumerate(self.classes):
            for f in sorted(os.listdir(os.path.join(root_dir, d))):
                if os.path.isfile(os.path.join(root_dir, d, f)):
                    self.items.append((os.path.join(d, f), lab))
        if limit:
            self.items = self.items[:int(limit)]
        self.n = len(self.items)
        return self

    def __len__(self):
        return self.n

    def decode(self, i):
        """host side: (HxWx3 uint8 ndarray, label) of sample i"""
        from ..noise.imagenet_s import decode
        name, lab = self.items[i]
        return decode(os.path.join(self.root, name), 'pil'), lab

    def decode_batch(self, indices, dev):
        """reader='hip': the decoded images of `indices` as CUDA uint8 HxWx3 tensors (one decode_batch_gpu call)"""
        from ..noise.imagenet_s import decode_batch_gpu
        with torch.cuda.device(dev):
            images, used = decode_batch_gpu([os.path.join(self.root, self.items[i][0]) for i in indices], self.num_workers,
                                            entropy=self.entropy)
        self.decode_stats['gpu'] += sum(used)
        self.decode_stats['fallback'] += len(used) - sum(used)
        return images

    def __getitem__(self, i):
        img, lab = self.batch([i], 'cuda')
        return img[0], int(lab[0]), i

    def box(self, i, hw, epoch=0):
        """STANDARD: (y, x, h, w, flip) of sample i in `epoch`, drawn from (seed, epoch, i) with the reference's
        get_params loop: torchvision's RandomResizedCrop / RandomHorizontalFlip redraw every time a sample is visited,
        so the epoch is part of the key -- still a pure function of its arguments (resume-safe, world-size invariant)."""
        import random as _random
        from ..noise.imagenet_s import _train_params
        r = _random.Random((self.seed * 1000003 + i) * 1000033 + int(epoch))
        y, x, h, w = _train_params(hw, r)
        return y, x, h, w, r.random() < 0.5

    def decode_indices(self, indices, dev):
        """step 1 of batch(): the decoded images of `indices` as CUDA uint8 HxWx3 tensors on `dev` -- a Pillow loop plus uploads for
        reader='pil', one decode_batch_gpu call for reader='hip'"""
        dev = torch.device(dev)
        if dev.type != 'cuda':
            raise RuntimeError('FileImageNet: the resize / crop of the transform runs on the GPU (no CPU fallback)')
        if self.reader == 'hip':
            return self.decode_batch(indices, dev)
        return [torch.from_numpy(self.decode(i)[0]).to(dev, non_blocking=True) for i in indices]

    def transform_batch(self, decoded, indices, epoch=0):
        """step 2 of batch() (also reachable as self.transform(...)): the transform of the decoded images in ONE pil_resize_batch call (rart_resize_batch_u8: box, resize,
        centre crop and flip fused), then the jitter -> the uint8 (n, size, size, 3) batch"""
        from ..noise.imagenet_s import pil_resize_batch
        if self.transform == 'ONECROP':
            r, t = self.test_resize, self.size
            o = int(round((r - t) / 2.0))                             # torchvision CenterCrop
            out = pil_resize_batch(decoded, (r, r), 1, crop=(o, o, t, t))
        else:
            draws = [self.box(i, tuple(img.shape[:2]), epoch) for i, img in zip(indices, decoded)]
            out = pil_resize_batch(decoded, (self.size, self.size), 1, boxes=[d[:4] for d in draws],
                                   flips=[d[4] and self.flip for d in draws])
            if self.jitter is not None:
                from .jitter import apply_jitter, draw_jitter
                apply_jitter(out, [draw_jitter(self.jitter, self.seed, epoch, i) for i in indices])
        return out

    def batch(self, indices, device, epoch=0):
        dev = torch.device(device)
        out = self.transform_batch(self.decode_indices(indices, dev), indices, epoch)
        return out, torch.tensor([self.items[i][1] for i in indices], dtype=torch.int64, device=dev)


def _entry(e, where):
    """one entry of a transform list -> (type, kwargs)"""
    if isinstance(e, str):
        return e, {}
    if not isinstance(e, dict) or not isinstance(e.get('type'), str) or not isinstance(e.get('kwargs') or {}, dict):
        raise ValueError('%s: an entry must be a mapping {type: NAME, kwargs: {...}}, got %r' % (where, e))
    return e['type'], dict(e.get('kwargs') or {})


def _square(v, where):
    """`size: s` or `size: [s, s]` -> s; None when the two sides differ"""
    if isinstance(v, (list, tuple)):
        if len(v) == 1:
            v = [v[0], v[0]]
        if len(v) != 2 or any(isinstance(s, bool) or not isinstance(s, int) for s in v):
            raise ValueError('%s: size must be an int or a pair of ints, got %r' % (where, v))
        return int(v[0]) if v[0] == v[1] else None
    if isinstance(v, bool) or not isinstance(v, int):
        raise ValueError('%s: size must be an int or a pair of ints, got %r' % (where, v))
    return int(v)


_LIST_TYPES = ('RandomResizedCrop', 'RandomHorizontalFlip', 'ColorJitter', 'ToTensor', 'Normalize', 'Resize', 'CenterCrop')


def read_transforms(dcfg, split):
    """`data.<split>.transforms` in either form -> {'type': 'ONECROP' / 'STANDARD', 'test_resize': int, 'jitter': ranges or None,
    'flip': bool}, the arguments FileImageNet takes.
      mapping {type: T} (or absent):  T (default ONECROP for test, STANDARD otherwise), data.test_resize, no jitter, flip on.
      list, a split other than test (exp/imagenet_s_loop/config_convnext_base.yaml:61-77): RandomResizedCrop(size = data.input_size),
          [RandomHorizontalFlip], [ColorJitter(...)], ToTensor, Normalize -> STANDARD, the jitter ranges of train/jitter.py, flip only
          when the entry is there.
      list, the test split (same file :88-101): Resize([r, r]) or Resize(r), CenterCrop(data.input_size), ToTensor, Normalize
          -> ONECROP with test_resize = r.
    ToTensor + Normalize are the engines' input kernel, which applies the ImageNet constants: another mean / std, a non-square Resize
    and any entry type outside these raise NotImplementedError; an entry out of place or a size other than data.input_size, ValueError."""
    sec = dcfg.get(split) or {}
    tr = sec.get('transforms')
    size = int(dcfg.get('input_size', 224))
    train = split != 'test'                # as the mapping form's default reads the split
    where = 'data.%s.transforms' % split
    if not tr or isinstance(tr, dict):                 # absent, null or empty reads as the mapping form's defaults, as before
        return {'type': (tr or {}).get('type', 'STANDARD' if train else 'ONECROP'), 'test_resize': int(dcfg.get('test_resize', 256)),
                'jitter': None, 'flip': True}
    if not isinstance(tr, (list, tuple)):
        raise ValueError('%s: a mapping {type: ...} or a list of torchvision entries, got %r' % (where, tr))
    entries = [_entry(e, where) for e in tr]
    for t, _ in entries:
        if t not in _LIST_TYPES:
            raise NotImplementedError('%s: entry type %r is not available in this build (%s)' % (where, t, ', '.join(_LIST_TYPES)))
    names = [t for t, _ in entries]
    if names[-2:] != ['ToTensor', 'Normalize']:
        raise ValueError('%s: the list must end with ToTensor, Normalize, got %s' % (where, names))
    nk = entries[-1][1]
    mean, std = nk.get('mean', IMAGENET_MEAN), nk.get('std', IMAGENET_STD)
    if [float(v) for v in mean] != list(IMAGENET_MEAN) or [float(v) for v in std] != list(IMAGENET_STD):
        raise NotImplementedError('%s: Normalize mean %r std %r: the solver applies the ImageNet constants %r / %r only'
                                  % (where, mean, std, IMAGENET_MEAN, IMAGENET_STD))
    head = entries[:-2]
    out = {'type': 'STANDARD' if train else 'ONECROP', 'test_resize': int(dcfg.get('test_resize', 256)), 'jitter': None, 'flip': False}
    if train:
        if not head or head[0][0] != 'RandomResizedCrop':
            raise ValueError('%s: a train list must start with RandomResizedCrop, got %s' % (where, names))
        kw = head[0][1]
        if set(kw) - {'size'}:
            raise NotImplementedError('%s: RandomResizedCrop kwargs %s (only size; scale and ratio keep torchvision\'s defaults)'
                                      % (where, sorted(set(kw) - {'size'})))
        if _square(kw.get('size'), where + ' RandomResizedCrop') != size:
            raise ValueError('%s: RandomResizedCrop size %r must equal data.input_size %d' % (where, kw.get('size'), size))
        rest = head[1:]
        if rest and rest[0][0] == 'RandomHorizontalFlip':
            if float(rest[0][1].get('p', 0.5)) != 0.5 or set(rest[0][1]) - {'p'}:
                raise NotImplementedError('%s: RandomHorizontalFlip kwargs %r (only p = 0.5)' % (where, rest[0][1]))
            out['flip'] = True
            rest = rest[1:]
        if rest and rest[0][0] == 'ColorJitter':
            from .jitter import jitter_ranges
            out['jitter'] = jitter_ranges(rest[0][1])
            rest = rest[1:]
        if rest:
            raise ValueError('%s: %s is out of place: a train list is RandomResizedCrop, [RandomHorizontalFlip], [ColorJitter], ToTensor, '
                             'Normalize' % (where, rest[0][0]))
        return out
    if [t for t, _ in head] != ['Resize', 'CenterCrop']:
        raise ValueError('%s: a test list must be Resize, CenterCrop, ToTensor, Normalize, got %s' % (where, names))
    (_, rk), (_, ck) = head
    if set(rk) - {'size'} or set(ck) - {'size'}:
        raise NotImplementedError('%s: Resize / CenterCrop kwargs other than size (%s)' % (where, sorted((set(rk) | set(ck)) - {'size'})))
    r = _square(rk.get('size'), where + ' Resize')
    if r is None:
        raise NotImplementedError('%s: a non-square Resize %r (ONECROP resizes to [r, r])' % (where, rk.get('size')))
    if _square(ck.get('size'), where + ' CenterCrop') != size:
        raise ValueError('%s: CenterCrop size %r must equal data.input_size %d' % (where, ck.get('size'), size))
    if r < size:
        raise ValueError('%s: Resize %d is smaller than the CenterCrop %d' % (where, r, size))
    out.update(test_resize=r, flip=True)
    return out


def make_dataset(dcfg, n, size, split='test'):
    """`data.read_from`: 'fake' (the reference configs' own setting) / 'structured' -> synthetic sets of n samples;
    'fs' (or 'file' / 'folder') -> FileImageNet over data.<split>.{root_dir, meta_file} (n = limit, 0 / None = all)."""
    rf = dcfg.get('read_from', 'fake')
    if rf == 'structured':
        return StructuredFakeImageNet(n, size, int(dcfg.get('structured_classes', 16)),
                                      float(dcfg.get('structured_contrast', 48.0)), float(dcfg.get('structured_noise', 40.0)))
    if rf in ('fs', 'file', 'folder'):
        sec = dcfg.get(split) or {}
        if not sec.get('root_dir') or not sec.get('meta_file'):
            raise ValueError('data.read_from: %s needs data.%s.root_dir and data.%s.meta_file' % (rf, split, split))
        t = read_transforms(dcfg, split)
        return FileImageNet(sec['root_dir'], sec['meta_file'], size, t['test_resize'], t['type'],
                            (sec.get('image_reader') or {}).get('type', 'pil'), dcfg.get('limit_samples'),
                            int(dcfg.get('seed', 0)), jitter=t['jitter'], flip=t['flip'], num_workers=int(dcfg.get('num_workers') or 8),
                            entropy=(sec.get('image_reader') or {}).get('entropy', 'host'))
    if rf != 'fake':
        raise NotImplementedError("data.read_from %r ('fake', 'structured', 'fs')" % (rf,))
    return FakeImageNet(n, size)


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


def shard_indices(n, rank, world):
    """`sampler.type: distributed` (non-repeating): contiguous ranges, the last ranks may get one fewer."""
    per = (n + world - 1) // world
    return list(range(min(rank * per, n), min((rank + 1) * per, n)))


class EpochSampler:
    """`sampler.type: distributed_iteration` of the training configs (pgd_adv_train/resnet50/config.yaml:39-41): every
    epoch visits a fresh random permutation of the train set, dealt to the ranks by stride.  ImageNet's train list is
    sorted by class, so file-order batches from contiguous per-rank ranges would hold one class each (degenerate
    BatchNorm statistics and SGD).  The permutation is a pure function of (seed, epoch) -- numpy's RandomState stream --
    so a resumed run and every world size of the same global batch see the same samples; the tail of an epoch wraps to
    the permutation's head (DistributedSampler's padding), so every iteration has a full batch.
    shuffle=False keeps file order (still strided over the ranks)."""

    def __init__(self, n, batch_size, rank, world, seed=0, shuffle=True):
        self.n, self.bs, self.rank, self.world = int(n), int(batch_size), int(rank), int(world)
        self.seed, self.shuffle = int(seed), bool(shuffle)
        self.per_epoch = max(1, -(-self.n // (self.bs * self.world)))
        self._epoch, self._mine = None, None

    def epoch_of(self, it):
        return int(it) // self.per_epoch

    def _order(self, epoch):
        import numpy as np
        if self._epoch != epoch:
            if self.shuffle:
                perm = np.random.RandomState((self.seed * 1000003 + epoch) % (2 ** 32)).permutation(self.n)
            else:
                perm = np.arange(self.n)
            total = self.per_epoch * self.bs * self.world
            perm = np.resize(perm, total)                      # repeats from the head when total > n
            self._epoch, self._mine = epoch, perm[self.rank::self.world]
        return self._mine

    def batch(self, it):
        """-> (global indices of this rank's batch at iteration `it`, epoch)"""
        epoch = self.epoch_of(it)
        k = int(it) % self.per_epoch
        return [int(v) for v in self._order(epoch)[k * self.bs:(k + 1) * self.bs]], epoch

    def batch_rows(self, it, device):
        """The same indices as an int64 tensor on `device`, a VIEW of this rank's share of the epoch's permutation, which is uploaded ONCE per
        epoch (the attack kernels read it as every row's global sample index: round 5 built a tensor from a Python list per step).  The
        range [0, 2^32) the counter generator needs is checked here, on the host, once per epoch -- the attack entry does not look at a
        device tensor's values (that was a blocking device-to-host copy per iteration)."""
        import torch
        epoch = self.epoch_of(it)
        mine = self._order(epoch)
        if getattr(self, '_dev_epoch', None) != (epoch, str(device)):
            if len(mine) and (int(mine.min()) < 0 or int(mine.max()) >= 1 << 32):
                raise ValueError('sample indices must lie in [0, 2^32)')
            self._dev = torch.as_tensor(mine, dtype=torch.int64).to(device)
            self._dev_epoch = (epoch, str(device))
        k = int(it) % self.per_epoch
        return self._dev[k * self.bs:(k + 1) * self.bs]


def cosine_lr(step, total, base_lr, warmup_lr, warmup_steps, min_lr=0.0):
    """lr_scheduler.type CosineEpoch with linear warm-up (config.yaml:21-29)."""
    if step < warmup_steps:
        return base_lr + (warmup_lr - base_lr) * step / max(warmup_steps, 1)
    t = (step - warmup_steps) / max(total - warmup_steps, 1)
    return min_lr + 0.5 * (warmup_lr - min_lr) * (1 + math.cos(math.pi * t))


def topk_correct(logits, labels, ks=(1, 5)):
    _, pred = logits.topk(max(ks), dim=1)
    hit = pred.eq(labels.view(-1, 1))
    return [int(hit[:, :k].any(1).sum()) for k in ks]


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


def all_reduce_counters(values, device):
    """The eval path's only collective: sum of a few int64 counters."""
    t = torch.tensor(values, dtype=torch.int64, device=device)
    if dist.is_available() and dist.is_initialized():
        dist.all_reduce(t)
    return [int(v) for v in t.tolist()]


def build_model(cfg, args=None):
    """get_model + `saver.pretrain.path` (or --recover): the weights an evaluation / fine-tuning run starts from."""
    from ..model import get_model
    model = get_model(cfg['model'])
    pre = (cfg.get('saver', {}) or {}).get('pretrain', {}) or {}
    path = getattr(args, 'recover', None) or pre.get('path')
    build_model.last_checkpoint = None
    if path:
        ck = load_pretrain(model, path, prefer='ema' if pre.get('use_ema', False) else 'model',
                           ignore_model=((pre.get('ignore') or {}).get('model')) or ())
        # `saver.pretrain.ignore.key: [optimizer, last_iter]` (pgd_adv_train/resnet50/config.yaml:67-70): fine-tuning from a
        # checkpoint instead of resuming it
        drop = set(((pre.get('ignore') or {}).get('key')) or [])
        build_model.last_checkpoint = {k: v for k, v in ck.items() if k not in drop and k != 'model'}
    return model


def natural_mode(dcfg):
    """`data.test.imagenet_a&o: True` (exp/imagenet-a_o-loop/config_vit_base.yaml:79-84): the ImageNet-A / ImageNet-O evaluation."""
    return bool(((dcfg or {}).get('test') or {}).get('imagenet_a&o', False))


def read_class_map(tcfg, num_classes):
    """The model's class index -> wnid: the lines of `data.test.class_index_file` (one wnid per line, the line number is the class
    index) or, without that key, the sorted sub-directory names of `imagenet_val_root_dir` (the order an image-folder training set
    gives its classes).  The count must equal the model's num_classes."""
    path = tcfg.get('class_index_file')
    if path:
        with open(path) as f:
            names = [ln.strip() for ln in f if ln.strip()]
        src = 'data.test.class_index_file %s' % path
    else:
        root = tcfg.get('imagenet_val_root_dir')
        if not root or not os.path.isdir(root):
            raise ValueError('data.test: imagenet_a&o needs class_index_file or a directory imagenet_val_root_dir with one folder per '
                             'class, got %r' % (root,))
        names = sorted(d for d in os.listdir(root) if os.path.isdir(os.path.join(root, d)))
        src = 'data.test.imagenet_val_root_dir %s' % root
    if len(names) != int(num_classes):
        raise ValueError('%s names %d classes, the model has num_classes = %d' % (src, len(names), int(num_classes)))
    if len(set(names)) != len(names):
        raise ValueError('%s names a class twice' % src)
    return names


def subset_of(folder_names, class_map, what):
    """class indices of a folder set's class names, in folder order -> list of ints; a name the map lacks is a ValueError"""
    pos = {w: i for i, w in enumerate(class_map)}
    for w in folder_names:
        if w not in pos:
            raise ValueError('%s: class folder %r is not in the class map' % (what, w))
    return [pos[w] for w in folder_names]


def natural_datasets(cfg):
    """The config side of the ImageNet-A / -O evaluation, all of it on the host: the class map, the three folder sets and the two
    class subsets -> {'a': (dataset, indices), 'o_in': (dataset, indices), 'o_out': (dataset, indices)}."""
    dcfg = cfg.get('data', {})
    tcfg = dcfg.get('test') or {}
    num_classes = int(((cfg.get('model') or {}).get('kwargs') or {}).get('num_classes', 1000))
    class_map = read_class_map(tcfg, num_classes)
    t = read_transforms(dcfg, 'test')
    size = int(dcfg.get('input_size', 224))
    sets = {}
    for key, name in (('a', 'imagenet_a_root_dir'), ('o_out', 'imagenet_o_root_dir'), ('o_in', 'imagenet_o_folder')):
        if not tcfg.get(name):
            raise ValueError('data.test: imagenet_a&o needs data.test.%s' % name)
        sets[key] = FileImageNet.from_folder(tcfg[name], size, t['test_resize'], t['type'], (tcfg.get('image_reader') or {}).get('type', 'pil'),
                                             dcfg.get('limit_samples'), int(dcfg.get('seed', 0)), num_workers=int(dcfg.get('num_workers') or 8),
                                             entropy=(tcfg.get('image_reader') or {}).get('entropy', 'host'))
    if sets['o_in'].classes != sets['o_out'].classes:
        raise ValueError('data.test.imagenet_o_folder must hold exactly the class folders of imagenet_o_root_dir: %d vs %d folders, '
                         'differing in %s' % (len(sets['o_in'].classes), len(sets['o_out'].classes),
                                              sorted(set(sets['o_in'].classes) ^ set(sets['o_out'].classes))[:5]))
    sub_a = subset_of(sets['a'].classes, class_map, 'data.test.imagenet_a_root_dir')
    sub_o = subset_of(sets['o_out'].classes, class_map, 'data.test.imagenet_o_root_dir')
    for sub, name in ((sub_a, 'imagenet_a_root_dir'), (sub_o, 'imagenet_o_root_dir')):
        if sub != sorted(sub):
            # the label of a folder sample is the folder's position, the prediction the class's rank in the subset: they are the same
            # coordinate only when the class map orders the folders as their names do
            raise ValueError('data.test.%s: the class map does not keep the order of the class folders\' names' % name)
    return {'a': (sets['a'], sub_a), 'o_in': (sets['o_in'], sub_o), 'o_out': (sets['o_out'], sub_o)}


def evaluate_natural(cfg, args, rank, world, device, model=None):
    """`data.test.imagenet_a&o`: three passes over sharded indices -- ImageNet-A, the in-distribution set of ImageNet-O's classes, and
    ImageNet-O (out of distribution, no labels).  Per batch: engine logits -> rart_logit_confidence_f32 over the set's class subset ->
    ConfidenceWriter.  After the barrier rank 0 computes the metrics from the merged files, as the reference does."""
    if not getattr(args, 'save_dir', None):
        raise ValueError('data.test.imagenet_a&o needs --save-dir: the metrics are computed from the merged result files')
    if (getattr(args, 'attack', None) and args.attack != 'none') or getattr(args, 'corruption', None):
        raise ValueError('data.test.imagenet_a&o cannot be combined with --attack / --corruption: no config of imagenet-a_o-loop has noise')
    dcfg = cfg.get('data', {})
    bs = int(dcfg.get('batch_size', 64))
    plan = natural_datasets(cfg)
    if device.type != 'cuda':
        raise RuntimeError('data.test.imagenet_a&o runs on the GPU (the resize and the subset confidence are HIP kernels; no CPU fallback)')
    from ..metrics import (ConfidenceWriter, ImageNetAEvaluator, ImageNetOEvaluator, class_subset, result_dir, subset_confidence)
    model = model or build_model(cfg, args)
    model = model.to(device).eval()
    use_hip = args.engine == 'hip'
    if use_hip:
        from ..model.engine import EngineModel
        prec = getattr(args, 'precision', None) or cfg.get('engine_precision', 'bf16')
        f_model = EngineModel(model, takes_normalized=False, precision=prec)
    mean = torch.tensor(IMAGENET_MEAN, device=device).view(1, 3, 1, 1)
    std = torch.tensor(IMAGENET_STD, device=device).view(1, 3, 1, 1)
    num_classes = int(((cfg.get('model') or {}).get('kwargs') or {}).get('num_classes', 1000))
    name = getattr(args, 'src_name', None) or cfg['model']['type']
    barrier = dist.barrier if dist.is_available() and dist.is_initialized() else None
    t0 = time.time()
    paths, counts, subsets = {}, {}, {}
    for key, noise_name, labelled in (('a', 'imagenet_a', True), ('o_in', 'imagenet_o_in', True), ('o_out', 'imagenet_o_out', False)):
        ds, sub = plan[key]
        if tuple(sub) not in subsets:
            subsets[tuple(sub)] = class_subset(sub, num_classes, device)         # validated on the host, uploaded once
        sub_dev = subsets[tuple(sub)]
        writer = ConfidenceWriter(result_dir(args.save_dir, name, noise_name, '0'), rank, world)
        idx = shard_indices(len(ds), rank, world)
        for s in range(0, len(idx), bs):
            items = idx[s:s + bs]
            imgs, labels = ds.batch(items, device)
            if use_hip:
                logits = f_model.rart_engine.logits_from_u8(imgs, IMAGENET_MEAN, IMAGENET_STD)
            else:
                with torch.no_grad():
                    logits = model((imgs.permute(0, 3, 1, 2).float() / 255.0 - mean) / std)
            if logits.shape[1] != num_classes:
                raise ValueError('the model returns %d logits, model.kwargs.num_classes says %d' % (logits.shape[1], num_classes))
            pred, conf, correct = subset_confidence(logits.float(), sub_dev, labels if labelled else None)
            writer.write_batch(pred, conf, correct, [ds.items[i][1] for i in items] if labelled else None, items)
        paths[key] = writer.close(barrier=barrier)
        counts[key] = len(ds)
    res = None
    if rank == 0:
        ev_a, ev_o = ImageNetAEvaluator(), ImageNetOEvaluator()
        a = ev_a.eval(paths['a'])
        o = ev_o.eval(paths['o_in'], paths['o_out'])
        res = {'imagenet_a': dict(a, count=counts['a']),
               'imagenet_o': {'AUPR': o['AUPR'], 'AUROC': ev_o.last_measures['AUROC'], 'FPR95': ev_o.last_measures['FPR95'],
                              'count_in': counts['o_in'], 'count_out': counts['o_out']},
               'world_size': world, 'seconds': time.time() - t0}
        print(json.dumps(res))
    return res


def imagenet_s_ops(spec=None):
    """`--imagenet-s-ops a,b,...` -> the resize operators of the ImageNet-S loop, in order; None / '' -> the eleven names of
    PIL_FILTERS then CV_MODES.  An unknown or repeated name is a ValueError."""
    from ..noise.imagenet_s import CV_MODES, PIL_FILTERS
    known = list(PIL_FILTERS) + list(CV_MODES)
    if spec is None or not str(spec).strip():
        return known
    ops = [t.strip() for t in str(spec).split(',') if t.strip()]
    for t in ops:
        if t not in known:
            raise ValueError('--imagenet-s-ops: unknown resize operator %r (%s)' % (t, ', '.join(known)))
    if len(set(ops)) != len(ops) or not ops:
        raise ValueError('--imagenet-s-ops: every operator once, got %r' % (spec,))
    return ops


def evaluate_imagenet_s(cfg, args, rank, world, device, model=None):
    """`--evaluate --imagenet-s`: the loop of exp/imagenet_s_loop (eval.sh:23, multi_eval_decoder_resize_solver): one model scored on
    the test set once per (decoder, resize operator) pair; the accuracies, their mean and their spread.  Per batch of sharded
    indices the files are decoded ONCE (data.test.image_reader.type pil | hip) and every operator runs on the decoded batch through
    image_transfer_batch(transform_type='val', resize=data.input_size): the operator under test replaces the config's Resize, so
    only input_size is taken from the transform list (which still has to parse).  The decoder is 'pil' (the others are not in this
    build).  `data.test.save_acc_var_neg` (with --save-dir) also writes <save_dir>/<model>/imagenet_s_summary.json; the reference
    solver that defines this key is absent from the reference tree, so the summary's form is unpinned."""
    ops = imagenet_s_ops(getattr(args, 'imagenet_s_ops', None))
    dcfg = cfg.get('data', {})
    if (getattr(args, 'attack', None) and args.attack != 'none') or getattr(args, 'corruption', None) or natural_mode(dcfg):
        raise ValueError('--imagenet-s cannot be combined with --attack, --corruption or data.test.imagenet_a&o: no config of '
                         'imagenet_s_loop has another noise')
    if device.type != 'cuda':
        raise RuntimeError('--imagenet-s runs on the GPU (the resize operators are HIP kernels; no CPU fallback)')
    from ..metrics import ImageNetSEvaluator, ResultWriter, result_dir
    from ..noise import imagenet_s as NS
    bs = int(dcfg.get('batch_size', 64))
    size = int(dcfg.get('input_size', 224))
    ds = make_dataset(dcfg, int(dcfg.get('fake_size', dcfg.get('limit_samples', 256))), size, 'test')    # parses the transforms
    if not isinstance(ds, FileImageNet):
        raise ValueError('--imagenet-s needs data.read_from: fs (the loop is about decoding and resizing files)')
    idx = shard_indices(len(ds), rank, world)
    model = model or build_model(cfg, args)
    model = model.to(device).eval()
    use_hip = args.engine == 'hip'
    if use_hip:
        from ..model.engine import EngineModel
        prec = getattr(args, 'precision', None) or cfg.get('engine_precision', 'bf16')
        f_model = EngineModel(model, takes_normalized=False, precision=prec)
    mean = torch.tensor(IMAGENET_MEAN, device=device).view(1, 3, 1, 1)
    std = torch.tensor(IMAGENET_STD, device=device).view(1, 3, 1, 1)
    name = getattr(args, 'src_name', None) or cfg['model']['type']
    save_dir = getattr(args, 'save_dir', None)
    writers = {op: ResultWriter(result_dir(save_dir, name, 'imagenet_s', 'pil_%s' % op), rank, world) for op in ops} if save_dir else {}
    counters = {op: [0, 0] for op in ops}
    cnt = 0
    t0 = time.time()
    for s in range(0, len(idx), bs):
        items = idx[s:s + bs]
        decoded = ds.decode_indices(items, device)                 # once per batch, whatever the number of operators
        labels = torch.tensor([ds.items[i][1] for i in items], dtype=torch.int64, device=device)
        cnt += len(items)
        for op in ops:
            imgs = NS.image_transfer_batch(None, 'pil', op, 'val', size, ds.num_workers, decoded=decoded)
            if use_hip:
                logits = f_model.rart_engine.logits_from_u8(imgs, IMAGENET_MEAN, IMAGENET_STD)
            else:
                with torch.no_grad():
                    logits = model((imgs.permute(0, 3, 1, 2).float() / 255.0 - mean) / std)
            a, b = topk_correct(logits.float(), labels)
            counters[op][0] += a
            counters[op][1] += b
            if writers:
                writers[op].write_batch(logits, labels, items)
    barrier = dist.barrier if dist.is_available() and dist.is_initialized() else None
    paths = {op: writers[op].close(barrier=barrier) for op in ops} if writers else {}
    flat = all_reduce_counters([v for op in ops for v in counters[op]] + [cnt], device)
    cnt = flat[-1]
    res = None
    if rank == 0:
        ev = ImageNetSEvaluator()
        for k, op in enumerate(ops):
            if paths:
                ev.eval(paths[op], 'pil', op)
            else:
                ev.metric.update({('pil', op): 100.0 * flat[2 * k] / max(cnt, 1)})
        acc = {'%s/%s' % k: v for k, v in ev.metric.metric.items()}
        res = {'imagenet_s': acc, 'Mean': ev.get_mean()['Mean'], 'Std.': ev.get_std()['Std.'], 'count': cnt, 'world_size': world,
               'seconds': time.time() - t0}
        if save_dir and bool((dcfg.get('test') or {}).get('save_acc_var_neg', False)):
            import numpy as np
            vals = list(acc.values())
            with open(os.path.join(save_dir, name, 'imagenet_s_summary.json'), 'w') as f:
                json.dump({'acc': acc, 'mean': res['Mean'], 'var': float(np.var(vals)), 'neg_std': -res['Std.']}, f)
        print(json.dumps(res))
    return res


def _once_each(spec, what):
    toks = [t.strip() for t in str(spec).split(',') if t.strip()]
    if not toks:
        raise ValueError('%s: an empty list' % what)
    if len(set(toks)) != len(toks):
        raise ValueError('%s: every entry once, got %r' % (what, spec))
    return toks


def imagenet_c_names(spec=None):
    """`--imagenet-c-names a,b,...` -> (corruption names in order, named explicitly?).  None: the 15 standard corruptions,
    CORRUPTION_NAMES[:15]; 'all': these and the four extras; both name frost only implicitly.  An unknown or repeated name or an empty
    list is a ValueError."""
    from ..noise.imagenet_c import CORRUPTION_NAMES
    if spec is None:
        return list(CORRUPTION_NAMES[:15]), False
    if str(spec).strip() == 'all':
        return list(CORRUPTION_NAMES), False
    names = _once_each(spec, '--imagenet-c-names')
    for t in names:
        if t not in CORRUPTION_NAMES:
            raise ValueError('--imagenet-c-names: unknown corruption %r (%s)' % (t, ', '.join(CORRUPTION_NAMES)))
    return names, True


def imagenet_c_severities(spec=None):
    """`--imagenet-c-severities 1,2,...` -> severities in order; None: 1..5.  Anything outside 1..5, a repeat or an empty list is a
    ValueError."""
    if spec is None:
        return [1, 2, 3, 4, 5]
    out = []
    for t in _once_each(spec, '--imagenet-c-severities'):
        if t not in ('1', '2', '3', '4', '5'):
            raise ValueError('--imagenet-c-severities: %r is not a severity (1..5)' % (t,))
        out.append(int(t))
    return out


def read_frost_textures(path):
    """The photographs of a folder as uint8 HxWx3 arrays, read with Pillow in sorted file order (the order decides which photograph
    a sample draws)."""
    import numpy as np
    from PIL import Image
    if not os.path.isdir(path):
        raise ValueError('the frost folder %r is not a directory' % (path,))
    out = []
    for fn in sorted(os.listdir(path)):
        p = os.path.join(path, fn)
        if os.path.isfile(p):
            with Image.open(p) as im:
                out.append(np.array(im.convert('RGB')))
    if not out:
        raise ValueError('the frost folder %r holds no photographs' % (path,))
    return out


def imagenet_c_plan(cfg, args):
    """Everything `--imagenet-c` decides from the arguments and the config alone, before a model, a dataset or the device is
    looked at -> {'names', 'severities', 'skipped', 'frost_dir'}.  Frost needs photographs (--imagenet-c-frost-dir, the key
    data.test.imagenet_c_frost_dir, or an earlier set_frost_textures): without them a frost that only the default list or 'all'
    names is left out and listed under 'skipped'; a frost named explicitly is a ValueError."""
    from ..noise import imagenet_c as C
    names, explicit = imagenet_c_names(getattr(args, 'imagenet_c_names', None))
    sevs = imagenet_c_severities(getattr(args, 'imagenet_c_severities', None))
    dcfg = cfg.get('data', {}) or {}
    if (getattr(args, 'attack', None) and args.attack != 'none') or getattr(args, 'corruption', None) or getattr(args, 'imagenet_s', False) \
            or natural_mode(dcfg):
        raise ValueError('--imagenet-c cannot be combined with --attack, --corruption, --imagenet-s or data.test.imagenet_a&o: the loop '
                         'applies every corruption itself and no config of imagenet_c_loop_mini has another noise')
    if getattr(args, 'imagenet_c_scores', False) and not getattr(args, 'save_dir', None):
        raise ValueError('--imagenet-c-scores writes the full result files: it needs --save-dir')
    frost_dir = getattr(args, 'imagenet_c_frost_dir', None) or (dcfg.get('test') or {}).get('imagenet_c_frost_dir')
    skipped = []
    if 'frost' in names and not frost_dir and not C._frost_textures:
        if explicit:
            raise ValueError('--imagenet-c-names names frost, which needs photographs: pass --imagenet-c-frost-dir (or '
                             'data.test.imagenet_c_frost_dir)')
        names = [t for t in names if t != 'frost']
        skipped = ['frost']
    return {'names': names, 'severities': sevs, 'skipped': skipped, 'frost_dir': frost_dir}


def evaluate_imagenet_c(cfg, args, rank, world, device, model=None):
    """`--evaluate --imagenet-c`: the loop of exp/imagenet_c_loop_mini: one model scored on every (corruption, severity) pair in one
    pass over the test set.  Per batch of sharded indices the dataset is read ONCE (any data.read_from); every pair corrupts that
    batch into one scratch buffer (the source batch is never written), the engine turns it into logits and rart_topk_score_f32 adds
    the top-1 / top-5 hits to the pair's two counters, which stay on the device: nothing is read on the host inside the loop, and
    one all_reduce and one read end it.  gaussian_noise and speckle_noise run all their severities in one noise_severities_ launch
    (bit-identical to the per-severity calls).  Seed and sample offset are those of a single `--corruption NAME --severity S` run,
    so a pair's inputs, logits and result directory <save_dir>/<model>/<corruption>_<severity>/ are that run's.  With --save-dir a
    pair's file holds RankWriter lines (prediction, label, rank: 8 bytes per sample off the device), or the full ResultWriter lines
    under --imagenet-c-scores; rank 0 evaluates every file with ImageNetCEvaluator.  Accuracies are percentages, as the evaluator's.
    The reference's multi_eval_solver, which defines this loop's summary, is absent from the reference tree: the form of the
    printed line ('imagenet_c' per pair, 'error' = mean top-1 error per corruption over the severities run, 'Mean' of those, 'skipped')
    is unpinned."""
    plan = imagenet_c_plan(cfg, args)
    if device.type != 'cuda':
        raise RuntimeError('--imagenet-c runs on the GPU (the corruptions and the scorer are HIP kernels; no CPU fallback)')
    from ..metrics import ImageNetCEvaluator, RankWriter, ResultWriter, result_dir, topk_score
    from ..noise import imagenet_c as C
    if plan['frost_dir'] and 'frost' in plan['names']:
        C.set_frost_textures(read_frost_textures(plan['frost_dir']))
    names, sevs = plan['names'], plan['severities']
    dcfg = cfg.get('data', {})
    bs = int(dcfg.get('batch_size', 64))
    size = int(dcfg.get('input_size', 224))
    ds = make_dataset(dcfg, int(dcfg.get('fake_size', dcfg.get('limit_samples', 256))), size, 'test')
    idx = shard_indices(len(ds), rank, world)
    model = model or build_model(cfg, args)
    model = model.to(device).eval()
    use_hip = args.engine == 'hip'
    if use_hip:
        from ..model.engine import EngineModel
        prec = getattr(args, 'precision', None) or cfg.get('engine_precision', 'bf16')
        f_model = EngineModel(model, takes_normalized=False, precision=prec)
    mean = torch.tensor(IMAGENET_MEAN, device=device).view(1, 3, 1, 1)
    std = torch.tensor(IMAGENET_STD, device=device).view(1, 3, 1, 1)
    name = getattr(args, 'src_name', None) or cfg['model']['type']
    save_dir = getattr(args, 'save_dir', None)
    full = bool(getattr(args, 'imagenet_c_scores', False))
    pairs = [(c, s) for c in names for s in sevs]
    slot = {p: k for k, p in enumerate(pairs)}
    writers = {}
    if save_dir:
        writers = {p: (ResultWriter if full else RankWriter)(result_dir(save_dir, name, p[0], '%d' % p[1]), rank, world) for p in pairs}
    counters = torch.zeros(2 * len(pairs) + 1, dtype=torch.int64, device=device)      # (top-1, top-5) per pair, then the sample count
    fused = [c for c in ('gaussian_noise', 'speckle_noise') if c in names and len(sevs) > 1]
    scratch = []
    cnt = 0
    t0 = time.time()

    def score(x, pair, labels, lab_host, items):
        if use_hip:
            logits = f_model.rart_engine.logits_from_u8(x, IMAGENET_MEAN, IMAGENET_STD)
        else:
            with torch.no_grad():
                logits = model((x.permute(0, 3, 1, 2).float() / 255.0 - mean) / std)
        w = writers.get(pair)
        keep = w is not None and not full
        p, r = topk_score(logits.float(), labels, ks=(1, 5), hits=counters[2 * slot[pair]:], pred=keep, rank=keep)
        if keep:
            w.write_batch(p, r, lab_host, items)
        elif w is not None:
            w.write_batch(logits, labels, items)

    for s in range(0, len(idx), bs):
        items = idx[s:s + bs]
        imgs, labels = ds.batch(items, device)                    # once per batch, whatever the number of pairs
        first = items[0]                                          # global index of the batch's first sample
        cnt += len(items)
        lab_host = labels.tolist() if writers and not full else None
        if not scratch or scratch[0].shape != imgs.shape:
            scratch = [torch.empty_like(imgs) for _ in range(len(sevs) if fused else 1)]
        for c in names:
            cid = C.CORRUPTION_NAMES.index(c)
            if c in fused:
                C.noise_severities_(imgs, scratch, sevs, seeds=[args.seed] * len(sevs), sample_offset=first, corruption_id=cid)
                for k, sv in enumerate(sevs):
                    score(scratch[k], (c, sv), labels, lab_host, items)
            else:
                for sv in sevs:
                    C.corrupt_batch_(imgs, cid, sv, seed=args.seed, sample_offset=first, out=scratch[0])
                    score(scratch[0], (c, sv), labels, lab_host, items)
    barrier = dist.barrier if dist.is_available() and dist.is_initialized() else None
    paths = {}
    if writers:
        for w in writers.values():
            w.f.close()
        if barrier is not None:
            barrier()                                             # one for all the files: every shard is on disk before rank 0 merges
        paths = {p: writers[p].close() for p in pairs}
    counters[-1] = cnt
    if dist.is_available() and dist.is_initialized():
        dist.all_reduce(counters)
    flat = counters.tolist()                                      # the loop's only read of a counter
    cnt = int(flat[-1])
    res = None
    if rank == 0:
        ev = ImageNetCEvaluator(topk=(1, 5))
        acc = {}
        for k, p in enumerate(pairs):
            if paths:
                m = ev.eval(paths[p]).metric
                acc['%s/%d' % p] = {'top1': m['top1'], 'top5': m['top5']}
            else:
                acc['%s/%d' % p] = {'top1': float(flat[2 * k] * (100.0 / max(cnt, 1))), 'top5': float(flat[2 * k + 1] * (100.0 / max(cnt, 1)))}
        error = {c: 100.0 - sum(acc['%s/%d' % (c, sv)]['top1'] for sv in sevs) / len(sevs) for c in names}
        res = {'imagenet_c': acc, 'error': error, 'Mean': sum(error.values()) / len(error) if error else None,
               'skipped': plan['skipped'], 'count': cnt, 'world_size': world, 'seconds': time.time() - t0}
        print(json.dumps(res))
    return res


def evaluate(cfg, args, rank, world, device, model=None):
    """Clean / corrupted / attacked evaluation over the sharded dataset; returns the reduced metrics dict."""
    dcfg = cfg.get('data', {})
    if getattr(args, 'imagenet_c', False):
        return evaluate_imagenet_c(cfg, args, rank, world, device, model)
    if getattr(args, 'imagenet_s', False):
        return evaluate_imagenet_s(cfg, args, rank, world, device, model)
    if natural_mode(dcfg):
        return evaluate_natural(cfg, args, rank, world, device, model)
    n = int(dcfg.get('fake_size', dcfg.get('limit_samples', 256)))
    bs = int(dcfg.get('batch_size', 64))
    size = int(dcfg.get('input_size', 224))
    ds = make_dataset(dcfg, n, size, 'test')
    n = len(ds)                                              # a file-backed set brings its own length
    idx = shard_indices(n, rank, world)
    model = model or build_model(cfg, args)
    model = model.to(device).eval()
    use_hip = device.type == 'cuda' and args.engine == 'hip'
    noise = None
    if use_hip:
        from ..model.engine import EngineModel
        # `engine_precision: fp32x` (or --precision fp32x): the reference-precision engine mode (logits within 1e-4 of the
        # fp32 network, ~3x the MFMA work); default bf16
        prec = getattr(args, 'precision', None) or cfg.get('engine_precision', 'bf16')
        f_model = EngineModel(model, takes_normalized=False, precision=prec)
        n_model = EngineModel(None, takes_normalized=True, engine=f_model.rart_engine)
    if args.corruption:
        from ..noise import AddNoise
        noise = AddNoise('imagenet-c')
        noise.config.update(corruption_name=args.corruption, severity=args.severity)
    attack = None
    if args.attack and args.attack != 'none':
        from ..noise import AddNoise
        attack = AddNoise(args.attack)
        key = 'f_model' if 'f_model' in attack.config else 'model'
        if not use_hip:
            raise RuntimeError('attacks need the GPU path (no CPU fallback)')
        attack.config[key] = f_model if key == 'f_model' else n_model      # ResNet-50 and ViT-B/16: HIP forward + backward
        attack.config['eps'] = parse_eps(args.eps)
        if 'steps' in attack.config and args.steps:
            attack.config['steps'] = args.steps
    mean = torch.tensor(IMAGENET_MEAN, device=device).view(1, 3, 1, 1)
    std = torch.tensor(IMAGENET_STD, device=device).view(1, 3, 1, 1)
    # transfer harness: adversarial examples crafted on cfg.model, scored on the target model
    tgt_model = None
    if getattr(args, 'tgt_type', None):
        from ..model import get_model
        tgt = get_model({'type': args.tgt_type}).to(device).eval()
        if use_hip:
            from ..model.engine import EngineModel
            try:
                tgt_model = EngineModel(tgt, takes_normalized=False)
            except Exception:                                   # no HIP engine for this architecture: torch module
                tgt_model = lambda z, _t=tgt: _t((z - mean) / std)   # noqa: E731
        else:
            tgt_model = lambda z, _t=tgt: _t((z - mean) / std)       # noqa: E731
    writer = None
    if getattr(args, 'save_dir', None):
        from ..metrics import ResultWriter, result_dir
        noise_name = args.corruption or (args.attack if args.attack and args.attack != 'none' else 'none')
        eps_name = ('%d' % args.severity) if args.corruption else (
            ('%.3f' % parse_eps(args.eps)) if noise_name != 'none' else '0')
        writer = ResultWriter(result_dir(args.save_dir, getattr(args, 'src_name', None) or cfg['model']['type'],
                                         noise_name, eps_name, tgt_name=getattr(args, 'tgt_name', None)), rank, world)
    c1 = c5 = cnt = 0
    t0 = time.time()
    for s in range(0, len(idx), bs):
        items = idx[s:s + bs]
        imgs, labels = ds.batch(items, device)
        first = items[0]                                       # global index of the batch's first sample
        if noise is not None:
            from ..noise import imagenet_c as C
            C.corrupt_batch_(imgs, C.CORRUPTION_NAMES.index(args.corruption), args.severity, seed=args.seed,
                             sample_offset=first)
        if attack is not None:
            # the attack's random starts are a function of (seed, dataset index): set the process-wide counter to the
            # batch's first global index, which every attack reads when no explicit sample_offset is passed
            from ..noise import rng
            rng.manual_seed(args.seed, first)
            x01 = imgs.permute(0, 3, 1, 2).float().div(255.0).contiguous()
            adv_x = attack.add_noise(x01, labels)
            with torch.no_grad():
                logits = (tgt_model or f_model)(adv_x)
        elif use_hip:
            logits = f_model.rart_engine.logits_from_u8(imgs, IMAGENET_MEAN, IMAGENET_STD)
        else:
            with torch.no_grad():
                logits = model((imgs.permute(0, 3, 1, 2).float() / 255.0 - mean) / std)
        a, b = topk_correct(logits.float(), labels)
        c1, c5, cnt = c1 + a, c5 + b, cnt + len(items)
        if writer is not None:
            writer.write_batch(logits, labels, idx[s:s + bs])
    if writer is not None:
        writer.close(barrier=dist.barrier if dist.is_available() and dist.is_initialized() else None)
    c1, c5, cnt = all_reduce_counters([c1, c5, cnt], device)
    res = {'top1': c1 / max(cnt, 1), 'top5': c5 / max(cnt, 1), 'count': cnt, 'world_size': world,
           'noise': args.corruption or args.attack or 'none', 'seconds': time.time() - t0}
    if rank == 0:
        print(json.dumps(res))
    return res


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
    model = build_model(cfg, args)
    from ..model.convstem_torch import convstem_of
    if convstem_of(model) is not None:         # before the model reaches the device: every reference config of these types evaluates
        raise NotImplementedError('training %r: the ConvStem models are evaluation only (forward and backward-to-input on the HIP '
                                  'engines; there is no train engine for the stem)' % (cfg['model']['type'],))
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
    resume = getattr(build_model, 'last_checkpoint', None) or {}
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
