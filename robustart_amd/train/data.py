"""The data side of cls_solver: the datasets behind `data.read_from`, the parser of the reference's transform lists, the eval and train samplers."""
import json
import os

import torch

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


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


def synthetic_size(dcfg):
    """the `n` an evaluation loop hands make_dataset: data.fake_size, else data.limit_samples, else 256"""
    return int(dcfg.get('fake_size', dcfg.get('limit_samples', 256)))


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
        epoch = self.epoch_of(it)
        mine = self._order(epoch)
        if getattr(self, '_dev_epoch', None) != (epoch, str(device)):
            if len(mine) and (int(mine.min()) < 0 or int(mine.max()) >= 1 << 32):
                raise ValueError('sample indices must lie in [0, 2^32)')
            self._dev = torch.as_tensor(mine, dtype=torch.int64).to(device)
            self._dev_epoch = (epoch, str(device))
        k = int(it) % self.per_epoch
        return self._dev[k * self.bs:(k + 1) * self.bs]
