"""Record tests/golden/row_engine_trace.json: what the row engines (ViT, MLP-Mixer, ConvNeXt, ConvNeXt-V2, their ConvStem variants and
the three train engines) hand to the library on tiny modules, driven on the CPU with the library replaced by a recorder.

    python tests/golden/make_row_engine_trace.py [--out PATH] [--dump CASE]

Per case: the launches in order (entry name, every scalar argument, every non-pointer descriptor field, every pointer as
`name+byte offset` of the engine buffer, weight table, parameter or gradient it points into, resolved at the moment of the call:
buffers are re-allocated when their shape changes) and, per weight table `refold` builds, shape, dtype and the SHA-256 of its bytes (its first
16 hex digits).
The JSON keeps one `entry:hash` string per launch.  It was recorded from the commit before the row engines moved onto one table
builder and one per-precision call path; tests/test_engine_launch_cpu.py regenerates the trace from the working tree and compares, so
the host code may be rearranged as long as every kernel still receives the same arguments on tables with the same bytes.  Buffer and
table attribute names are part of the trace.  --dump prints one case in full, to diff two trees by hand."""
import argparse
import contextlib
import ctypes
import hashlib
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
B, CLASSES = 2, 10
SKIP_ATTRS = ('lib', '_buf', '_w_il', 'model', 'profile', 'eng', '_saved', '_kept', 'last_dlogits')


def _span(t):
    return t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()


def _tensors(obj, path, out):
    """every tensor reachable from the engine attribute `obj` (dicts, lists, tuples, the ConvStem helper), by attribute path"""
    if torch.is_tensor(obj):
        out.append((path, obj))
    elif isinstance(obj, dict):
        for k in obj:
            _tensors(obj[k], '%s.%s' % (path, k), out)
    elif isinstance(obj, (list, tuple)):
        for i, v in enumerate(obj):
            _tensors(v, '%s[%d]' % (path, i), out)
    elif type(obj).__module__.startswith('robustart_amd.model') and not isinstance(obj, torch.nn.Module):
        for k, v in vars(obj).items():
            if k not in SKIP_ATTRS:
                _tensors(v, '%s.%s' % (path, k) if path else k, out)


def _named_tables(eng):
    """[(attribute path, tensor)] of everything `refold` built, the interleaved copies in `_w_il` by the table they belong to"""
    tabs = []
    _tensors(eng, '', tabs)
    return tabs + [('w_il(%s)' % next(n for n, t in tabs if t.data_ptr() == k), il) for k, il in eng._w_il.items()]


class Library:
    """stands in for the shared library: answers every rart_* entry, records it with its pointers named"""

    def __init__(self):
        self.engine, self.fixed, self.launches = None, [], []

    def names(self):
        """[(first byte, past the last byte, name)] in the order a pointer is looked up: engine buffers, weight tables, then the
        fixed tensors of the case (gradients, parameters, inputs)"""
        eng, out = self.engine, []
        if eng is None:                      # a question the constructor asks the library
            return out
        tabs = _named_tables(eng)
        for name, t in [('buf:' + k, eng._buf[k]) for k in sorted(eng._buf)] + tabs + self.fixed:
            if t.numel():
                out.append(_span(t) + (name,))
        return out

    def _ptr(self, p, names):
        if p is None:
            return 'null'
        for lo, hi, name in names:
            if lo <= p < hi:
                return '%s+%d' % (name, p - lo)
        return ('?', p)                      # a tensor the engine returns: named by role when the call is over

    def _field(self, v):
        if isinstance(v, ctypes.Array):
            return [int(x) if isinstance(x, int) else float(x) for x in v]
        return v

    def _arg(self, a, names):
        if isinstance(a, ctypes.c_void_p):
            return self._ptr(a.value, names)
        if hasattr(a, '_obj'):               # byref(descriptor)
            d = a._obj
            return {f: self._ptr(getattr(d, f), names) if t is ctypes.c_void_p else self._field(getattr(d, f))
                    for f, t in d._fields_}
        if isinstance(a, ctypes.Array):
            return self._field(a)
        if a is None:
            return 'null'
        if isinstance(a, (bool, int, float)):
            return a
        raise TypeError('argument %r of an unexpected type' % (a,))

    def __getattr__(self, name):
        if not name.startswith('rart_'):
            raise AttributeError(name)

        def call(*args):
            names = self.names()
            self.launches.append([name] + [self._arg(a, names) for a in args])
            if name.endswith('_workspace_bytes'):
                return 4096
            if name.endswith('_supported'):
                return 0 if name == 'rart_gemm256_supported' else 1
            return 0
        return call

    def settle(self, roles):
        """name the pointers left open by the tensors the call returned: roles = [(name, tensor)]"""
        spans = [_span(t) + (n,) for n, t in roles if t is not None and t.numel()]

        def fix(v):
            if isinstance(v, tuple) and v and v[0] == '?':
                for lo, hi, name in spans:
                    if lo <= v[1] < hi:
                        return '%s+%d' % (name, v[1] - lo)
                raise RuntimeError('pointer %#x of %s points into no named tensor' % (v[1], launch[0]))
            if isinstance(v, dict):
                return {k: fix(x) for k, x in v.items()}
            return v
        for launch in self.launches:
            launch[1:] = [fix(v) for v in launch[1:]]


@contextlib.contextmanager
def cpu_library(lib, loss):
    from robustart_amd import _lib
    from robustart_amd.noise import adv
    saved = [(_lib, 'require_gpu', _lib.require_gpu), (_lib, 'load', _lib.load), (_lib, 'stream_ptr', _lib.stream_ptr),
             (adv, 'logit_loss', adv.logit_loss)]
    _lib.require_gpu, _lib.load, _lib.stream_ptr = (lambda: torch), (lambda: lib), (lambda: None)
    adv.logit_loss = lambda logits, *a: loss
    try:
        yield
    finally:
        for mod, name, fn in saved:
            setattr(mod, name, fn)


def _fill(model, seed):
    """deterministic parameters from the uniform generator alone (the same bits on every CPU)"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            p.copy_((torch.rand(p.shape, generator=g) - 0.5) * 0.2)
            if 'norm' in name and name.endswith('weight'):
                p.add_(1.0)
    return model.eval()


def _vit():
    from robustart_amd.model.vit_torch import VisionTransformer
    return VisionTransformer(img_size=32, num_classes=CLASSES, embed_dim=128, depth=1, num_heads=2)


def _vit_cvst():
    from robustart_amd.model.convstem_torch import VisionTransformerCvSt
    return VisionTransformerCvSt(stem_widths=(32, 48, 64, 96), img_size=32, num_classes=CLASSES, embed_dim=128, depth=1, num_heads=2)


def _mixer():
    from robustart_amd.model.mixer_torch import MlpMixer
    return MlpMixer(num_classes=CLASSES, img_size=32, patch_size=16, embed_dim=128, depth=1)


def _convnext():
    from robustart_amd.model.convnext_torch import ConvNeXt
    return ConvNeXt(depths=(1, 1, 1, 1), dims=(32, 64, 128, 256), num_classes=CLASSES)


def _convnext_v2():
    from robustart_amd.model.convnext_torch import ConvNeXtV2
    return ConvNeXtV2(depths=(1, 1, 1, 1), dims=(32, 64, 128, 256), num_classes=CLASSES)


def _convnext_cvst():
    from robustart_amd.model.convstem_torch import ConvNeXtCvSt
    return ConvNeXtCvSt(stem_widths=(32, 48), depths=(1, 1, 1, 1), dims=(48, 64, 128, 256), num_classes=CLASSES)


def _engine_class(name):
    import importlib
    mod, cls = name.split('.')
    return getattr(importlib.import_module('robustart_amd.model.' + mod), cls)


# (case, module, engine class, keyword arguments of the case)
EVAL = [('vit', _vit, 'vit_engine.ViTEngine', {}),
        ('vit_unfused', _vit, 'vit_engine.ViTEngine', dict(unfused=True)),
        ('vit_cvst', _vit_cvst, 'vit_engine.ViTEngine', {}),
        ('mixer', _mixer, 'mixer_engine.MixerEngine', {}),
        ('convnext', _convnext, 'convnext_engine.ConvNeXtEngine', {}),
        ('convnext_v2', _convnext_v2, 'convnext_engine.ConvNeXtEngine', {}),
        ('convnext_cvst', _convnext_cvst, 'convnext_engine.ConvNeXtEngine', {})]
TRAIN = [('vit_train', _vit, 'vit_train_engine.ViTTrainEngine'),
         ('mixer_train', _mixer, 'mixer_train_engine.MixerTrainEngine'),
         ('convnext_train', _convnext, 'convnext_train_engine.ConvNeXtTrainEngine'),
         ('convnext_v2_train', _convnext_v2, 'convnext_train_engine.ConvNeXtTrainEngine')]


def _tables(lib):
    out = {}
    for name, t in _named_tables(lib.engine):
        assert t.is_contiguous(), '%s is a strided view: the kernels read it through data_ptr()' % name
        raw = t.detach().view(torch.uint8).numpy().tobytes() if t.numel() else b''
        out[name] = '%s %s %s' % ('x'.join(map(str, t.shape)), str(t.dtype).replace('torch.', ''), hashlib.sha256(raw).hexdigest()[:16])
    return out


def _input():
    return torch.rand(B, 3, 32, 32, generator=torch.Generator().manual_seed(7))


def trace_eval(make, engine, precision, unfused=False, interleaved=False):
    """-> (launches of logits() then forward_backward(), tables) of an evaluation engine built by its own constructor on the CPU"""
    lib = Library()
    loss = (torch.zeros(B), torch.ones(B, CLASSES), torch.zeros(B, dtype=torch.int32))
    model, x = _fill(make(), 1), _input()
    old = os.environ.get('RART_PAIR_WIL')
    os.environ['RART_PAIR_WIL'] = '1' if interleaved else '0'
    try:
        with cpu_library(lib, loss):
            eng = lib.engine = _engine_class(engine)(model, 'cpu', precision)
            tables = _tables(lib)
            if unfused:
                eng.fused_attention = eng.fused_attention_bwd = False
            lib.fixed = [('input', x), ('dlogits', loss[1])] + [('param:' + n, p) for n, p in model.named_parameters()]
            lib.launches.clear()
            logits = eng.logits(x, MEAN, STD)
            lib.settle([('logits', logits)])
            n = len(lib.launches)
            logits, _, grad, _ = eng.forward_backward(x, MEAN, STD, None, 0)
            lib.settle([('logits', logits), ('input_grad', grad)])
            assert n and len(lib.launches) > 2 * n
    finally:
        if old is None:
            del os.environ['RART_PAIR_WIL']
        else:
            os.environ['RART_PAIR_WIL'] = old
    return lib.launches, tables


def trace_train(make, engine):
    """-> (launches of forward() then backward(), `grad_ready` marks among them, tables) of a train engine (bf16)"""
    lib = Library()
    model, x = _fill(make(), 1), _input()
    names = {}
    for n, p in model.named_parameters():
        p.grad = torch.zeros_like(p)
        names[id(p)] = n
    dlogits = torch.full((B, CLASSES), 0.25)
    with cpu_library(lib, None):
        eng = lib.engine = _engine_class(engine)(model, 'cpu', on_grad_ready=lambda p: lib.launches.append(['grad_ready', names[id(p)]]))
        tables = _tables(lib)
        lib.fixed = [('input', x), ('dlogits', dlogits)] + [('grad:' + n, p.grad) for n, p in model.named_parameters()] + \
            [('param:' + n, p) for n, p in model.named_parameters()]
        lib.launches.clear()
        logits = eng.forward(x, False, MEAN, STD)
        lib.settle([('logits', logits)])
        n = len(lib.launches)
        eng.backward(dlogits)
        lib.settle([])
        assert n and len(lib.launches) > 2 * n
        assert sorted(a[1] for a in lib.launches if a[0] == 'grad_ready') == sorted(names.values())
    return lib.launches, tables


def cases():
    """{case name: thunk -> (launches, tables)}"""
    out = {}
    for name, make, engine, kw in EVAL:
        for precision in ('bf16', 'fp32x'):
            out['%s/%s' % (name, precision)] = lambda make=make, engine=engine, precision=precision, kw=kw: \
                trace_eval(make, engine, precision, **kw)
    out['vit_interleaved/fp32x'] = lambda: trace_eval(_vit, 'vit_engine.ViTEngine', 'fp32x', interleaved=True)
    for name, make, engine in TRAIN:
        out['%s/bf16' % name] = lambda make=make, engine=engine: trace_train(make, engine)
    return out


def digest(launches, tables):
    return dict(launches=['%s:%s' % (a[0], hashlib.sha256(json.dumps(a, sort_keys=True).encode()).hexdigest()[:10]) for a in launches],
                tables=tables)


def record():
    return {name: digest(*run()) for name, run in cases().items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(HERE, 'row_engine_trace.json'))
    ap.add_argument('--dump', help='print the launches and tables of one case in full instead')
    args = ap.parse_args()
    if args.dump:
        launches, tables = cases()[args.dump]()
        for i, a in enumerate(launches):
            print(i, json.dumps(a, sort_keys=True))
        for k in tables:
            print(k, tables[k])
        return
    rec = record()
    with open(args.out, 'w') as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write('\n')
    print('%d cases, %s launches' % (len(rec), [len(v['launches']) for v in rec.values()]))


if __name__ == '__main__':
    main()
