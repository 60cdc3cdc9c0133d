"""Writes tests/golden/pair_plan.json: every distinct pair GEMM launch of one ResNet-50 and one ViT-B/16 gradient evaluation at
B = 256 in reference precision, and the plan rart_gemm_pair_plan_bf16 reports for it (256 CUs) under every schedule, lab level and
tile override the tests use.

    python tests/golden/make_pair_plan.py

The descriptors come from the engines themselves, driven on the CPU at B = 2 with the library replaced by a recorder (tests/_recorder.py),
with the batch rewritten to 256: a plan reads no memory, so the planes are dummy addresses.  tests/test_pair_plan_cpu.py and
profiles/pair_plan_trace.py read the file through `load`, `to_desc` and `plan` below."""
import contextlib
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [p for p in (os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))) if p not in sys.path]
PATH = os.path.join(HERE, 'pair_plan.json')
B_SMALL, B = 2, 256
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
ENTRIES = ('rart_gemm_pair_bf16', 'rart_gemm_pair2_bf16', 'rart_gemm_pair_classes_bf16')
PLANES = ('a_hi', 'a_lo', 'w_hi', 'w_lo', 'bias', 'res_hi', 'res_lo', 'dst_hi', 'dst_lo', 'aux_hi', 'aux_lo', 'mask_bits', 'sign_out')
INTS2 = ('lda2', 'k2', 'src2_h', 'src2_w', 'sy2', 'sx2')
CLS = ('tap_begin', 'n_taps', 'k_off', 'dst_oy', 'dst_ox', 'src2')
REC = ('family', 'tile_m', 'tile_n', 'tile_rows', 'm_begin', 'M', 'grid_x', 'grid_y', 'walk_wgs', 'block')
DEFAULT = dict(schedule=1, env={}, tile_m=0, tile_n=0)


def variants():
    """label -> (schedule, lab variables, tile_m, tile_n): what every shape is planned under"""
    v = {'schedule%d' % s: dict(DEFAULT, schedule=s) for s in (0, 1, 2, 3)}
    v.update({'rows224=%d' % r: dict(DEFAULT, env={'RART_PAIR_ROWS224': str(r)}) for r in (0, 2, 3)})
    v['split=0'] = dict(DEFAULT, env={'RART_PAIR_SPLIT': '0'})
    v['schedule3 plain'] = dict(DEFAULT, schedule=3, env={'RART_PAIR_ROWS224': '0', 'RART_PAIR_SPLIT': '0'})      # what is left is walked
    v.update({'tile_m=%d' % t: dict(DEFAULT, tile_m=t) for t in (128, 224, 256)})
    v.update({'tile_n=%d' % t: dict(DEFAULT, tile_n=t) for t in (64, 128, 256)})
    return v


# ---------------------------------------------------------------------- descriptors <-> plain dictionaries
def _ints(struct, skip=()):
    out = {}
    for name, typ in struct._fields_:
        if name in skip or typ is ctypes.c_void_p or issubclass(typ, ctypes.Structure):
            continue
        v = getattr(struct, name)
        out[name] = list(v) if hasattr(v, '__len__') else int(v)
    return out


def _case(entry, d):
    """a recorded descriptor as a dictionary of its integers and of which optional planes it has"""
    two = d.two if entry == ENTRIES[2] else d if entry == ENTRIES[1] else None
    one = two.one if two is not None else d
    c = dict(one=_ints(one), planes=[n for n in PLANES if getattr(one, n)])
    if two is not None and two.a2_hi:
        c['two'] = {n: getattr(two, n) for n in INTS2}
    if entry == ENTRIES[2]:
        c['classes'] = [{n: getattr(d.cls[i], n) for n in CLS} for i in range(d.n_classes)]
    return c


def _at_256(c):
    """the batch of a case recorded at B_SMALL rewritten to B"""
    o = c['one']
    if o['conv']:
        assert o['batch'] == B_SMALL
        o['batch'] = B
        o['M'] = o['M'] // B_SMALL * B if o['M'] else 0
    elif o['n_batched'] > 1:           # one problem per (image, head): the images are in n_batched and the outer strides
        assert o['n_batched'] % B_SMALL == 0
        o['n_batched'] = o['n_batched'] // B_SMALL * B
    else:
        assert o['M'] % B_SMALL == 0
        o['M'] = o['M'] // B_SMALL * B
    return c


def to_desc(case, tile_m=0, tile_n=0):
    """the rart_gemm_pair_cls_desc of a case, its planes dummy non-null addresses (never read by a plan)"""
    from robustart_amd import _lib
    d = _lib.GemmPairClsDesc()
    one = d.two.one
    for k, v in case['one'].items():
        if isinstance(v, list):
            getattr(one, k)[:] = v
        else:
            setattr(one, k, v)
    for i, n in enumerate(case['planes']):
        setattr(one, n, 4096 * (i + 1))
    if 'two' in case:
        d.two.a2_hi, d.two.a2_lo = 4096 * 20, 4096 * 21
        for k, v in case['two'].items():
            setattr(d.two, k, v)
    for i, c in enumerate(case.get('classes', ())):
        for k, v in c.items():
            setattr(d.cls[i], k, v)
    d.n_classes = len(case.get('classes', ()))
    one.tile_m, one.tile_n = tile_m, tile_n
    return d


def name_of(case):
    o = case['one']
    n = '%d x %d -> %d' % (o['M'] if not o['conv'] else o['batch'] * o['grid_h'] * o['grid_w'],
                           o['K'] if not o['conv'] else o['k_per_tap'] * o['n_taps'] + case.get('two', {}).get('k2', 0), o['N'])
    if o['conv']:
        n += ' conv %d taps' % o['n_taps']
    if 'two' in case:
        n += ' two sources'
    if 'classes' in case:
        n += ' %d classes' % len(case['classes'])
    if o['n_batched'] > 1:
        n += ' batched %d' % o['n_batched']
    return n


# ---------------------------------------------------------------------- the plan entry
@contextlib.contextmanager
def lab(lib, schedule, env):
    """the schedule and the lab variables of the calls inside, put back afterwards"""
    names = ('RART_PAIR_ROWS224', 'RART_PAIR_SPLIT', 'RART_PAIR_NT_MIN_MB')
    old_env, old_schedule = {n: os.environ.get(n) for n in names}, lib.rart_gemm_pair_get_schedule()
    try:
        for n in names:
            os.environ.pop(n, None)
        os.environ.update(env)
        assert lib.rart_gemm_pair_set_schedule(schedule) == 0
        yield
    finally:
        lib.rart_gemm_pair_set_schedule(old_schedule)
        for n, v in old_env.items():
            os.environ.pop(n, None)
            if v is not None:
                os.environ[n] = v


def plan(lib, desc, cus=256):
    """the launch records rart_gemm_pair_plan_bf16 reports (a list of dictionaries); raises with the library's message when it refuses"""
    from robustart_amd import _lib
    out = _lib.GemmPairPlan()
    st = lib.rart_gemm_pair_plan_bf16(ctypes.byref(desc), cus, ctypes.byref(out))
    if st != 0:
        raise ValueError('status %d: %s' % (st, lib.rart_last_error_string().decode()))
    return [{n: getattr(out.launch[i], n) for n in REC} for i in range(out.n_launches)]


def plans_of(lib, case):
    out = {}
    for label, v in variants().items():
        with lab(lib, v['schedule'], v['env']):
            out[label] = plan(lib, to_desc(case, v['tile_m'], v['tile_n']))
    return out


# ---------------------------------------------------------------------- the shape table, from the engines
@contextlib.contextmanager
def _recording():
    """robustart_amd._lib answering from a recorder that says what the real library says about sources and classes"""
    import torch
    from _recorder import Recorder
    from robustart_amd import _lib

    class Rec(Recorder):
        def __getattr__(self, name):
            fixed = {'rart_gemm_pair_max_sources': 2, 'rart_gemm_pair_max_classes': 4}
            return (lambda: fixed[name]) if name in fixed else Recorder.__getattr__(self, name)
    rec = Rec()
    rec.supported = lambda name, args: 1
    old = _lib.require_gpu, _lib.stream_ptr, _lib.load
    _lib.require_gpu, _lib.stream_ptr, _lib.load = (lambda: torch), (lambda: None), (lambda: rec)
    try:
        yield rec
    finally:
        _lib.require_gpu, _lib.stream_ptr, _lib.load = old


def _stub_loss(n):
    import torch
    from robustart_amd.noise import adv
    old = adv.logit_loss
    adv.logit_loss = lambda logits, *a: (torch.zeros(B_SMALL), torch.ones(B_SMALL, n), torch.zeros(B_SMALL, dtype=torch.int32))
    return lambda: setattr(adv, 'logit_loss', old)


def _collect(rec, cases):
    for entry, args in rec.calls:
        if entry in ENTRIES:
            c = _at_256(_case(entry, args[0]._obj))
            c['name'] = name_of(c)
            if c not in cases:
                cases.append(c)
    rec.calls.clear()


def engine_cases():
    """the distinct pair launches of one gradient evaluation of ResNet-50 and of ViT-B/16 (fused attention and its decomposition)"""
    import torch
    from robustart_amd.model import get_model
    from robustart_amd.model.engine import ResNet50Engine
    from robustart_amd.model.vit_engine import ViTEngine
    from robustart_amd.model.vit_torch import VisionTransformer
    cases = []
    x = torch.rand(B_SMALL, 3, 224, 224)
    with _recording() as rec:
        undo = _stub_loss(1000)
        try:
            torch.manual_seed(0)
            eng = ResNet50Engine(get_model({'type': 'resnet50_official'}).eval(), 'cpu', 'fp32x')
            rec.calls.clear()
            eng.forward_backward(x, MEAN, STD, None, 0)
            _collect(rec, cases)
            vit = ViTEngine(VisionTransformer(img_size=224, num_classes=1000, embed_dim=768, depth=1, num_heads=12).eval(), 'cpu', 'fp32x')
            for fused in (True, False):
                vit.fused_attention = vit.fused_attention_bwd = fused
                rec.calls.clear()
                vit.forward_backward(x, MEAN, STD, None, 0)
                _collect(rec, cases)
        finally:
            undo()
    return cases


def load():
    return json.load(open(PATH))


if __name__ == '__main__':
    from robustart_amd import _lib
    lib = _lib.load()
    cases = engine_cases()
    for c in cases:
        c['plans'] = plans_of(lib, c)
    with open(PATH, 'w') as f:
        f.write('{"cus": 256, "cases": [\n' + ',\n'.join(json.dumps(c, sort_keys=True) for c in cases) + '\n]}\n')
    print('%d cases -> %s' % (len(cases), PATH))
