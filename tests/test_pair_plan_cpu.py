"""The pair GEMM's launch plan (csrc/gemm_pair.hip: gp_plan behind rart_gemm_pair_plan_bf16) without a GPU: the plans of every pair launch
of a ResNet-50 and a ViT-B/16 gradient evaluation at B = 256 against tests/golden/pair_plan.json, the invariants every plan keeps, over
that table and a sweep of shapes, that planning is a function of its inputs, and that the plan entry refuses what the launching entries
refuse, in the same words.  All plans are for 256 compute units unless a test says otherwise; the planes are dummy addresses."""
import ctypes
import importlib.util
import itertools
import os

import pytest

from robustart_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location('make_pair_plan', os.path.join(ROOT, 'tests', 'golden', 'make_pair_plan.py'))
mpp = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mpp)

TWO_STAGE, PING_PONG, PERSISTENT = 0, 1, 2


@pytest.fixture(scope='module')
def lib():
    return _lib.load()


@pytest.fixture(scope='module')
def golden():
    return mpp.load()


# ---------------------------------------------------------------------- the shape table
def test_table_is_what_the_engines_launch(golden):
    """the cases of the golden file are the distinct pair launches the engines make, and hold the shapes the measurements were about"""
    cases = golden['cases']
    assert [{k: v for k, v in c.items() if k != 'plans'} for c in cases] == mpp.engine_cases()
    names = [c['name'] for c in cases]
    for want in ('200704 x 384 -> 512 conv 1 taps two sources', '50176 x 768 -> 1024 conv 1 taps two sources',
                 '12544 x 1536 -> 2048 conv 1 taps two sources', '802816 x 320 -> 64 conv 1 taps two sources',
                 '200704 x 1024 -> 256 conv 4 taps two sources 4 classes',      # layer2's shortcut^T in conv1^T's class launch
                 '50432 x 768 -> 768', '50432 x 768 -> 2304', '50432 x 768 -> 3072', '50432 x 3072 -> 768',
                 '197 x 64 -> 200 batched 3072', '197 x 224 -> 64 batched 3072'):
        assert want in names, want


def test_plans_of_the_table(lib, golden):
    """every case under schedules 0-3, the lab levels of RART_PAIR_ROWS224 / RART_PAIR_SPLIT and the tile overrides of the GPU tests (and
    schedule 3 with the 224-row tiles and the split off, where the walked launches show)"""
    assert golden['cus'] == 256 and set(mpp.variants()) == {'schedule0', 'schedule1', 'schedule2', 'schedule3', 'rows224=0', 'rows224=2',
                                                            'rows224=3', 'split=0', 'schedule3 plain', 'tile_m=128', 'tile_m=224', 'tile_m=256',
                                                            'tile_n=64', 'tile_n=128', 'tile_n=256'}
    for c in golden['cases']:
        got = mpp.plans_of(lib, c)
        for label, want in c['plans'].items():
            assert got[label] == want, (c['name'], label)
        assert set(got) == set(c['plans'])


def test_the_measured_choices(golden):
    """the choices rounds 4-6 measured, spelled out: a slip in the policy shows here by name"""
    by_name = {c['name']: c['plans']['schedule1'] for c in golden['cases']}

    def tiles(name):
        return [(r['family'], r['tile_m'], r['tile_n'], r['tile_rows'], r['m_begin'], r['M']) for r in by_name[name]]
    for name, rows in (('200704 x 384 -> 512 conv 1 taps two sources', 200704), ('50176 x 768 -> 1024 conv 1 taps two sources', 50176),
                       ('12544 x 1536 -> 2048 conv 1 taps two sources', 12544)):
        assert tiles(name) == [(PING_PONG, 256, 256, 224, 0, rows)]
    assert tiles('802816 x 320 -> 64 conv 1 taps two sources') == [(TWO_STAGE, 128, 64, 128, 0, 802816)]
    assert tiles('200704 x 1024 -> 256 conv 4 taps two sources 4 classes') == [(PING_PONG, 256, 256, 256, 0, 200704)]
    # ViT-B/16's 197 row tiles: N = 768 (3 column tiles) on 224-row tiles; N = 2304 / 3072 split into the whole passes and the rest
    assert tiles('50432 x 768 -> 768') == [(PING_PONG, 256, 256, 224, 0, 50432)]
    for name in ('50432 x 768 -> 2304', '50432 x 768 -> 3072'):
        assert tiles(name) == [(PING_PONG, 256, 256, 256, 0, 192 * 256), (PING_PONG, 256, 128, 256, 192 * 256, 50432)]
    assert tiles('197 x 64 -> 200 batched 3072') == [(PING_PONG, 256, 256, 256, 0, 197)] and by_name['197 x 64 -> 200 batched 3072'][0]['grid_y'] == 3072


# ---------------------------------------------------------------------- invariants
def _check_invariants(plan, M, N, conv, two, classes, cus, what):
    assert 1 <= len(plan) <= 2, what
    assert plan[0]['m_begin'] == 0 and plan[-1]['M'] == M, what
    for a, b in zip(plan, plan[1:]):          # the row ranges [m_begin, M) partition [0, M) at multiples of 256
        assert a['M'] == b['m_begin'] and b['m_begin'] % 256 == 0 and 0 < b['m_begin'] < M, what
    for r in plan:
        fam, tm, tn, rows = r['family'], r['tile_m'], r['tile_n'], r['tile_rows']
        assert rows in (tm, tm - 32), what
        mt, nt = -(-(r['M'] - r['m_begin']) // rows), -(-N // tn)
        tiles = (-(-mt // 8) * 8 if mt >= 16 else mt) * nt
        walked = r['walk_wgs'] > 0
        if fam == PERSISTENT:
            assert walked and r['grid_x'] == r['walk_wgs'] == cus and mt * nt >= 2 * cus, what
        elif walked:
            assert r['grid_x'] == min(r['walk_wgs'], tiles) and tiles > cus, what
        else:
            assert r['grid_x'] == tiles, what
        assert 0 < r['grid_x'] < 2 ** 31 and 0 < r['grid_y'] <= 65535, what
        if walked:
            assert r['grid_y'] == 1 and not two and not classes, what
        # an instance the issue step has: k_gemm_pair<128 | 256, 64 | 128 | 256>, k_gemm_pair_pp<128 | 256> (256-row tiles), k_gemm_pair_ps
        # (256 x 128); a second source and classes on conv instances only, classes in blockIdx.y
        if fam == TWO_STAGE:
            assert tm in (128, 256) and tn in (64, 128, 256) and r['block'] == 2 * tm and not walked, what
        elif fam == PING_PONG:
            assert tm == 256 and tn in (128, 256) and r['block'] == 512, what
        else:
            assert fam == PERSISTENT and (tm, tn, rows, r['block']) == (256, 128, 256, 512), what
        assert conv or not (two or classes), what
        if classes:
            assert r['grid_y'] == classes, what


def test_invariants_over_the_table(golden):
    for c in golden['cases']:
        o = c['one']
        M = o['batch'] * o['grid_h'] * o['grid_w'] if o['conv'] else o['M']
        for label, plan in c['plans'].items():
            _check_invariants(plan, M, o['N'], o['conv'], 'two' in c, len(c.get('classes', ())), 256, (c['name'], label))


def _sweep_case(M, N, K, conv):
    one = dict(M=M, N=N, K=K, lda=K, ldw=K, ldc=N, w_rows=N, conv=0, flags=0, n_batched=0, z_inner=0)
    if conv:          # rows = an M x 1 grid of one image; K = one tap, or the nine taps of a 3x3 where K is no power of two
        taps = 1 if K & (K - 1) == 0 else 9
        t = [(r - 1, s - 1) for r in range(3) for s in range(3)] if taps == 9 else [(0, 0)]
        one.update(conv=1, batch=1, grid_h=M, grid_w=1, src_h=M, src_w=1, sy=1, sx=1, k_per_tap=K // taps, n_taps=taps, lda=K // taps,
                   tap_dy=[a for a, _ in t] + [0] * (16 - taps), tap_dx=[b for _, b in t] + [0] * (16 - taps),
                   dst_h=M, dst_w=1, dst_sy=1, dst_sx=1)
    return dict(one=one, planes=['a_hi', 'a_lo', 'w_hi', 'w_lo', 'dst_hi', 'dst_lo'])


def test_invariants_over_a_sweep(lib):
    Ms = (1, 255, 256, 257, 4095, 4096, 12544, 50176, 50432, 200704, 802816)
    Ns = (8, 64, 72, 128, 136, 256, 264, 768, 2048)
    Ks = (32, 64, 256, 288, 1024, 4608)
    planned = 0
    for conv, M, N, K in itertools.product((1, 0), Ms, Ns, Ks):
        d = mpp.to_desc(_sweep_case(M, N, K, conv))
        for schedule in (0, 1, 2, 3):
            with mpp.lab(lib, schedule, {}):
                for cus in (8, 64, 256, 304):
                    try:
                        plan = mpp.plan(lib, d, cus)
                    except ValueError as e:      # the one refusal the sweep can meet: a plain source plane of M x K elements past 2 GiB
                        assert not conv and M * K >= 2 ** 30 and 'a source plane must stay below 2 GiB' in str(e), (M, N, K, conv, str(e))
                        continue
                    _check_invariants(plan, M, N, conv, False, 0, cus, (M, N, K, conv, schedule, cus))
                    planned += 1
    assert planned > 4 * 4 * 1000


# ---------------------------------------------------------------------- purity
def test_planning_is_a_function_of_its_inputs(lib, golden):
    by_name = {c['name']: c for c in golden['cases']}
    before = lib.rart_gemm_pair_get_schedule()
    vit, r50 = by_name['50432 x 768 -> 2304'], by_name['50176 x 1024 -> 512 conv 1 taps']
    with mpp.lab(lib, 1, {}):
        d = mpp.to_desc(vit)
        first = mpp.plan(lib, d)
        assert mpp.plan(lib, d) == first and len(first) == 2
        # the lab variables are read on every call: a change between two calls changes the second plan
        os.environ['RART_PAIR_SPLIT'] = '0'
        assert len(mpp.plan(lib, d)) == 1
        del os.environ['RART_PAIR_SPLIT']
        assert mpp.plan(lib, d) == first
        d = mpp.to_desc(r50)
        assert mpp.plan(lib, d)[0]['tile_rows'] == 224
        os.environ['RART_PAIR_ROWS224'] = '0'
        assert mpp.plan(lib, d)[0]['tile_rows'] == 256
        del os.environ['RART_PAIR_ROWS224']
        assert lib.rart_gemm_pair_get_schedule() == 1
    with mpp.lab(lib, 2, {}):          # the CU count is an input like the others: the persistent kernel's grid
        assert [mpp.plan(lib, d, cus)[0]['grid_x'] for cus in (256, 304)] == [256, 304]
    assert lib.rart_gemm_pair_get_schedule() == before


# ---------------------------------------------------------------------- error parity
def _malformed(golden):
    """(what, descriptor): descriptors the launching entries refuse before any HIP call"""
    by_name = {c['name']: c for c in golden['cases']}
    conv, plain = by_name['50176 x 2304 -> 256 conv 9 taps'], by_name['50432 x 768 -> 2304']
    two, cls = by_name['50176 x 768 -> 1024 conv 1 taps two sources'], by_name['12544 x 4096 -> 1024 conv 4 taps two sources 4 classes']
    batched = by_name['197 x 64 -> 200 batched 3072']

    def bad(case, what, **one):
        d = mpp.to_desc(case)
        for k, v in one.items():
            setattr(d.two.one, k, v)
        return what, d
    out = [bad(conv, 'n_taps must be 1..16', n_taps=17), bad(conv, 'power of two', k_per_tap=48), bad(conv, 'multiple of 8', N=12),
           bad(plain, 'leading dimensions', ldw=760), bad(plain, 'lda must cover', lda=764), bad(batched, 'n_batched', n_batched=70000),
           bad(plain, 'null operand plane', a_lo=None), bad(plain, 'unknown flag', flags=1 << 10), bad(plain, 'GELU_KEEP', flags=64),
           bad(two, 'leading dimensions', ldw=512), bad(plain, 'residual is a pair', res_hi=4096)]
    what, d = bad(two, 'k2 must be')
    d.two.k2 = 40
    out.append((what, d))
    what, d = bad(two, 'both planes or none')
    d.two.a2_lo = None
    out.append((what, d))
    what, d = bad(cls, 'inside the rows of the weight table')      # a class slice past ldw
    d.cls[1].k_off = d.two.one.ldw - 8
    out.append((what, d))
    what, d = bad(cls, '1..4 classes')
    d.n_classes = 5
    out.append((what, d))
    return out


def test_the_plan_entry_refuses_what_the_launching_entries_refuse(lib, golden):
    cases = _malformed(golden)
    assert len(cases) >= 10
    for what, d in cases:
        if d.n_classes:
            st = lib.rart_gemm_pair_classes_bf16(ctypes.byref(d), None)
        elif d.two.a2_hi or d.two.a2_lo:
            st = lib.rart_gemm_pair2_bf16(ctypes.byref(d.two), None)
        else:
            st = lib.rart_gemm_pair_bf16(ctypes.byref(d.two.one), None)
        msg = lib.rart_last_error_string()
        assert st == 1 and what.encode() in msg, (what, st, msg)
        out = _lib.GemmPairPlan()
        assert lib.rart_gemm_pair_plan_bf16(ctypes.byref(d), 256, ctypes.byref(out)) == st and lib.rart_last_error_string() == msg, what
    assert lib.rart_gemm_pair_plan_bf16(None, 256, None) == 1 and b'rart_gemm_pair_plan_bf16' in lib.rart_last_error_string()
