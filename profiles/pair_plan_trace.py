"""The pair GEMM's launches as the GPU sees them, for a library given by path: every case of tests/golden/pair_plan.json once at the
default schedule, then five of them under schedules 0, 2 and 3, on zero-filled buffers.

    rocprofv3 --kernel-trace -f csv -d DIR -o NAME -- python profiles/pair_plan_trace.py run LIBRARY [PLANS.json]
    python profiles/pair_plan_trace.py compare PARENT_kernel_trace.csv NEW_kernel_trace.csv PLANS.json profiles/pair_plan_trace.json

`run` issues the launches (and, where the library has rart_gemm_pair_plan_bf16, writes what it reports for each of them to PLANS.json);
`compare` reads the two kernel traces and checks that the ordered lists of (kernel, grid, workgroup, LDS bytes) are equal and that the
new library's list is what its plans say.  Exit status 1 on any difference."""
import csv
import ctypes
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
_spec = importlib.util.spec_from_file_location('make_pair_plan', os.path.join(ROOT, 'tests', 'golden', 'make_pair_plan.py'))
mpp = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mpp)

MARGIN = 256 << 20
OTHER_SCHEDULES = (0, 2, 3)
OTHER_SHAPES = ('50176 x 1024 -> 512 conv 1 taps', '50176 x 768 -> 1024 conv 1 taps two sources',
                '12544 x 4096 -> 1024 conv 4 taps two sources 4 classes', '50432 x 768 -> 2304', '50432 x 3072 -> 768')


def jobs(cases):
    """(case, schedule) in issue order"""
    out = [(c, 1) for c in cases]
    for name in OTHER_SHAPES:
        c = next(c for c in cases if c['name'] == name)
        out += [(c, s) for s in OTHER_SCHEDULES]
    return out


def extent(case):
    """an upper bound of the bytes any plane of the case spans from its base address"""
    o = case['one']
    out_b = 4 if o['flags'] & 2 else 2
    w = (o['w_rows'] if o['w_rows'] > 0 else o['N']) * o['ldw'] * 2
    if o['conv']:
        a = o['batch'] * o['src_h'] * o['src_w'] * o['lda'] * 2
        t = case.get('two')
        a2 = o['batch'] * t['src2_h'] * t['src2_w'] * t['lda2'] * 2 if t else 0
        return max(a, a2, w, o['batch'] * o['dst_h'] * o['dst_w'] * o['ldc'] * out_b)
    M, rpi = o['M'], o['rows_per_image']
    imgs = -(-M // rpi) if 0 < rpi < M else 1
    per = max(rpi, o['src_rows_per_image'], o['dst_rows_per_image'])
    rows = (imgs * per if imgs > 1 else M) + o['src_row_off'] + o['dst_row_off']
    nz, zi = max(o['n_batched'], 1), max(o['z_inner'], 1)
    zo_max, zi_max = (nz - 1) // zi, zi - 1

    def z(outer, inner):
        return zo_max * o[outer] + zi_max * o[inner]
    return max((rows * o['lda'] + z('a_z_outer', 'a_z_inner')) * 2, w + z('w_z_outer', 'w_z_inner') * 2,
               (rows * o['ldc'] + z('c_z_outer', 'c_z_inner')) * out_b)


def desc_on(case, base):
    """the case's descriptor with every plane at `base` (all operands zero, so every output is zero: the planes may share memory)"""
    d = mpp.to_desc(case)
    one = d.two.one
    for n in case['planes']:
        setattr(one, n, base)
    if 'two' in case:
        d.two.a2_hi = d.two.a2_lo = base
    return d


def run(lib_path, plans_out=None):
    import torch
    lib = ctypes.CDLL(lib_path)
    lib.rart_last_error_string.restype = ctypes.c_char_p
    cases = mpp.load()['cases']
    need = max(extent(c) for c in cases)
    assert need < (16 << 30), need
    buf = torch.zeros(need + 2 * MARGIN, dtype=torch.uint8, device='cuda')
    base = buf.data_ptr() + MARGIN
    torch.cuda.synchronize()
    has_plan = hasattr(lib, 'rart_gemm_pair_plan_bf16')
    plans = []
    for case, schedule in jobs(cases):
        assert lib.rart_gemm_pair_set_schedule(schedule) == 0
        d = desc_on(case, base)
        if has_plan:
            plans.append(dict(name=case['name'], schedule=schedule, conv=case['one']['conv'], two='two' in case, classes='classes' in case,
                              launches=mpp.plan(lib, d, 0)))
        if 'classes' in case:
            st = lib.rart_gemm_pair_classes_bf16(ctypes.byref(d), None)
        elif 'two' in case:
            st = lib.rart_gemm_pair2_bf16(ctypes.byref(d.two), None)
        else:
            st = lib.rart_gemm_pair_bf16(ctypes.byref(d.two.one), None)
        assert st == 0, (case['name'], schedule, lib.rart_last_error_string())
        torch.cuda.synchronize()
    assert not buf[::4096].any()
    if has_plan and plans_out:
        json.dump(plans, open(plans_out, 'w'))
    print('issued %d pair GEMM calls from %s' % (len(jobs(cases)), lib_path))


def launches(trace_csv):
    """the pair GEMM dispatches of a rocprofv3 kernel trace, in dispatch order: [kernel, grid (workgroups), workgroup, LDS bytes]"""
    rows = [r for r in csv.DictReader(open(trace_csv)) if 'k_gemm_pair' in r['Kernel_Name']]
    rows.sort(key=lambda r: int(r['Dispatch_Id']))
    lds = next(k for k in rows[0] if k.startswith('LDS'))
    out = []
    for r in rows:
        wg = [int(r['Workgroup_Size_' + a]) for a in 'XYZ']
        grid = [int(r['Grid_Size_' + a]) // w for a, w in zip('XYZ', wg)]          # the trace counts work-items
        out.append([r['Kernel_Name'], grid, wg, int(r[lds])])
    return out


def planned(plans):
    """what the plans say the trace holds: [kernel name with template arguments, grid, workgroup]"""
    b = ('false', 'true')
    out = []
    for p in plans:
        for r in p['launches']:
            conv, two, cls = b[bool(p['conv'])], b[p['two'] or p['classes']], b[p['classes']]      # (the class instances are two-source instances)
            if r['family'] == 0:
                name = 'k_gemm_pair<%d, %d, %s, %s, %s>' % (r['tile_m'], r['tile_n'], conv, two, cls)
            elif r['family'] == 1:
                name = 'k_gemm_pair_pp<%d, %s, %d, %s, %s>' % (r['tile_n'], conv, 3 if r['walk_wgs'] else 1, two, cls)
            else:
                name = 'k_gemm_pair_ps<%s>' % conv
            out.append([name, [r['grid_x'], r['grid_y'], 1], [r['block'], 1, 1]])
    return out


def compare(parent_csv, new_csv, plans_json, out_json):
    old, new, plans = launches(parent_csv), launches(new_csv), json.load(open(plans_json))
    want = planned(plans)

    def bare(name):          # 'void (anonymous namespace)::k<...>(GemmPairDev)' -> 'k<...>'
        name = name.replace('(anonymous namespace)::', '').replace('void ', '')
        return name[:name.rindex('>') + 1]
    same = old == new
    as_planned = [[bare(n), g, w] for n, g, w, _ in new] == want
    json.dump(dict(jobs=[[p['name'], p['schedule']] for p in plans], parent=old, new=new, planned=want,
                   parent_equals_new=same, new_equals_plan=as_planned), open(out_json, 'w'), indent=0)
    print('%d launches (parent), %d (new); parent == new: %s; new == plan: %s' % (len(old), len(new), same, as_planned))
    if not same:
        for i, (a, c) in enumerate(zip(old, new)):
            if a != c:
                print('first difference at launch %d:\n  parent %s\n  new    %s' % (i, a, c))
                break
    if not as_planned:
        for i, (a, c) in enumerate(zip([[bare(n), g, w] for n, g, w, _ in new], want)):
            if a != c:
                print('first difference from the plan at launch %d:\n  traced  %s\n  planned %s' % (i, a, c))
                break
    return 0 if same and as_planned else 1


if __name__ == '__main__':
    if sys.argv[1] == 'run':
        run(*sys.argv[2:4])
    else:
        sys.exit(compare(*sys.argv[2:6]))
