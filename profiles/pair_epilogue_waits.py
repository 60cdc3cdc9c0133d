"""Store drains in the pair epilogues, read from the device assembly (no GPU needed): compiles csrc/gemm_pair.hip, csrc/gemm_pair_pp.hip
and csrc/conv_tail_pair.hip of a tree for gfx950 with the flags of csrc/build.py and reports, per kernel instance,

  * the epilogue blocks / chunks: the stretches of the instruction stream between two wave barriers or workgroup barriers that hold
    global stores, each with its number of stores and the `s_waitcnt vmcnt(N)` instructions that lie between its first and its last store
    (loads and stores share the counter on gfx950: a vmcnt(0) there waits for every store issued so far), and the `vmcnt` waits between
    the block's first operand load (the first global load behind the previous store or workgroup barrier) and its first store: one is
    the block's own wait, more mean that operands are waited for one by one (a load round trip each, in series);
  * the global loads and stores of the kernel that carry the non-temporal hint (`nt`), beside all of them: the epilogue's streams are
    non-temporal under the descriptor's `nt`, and a compiler that merges the two arms of that choice drops the hint without a word;
  * VGPRs (and AGPRs), scratch bytes, LDS bytes and the occupancy the compiler states in the assembly's kernel footer (the figures
    `-Rpass-analysis=kernel-resource-usage` prints).

    python profiles/pair_epilogue_waits.py [--root TREE] [--label NAME] [--out FILE]

--out FILE merges the report into FILE under NAME (profiles/pair_epilogue_waits.json holds `parent` and `new`): per instance the totals
and the blocks that hold a wait.  A report, not a test."""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

FILES = ('gemm_pair.hip', 'gemm_pair_pp.hip', 'conv_tail_pair.hip')
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
STORE = re.compile(r'^\s*(global_store|buffer_store|flat_store)_')
WAIT = re.compile(r'^\s*s_waitcnt\b(.*)$')
VMCNT = re.compile(r'vmcnt\((\d+)\)')
FENCE = re.compile(r'^\s*(s_barrier\b|; wave barrier)')
LOAD = re.compile(r'^\s*global_load_')
HARD = re.compile(r'^\s*s_barrier\b')
STAT = {'vgprs': r'; NumVgprs: (\d+)', 'agprs': r'; NumAgprs: (\d+)', 'scratch_bytes': r'; ScratchSize: (\d+)',
        'lds_bytes': r'; LDSByteSize: (\d+)', 'occupancy_waves_per_simd': r'; Occupancy: (\d+)'}


def demangle(names):
    filt = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(HIPCC))), 'llvm', 'bin', 'llvm-cxxfilt')
    if not os.path.exists(filt):
        filt = shutil.which('llvm-cxxfilt') or shutil.which('c++filt') or filt
    try:
        out = subprocess.run([filt], input='\n'.join(names), capture_output=True, text=True, check=True).stdout.split('\n')
        return [re.sub(r'^void \(anonymous namespace\)::', '', o).replace('(anonymous namespace)::', '') for o in out[:len(names)]]
    except (OSError, subprocess.CalledProcessError):
        return list(names)


def kernels(asm):
    """-> [(mangled name, body lines)] of the .amdhsa kernels of a device assembly text"""
    names = re.findall(r'^\s*\.amdhsa_kernel (\S+)', asm, re.M)
    lines = asm.split('\n')
    out = []
    for n in names:
        b = next(i for i, l in enumerate(lines) if l.startswith(n + ':'))
        e = next(i for i in range(b, len(lines)) if lines[i].startswith('.Lfunc_end') or lines[i].strip().startswith('.section'))
        tail = next(i for i in range(e, len(lines)) if '; Occupancy:' in lines[i])
        out.append((n, lines[b:e], '\n'.join(lines[e:tail + 1])))
    return out


def vm_waits(lines):
    out = []
    for l in lines:
        m = WAIT.match(l)
        v = VMCNT.search(m.group(1)) if m else None
        if v:
            out.append(int(v.group(1)))
    return out


def blocks(body):
    """the store-holding stretches between barriers: [{stores, vmcnt_waits_between_first_and_last_store: [N, ...],
    vmcnt_waits_between_first_operand_load_and_first_store: [N, ...]}]"""
    out, cur, pre = [], [], []          # pre: the lines since the last store or workgroup barrier, over wave barriers
    for ln in body + ['s_barrier']:
        if FENCE.match(ln):
            st = [i for i, l in enumerate(cur) if STORE.match(l)]
            if st:
                before = pre + cur[:st[0]]
                first = next((i for i, l in enumerate(before) if LOAD.match(l)), len(before))
                out.append({'stores': len(st), 'vmcnt_waits_between_first_and_last_store': vm_waits(cur[st[0] + 1:st[-1]]),
                            'vmcnt_waits_between_first_operand_load_and_first_store': vm_waits(before[first:])})
                pre = cur[st[-1] + 1:]
            else:
                pre = [] if HARD.match(ln) else pre + cur
            cur = []
        else:
            cur.append(ln)
    return out


def report(root):
    csrc = os.path.join(root, 'robustart_amd', 'csrc')
    flags = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-I', os.path.join(root, 'include'), '--offload-device-only', '-S']
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        tmp = os.environ.get('RART_KEEP_ASM', tmp)         # (a directory that keeps the assembly texts)
        for f in FILES:
            s = os.path.join(tmp, f + '.s')
            subprocess.run([HIPCC] + flags + [os.path.join(csrc, f), '-o', s], check=True)
            ks = kernels(open(s).read())
            for (_, body, tail), name in zip(ks, demangle([k[0] for k in ks])):
                bl = blocks(body)
                e = {k: int(re.search(p, tail).group(1)) for k, p in STAT.items() if re.search(p, tail)}
                for what, pat in (('loads', LOAD), ('stores', STORE)):
                    hits = [l for l in body if pat.match(l)]
                    e['global_' + what] = len(hits)
                    e['nt_' + what] = sum(1 for l in hits if re.search(r'\bnt\b', l))
                e['store_blocks'] = len(bl)
                e['vmcnt_waits_inside_store_blocks'] = sum(len(b['vmcnt_waits_between_first_and_last_store']) for b in bl)
                e['full_drains_inside_store_blocks'] = sum(b['vmcnt_waits_between_first_and_last_store'].count(0) for b in bl)
                e['operand_waits_before_first_store'] = [len(b['vmcnt_waits_between_first_operand_load_and_first_store']) for b in bl]
                e['blocks_with_waits'] = [dict(b, block=i) for i, b in enumerate(bl) if b['vmcnt_waits_between_first_and_last_store'] or
                                          len(b['vmcnt_waits_between_first_operand_load_and_first_store']) > 1]
                res.setdefault(f, {})[name] = e
    return res


def write(doc, path):
    """the report as JSON, one line per kernel instance"""
    with open(path, 'w') as f:
        f.write('{\n')
        for i, (key, val) in enumerate(doc.items()):
            if isinstance(val, dict):
                f.write(' %s: {\n' % json.dumps(key))
                for j, (src, ks) in enumerate(val.items()):
                    rows = ['   %s: %s' % (json.dumps(k), json.dumps(e)) for k, e in ks.items()]
                    f.write('  %s: {\n%s\n  }%s\n' % (json.dumps(src), ',\n'.join(rows), ',' if j + 1 < len(val) else ''))
                f.write(' }')
            else:
                f.write(' %s: %s' % (json.dumps(key), json.dumps(val)))
            f.write(',\n' if i + 1 < len(doc) else '\n')
        f.write('}\n')


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument('--label', default='new')
    ap.add_argument('--out')
    a = ap.parse_args()
    rep = report(os.path.abspath(a.root))
    for f, ks in rep.items():
        for k, e in ks.items():
            print('%-20s %4d vgpr %4d agpr %6d scratch %7d lds | %2d store blocks, %2d vmcnt waits inside (%2d full), before the first store %s, nt %d / %d loads %d / %d stores | %s' % (
                f, e.get('vgprs', -1), e.get('agprs', -1), e.get('scratch_bytes', -1), e.get('lds_bytes', -1), e['store_blocks'],
                e['vmcnt_waits_inside_store_blocks'], e['full_drains_inside_store_blocks'], e['operand_waits_before_first_store'], e['nt_loads'], e['global_loads'], e['nt_stores'], e['global_stores'], k))
    if a.out:
        doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
        doc.setdefault('what', 'profiles/pair_epilogue_waits.py: per kernel instance, the s_waitcnt vmcnt(N) instructions between the first and '
                               'the last global store of each epilogue block / chunk (a stretch between two barriers), the number of vmcnt waits between a '
                               'block\'s first operand load and its first store (operand_waits_before_first_store), and the resources from the '
                               'assembly\'s kernel footer (what -Rpass-analysis=kernel-resource-usage prints); nt_loads / nt_stores: the global loads / '
                               'stores with the non-temporal hint; the stream is read in text order, so both arms of a branch are counted (the '
                               'non-temporal and the ordinary form of a load group each carry their wait)')
        doc[a.label] = rep
        write(doc, a.out)
        sys.stderr.write('wrote %s [%s]\n' % (a.out, a.label))
