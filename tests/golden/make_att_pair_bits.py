"""Record tests/golden/att_pair_bits.json: per case of tests/test_att_pair_bits_gpu.py a sha256 of the input bytes and one of every
whole output buffer, with the commit the library was built from and torch.version.hip.  Needs a GPU.

    python tests/golden/make_att_pair_bits.py --commit HASH [--lib PATH] [--out PATH]

The committed file was recorded from the library of the commit BEFORE the one-item and the walking pair attention kernels got their
per-tile arithmetic from shared helpers, so the test pins the shared text against the two separate copies, not against itself.  The
walking and the one-item kernels must agree at the shapes both run, or nothing is written.  It is not re-recorded after a kernel
edit: a mismatch is a change of the arithmetic and is fixed in the code."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--commit', required=True, help='the commit the library was built from')
    ap.add_argument('--lib', default=None, help='shared library to record from (default: the built product)')
    ap.add_argument('--out', default=os.path.join(HERE, 'att_pair_bits.json'))
    args = ap.parse_args()
    import torch
    from robustart_amd import _lib
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    import test_att_pair_bits_gpu as T
    cases = {}
    for case in T.CASES:
        cases[T.case_id(case)] = T.run_case(case)
        print(T.case_id(case), flush=True)
    for case in T.CASES:
        if case[1] == 'walk':
            one = (case[0], 'one') + case[2:]
            assert cases[T.case_id(case)] == cases[T.case_id(one)], 'the walking and the one-item kernels differ at %s' % T.case_id(case)
    with open(args.out, 'w') as f:
        json.dump({'what': 'sha256 of the input bytes and of each whole output buffer, little endian; outputs pre-filled with 0x7FA5, '
                           'the fp32 statistics with 0x7FA57FA5',
                   'commit': args.commit, 'hip': torch.version.hip, 'cases': cases}, f, indent=1, sort_keys=True)
        f.write('\n')


if __name__ == '__main__':
    main()
