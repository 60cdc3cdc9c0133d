"""Record tests/golden/pair_epilogue_bits.json: per case of tests/test_pair_epilogue_bits_gpu.py a sha256 of the input bytes and one of
every whole output buffer (the guard behind it and the gap between the planes of a pair included), with the commit the library was
built from and torch.version.hip.  Needs a GPU.

    python tests/golden/make_pair_epilogue_bits.py --commit HASH [--lib PATH] [--out PATH]

The committed file was recorded from the library of the commit BEFORE gp_epilogue (csrc/rart_gemm_pair_dev.h) was given its counted
vmcnt wait per block and its straight-line operand loads, and the conv instances lost the GELU forms, so the test pins the new
epilogue against the old one, not against itself.  It is not re-recorded after a kernel edit: a mismatch is a change of the
arithmetic and is fixed in the code."""
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
    ap.add_argument('--out', default=os.path.join(HERE, 'pair_epilogue_bits.json'))
    args = ap.parse_args()
    import torch
    from robustart_amd import _lib
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    import test_pair_epilogue_bits_gpu as T
    cases = {}
    for case in T.CASES:
        cases[T.case_id(case)] = T.run_case(case)
        print(T.case_id(case), flush=True)
    with open(args.out, 'w') as f:
        json.dump({'what': 'sha256 of the input bytes and of each whole output buffer, little endian; outputs pre-filled with 0x7FA5 '
                           '(fp32: 0x7FA57FA5, bytes: 0xA5)',
                   'commit': args.commit, 'hip': torch.version.hip, 'cases': cases}, f, indent=1, sort_keys=True)
        f.write('\n')


if __name__ == '__main__':
    main()
