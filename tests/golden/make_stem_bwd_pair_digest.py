"""Record tests/golden/stem_bwd_pair_digest.json: the SHA-256 of the fp32 gradient bytes rart_engine_stem_bwd_fused_pair writes for the
cases of tests/test_stem_pair_kernels_gpu.py (fixed seeds, a fixed random weight table).  Needs a GPU.

    python tests/golden/make_stem_bwd_pair_digest.py [--lib PATH] [--out PATH]

The committed file was recorded from the library of the commit BEFORE the kernel's pool-tile layout, load order and weight path changed (--lib
points at such a build), so the test pins "same products, same order, same rounding points" against that kernel, not against itself.
Re-record only when a change of the summation order is intended, and say so."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--lib', default=None, help='shared library to record from (default: the built product)')
    ap.add_argument('--out', default=os.path.join(HERE, 'stem_bwd_pair_digest.json'))
    args = ap.parse_args()
    from robustart_amd import _lib
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    import test_stem_pair_kernels_gpu as T
    table = T.stem_bwd_table()
    out = {}
    for size in T.SIZES:
        for codes in T.CODES:
            out[T.digest_key(size, codes)] = T.digest(T.stem_bwd_direct(size, codes, table))
            print(T.digest_key(size, codes), out[T.digest_key(size, codes)], flush=True)
    with open(args.out, 'w') as f:
        json.dump({'kernel': 'rart_engine_stem_bwd_fused_pair', 'what': 'sha256 of the fp32 gradient [n][3][h][w], little endian',
                   'sha256': out}, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
