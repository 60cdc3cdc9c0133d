"""Lab builds of the library with another csrc/stem_pair.hip or other defines for it (the product build is untouched):

    python profiles/stem_pair_lab_build.py OUT.so [-DRART_STEM_STAMPS] [-DRART_STEM_U8_PREFETCH=1] [--source OTHER_stem_pair.hip]

Links the product's cached objects (robustart_amd/csrc/_obj, so build the product first) with the one recompiled file.  --source takes
the file of another commit (`git show REV:robustart_amd/csrc/stem_pair.hip > f`) for a parent build to A/B against."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from robustart_amd.csrc import build as B      # noqa: E402


def main(argv):
    out, defs, src = argv[0], [a for a in argv[1:] if a.startswith('-D')], os.path.join(B.HERE, 'stem_pair.hip')
    if '--source' in argv:
        src = argv[argv.index('--source') + 1]
    obj = out + '.stem_pair.o'
    subprocess.check_call([B.HIPCC] + B.FLAGS + ['-I', B.HERE] + defs + ['-c', src, '-o', obj])
    objs = [os.path.join(B.OBJ, f + '.o') for f in B.sources() if f != 'stem_pair.hip']
    subprocess.check_call([B.HIPCC, '--offload-arch=gfx950', '-shared', '-fPIC', '-o', out] + objs + [obj])
    os.remove(obj)
    print('built', out)


if __name__ == '__main__':
    main(sys.argv[1:])
