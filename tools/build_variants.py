"""Build instrumented variants of libnrhip.so into neurecon_amd/_exp/ (select one at run time with
NR_LIB=...).  `stamps` (NR_EXP_STAMPS) adds per-phase shader-clock totals to sdf4_kernel and
tgemm_kernel (tools/mlp_driver.py --stamps, tools/tg_driver.py --stamps): its results are valid, its
timing is not the product's.  `base` is the product's flags, for an A/B from the same tree."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from neurecon_amd import build as B  # noqa: E402

VARIANTS = {
    'base': [],
    'stamps': ['-DNR_EXP_STAMPS'],
    # every sdf4_kernel instance on one embed_feature / embed_backward call per row (the encoding before Enc4)
    'rowenc': ['-DNR_EXP_ROW_ENC'],
    'stamps_rowenc': ['-DNR_EXP_STAMPS', '-DNR_EXP_ROW_ENC'],
}


def one(name):
    out_dir = os.environ.get('NR_EXP_DIR', os.path.join(ROOT, 'neurecon_amd', '_exp'))
    objs = []
    for src in B._sources():
        obj = os.path.join(out_dir, f'{name}_{os.path.basename(src)}.o')
        subprocess.check_call([B.HIPCC] + B.flags_for(src) + ['-DNR_VARIANT_BUILD'] + VARIANTS[name] +
                              ['-c', src, '-o', obj])
        objs.append(obj)
    lib = os.path.join(out_dir, f'libnrhip_{name}.so')
    subprocess.check_call([B.HIPCC, '-shared', '-fPIC', f'--offload-arch={B.ARCH}', '-o', lib] + objs)
    return lib


def main(names):
    import concurrent.futures as cf
    os.makedirs(os.environ.get('NR_EXP_DIR', os.path.join(ROOT, 'neurecon_amd', '_exp')), exist_ok=True)
    with cf.ThreadPoolExecutor(4) as ex:
        for lib in ex.map(one, names):
            print(lib)


if __name__ == '__main__':
    main(sys.argv[1:] or list(VARIANTS))
