"""Record tests/golden/stat_sgd_bits.npz: the output bits of the BatchNorm statistics kernels and the SGD update on the
cases of tests/stat_sgd_cases.py (tests/test_hip_stat_sgd_bits.py compares against them).  Only outputs are stored; the
inputs are regenerated from seeds.  Run on the GPU with the library to pin selected through KODHIP_LIB, e.g. the parent
commit's build before a refactor of these kernels:

    KODHIP_LIB=/path/to/parent/libkodhip.so python tools/record_stat_sgd_bits.py [out.npz]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import stat_sgd_cases as cases  # noqa: E402
from object_detection_cib_amd import _lib  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "stat_sgd_bits.npz")
    lib, arrays = _lib.lib(), {}
    for fam in cases.FAMILIES:
        res = fam(lib)
        arrays.update({k: v.numpy() for k, v in res.items()})
        arrays["count__" + fam.__name__] = np.array(len(res))
    np.savez_compressed(out, **arrays)
    print(f"{out}: {len(arrays)} arrays, {os.path.getsize(out)} bytes, library {_lib.LIB_PATH}")


if __name__ == "__main__":
    main()
