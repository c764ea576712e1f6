"""Generate tests/golden/gemm1_parent_bits.npz: the fitnesses of every case of
tests/test_gpu_gemm1_bits.py as the library computes them on the GPU.

It was run once with TBLUP_GPU_LIB pointing at a build of the commit BEFORE the GEMM1 stage loop's
B-operand prefetch was reordered (tools/ab_build.sh builds it as ab/base.so):

    TBLUP_GPU_LIB=ab/base.so python tests/golden/make_gemm1_golden.py [out.npz]

so the file pins that commit's bits; regenerate it only when a change is meant to alter them.
Recorded results only, a few KB.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import test_gpu_gemm1_bits as G  # noqa: E402


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "gemm1_parent_bits.npz")
    panel = G.make_panel()
    out = {"geno_sum": np.int64(panel["geno"].astype(np.int64).sum())}
    for name in G.CASES:
        out[name] = np.asarray(G.run_case(panel, name), dtype=np.float64)
        print(name, out[name][:3])
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
