"""Writes tests/golden/twin_bits.npz: the kernel-order twin's outputs on the cases of
tests/twin_bits_cases.py, as raw 64-bit patterns.

The twin and the kernels evaluate one source of lane arithmetic (csrc/qsp_fp.hpp, qsp_math.hpp,
qsp_riccati.hpp, qsp_ipm.hpp), so a change of rounding order there moves both sides together and the GPU-vs-twin
comparison cannot see it; this fixture can.  Each case was written by the last twin that restated
the arithmetic it reaches by hand.  Regenerate it only when a change of the arithmetic is the intent:
    python tests/golden/make_twin_bits.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from twin_bits_cases import as_bits, run_cases  # noqa: E402

if __name__ == "__main__":
    out = {k: as_bits(v) for k, v in run_cases().items()}
    np.savez_compressed(os.path.join(HERE, "twin_bits.npz"), **out)
    print("twin_bits.npz:", len(out), "arrays")
