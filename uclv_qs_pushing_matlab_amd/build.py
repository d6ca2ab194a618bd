"""Build recipe for the HIP extension (libqsp_nmpc.so, gfx950).

hipcc compiles the kernels and the C-ABI into one shared library in-tree, so it
travels to the GPU box with the repository snapshot.
"""
import os
import subprocess
import sys

PKG = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(PKG, "csrc")
LIB = os.path.join(PKG, "libqsp_nmpc.so")
SOURCES = ["qsp_solver.hip", "qsp_sim.hip", "qsp_capi.hip", "qsp_rollout.hip", "qsp_openloop.hip", "qsp_kkt.hip",
           "qsp_sens.hip"]
HEADERS = ["qsp_math.hpp", "qsp_fp.hpp", "qsp_riccati.hpp", "qsp_ipm.hpp", "qsp_types.h", "qsp_kernels.h", "qsp_layout.h", "qsp_candidates.hpp",
           "qsp_devbuf.hpp", "qsp_noise.hpp", "qsp_kkt.hpp", "qsp_sens.hpp", "../../include/qsp_nmpc.h"]
ARCH = os.environ.get("QSP_OFFLOAD_ARCH", "gfx950")


# -greedy-regclass-priority-trumps-globalness: the register allocator assigns by register class
# before live-range globalness.  It changes only the S = 2 kernels' allocation (configs[4], which
# run at 256 VGPRs + ~200 AGPRs): 16 fewer AGPR copies per factor-walk step, scratch 68 -> 0 B/lane,
# 92.9k -> 94.5k solves/s, bit-identical (profiles/r04/ab_s2_regclass.txt); the S = 1 kernels'
# code is unchanged.
# -amdgpu-mfma-vgpr-form: the matrix-core factor walk's operands and results in VGPRs (the S = 1
# kernels keep two waves per SIMD only without AGPRs).
FLAGS = ["-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
         "-mllvm", "-greedy-regclass-priority-trumps-globalness", "-mllvm", "-amdgpu-mfma-vgpr-form"]


def source_digest():
    """Digest of what determines the kernels' code: the sources and headers with their comments
    and whitespace stripped, and the compile flags.  profiles/pmc_traffic.json records the digest
    its counters were collected at, and bench.py reports that traffic only while the library is
    built from the same code."""
    import hashlib
    import re
    h = hashlib.sha256(" ".join([ARCH] + FLAGS).encode())
    for f in SOURCES + HEADERS:
        with open(os.path.join(CSRC, f)) as fh:
            src = fh.read()
        src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)      # block comments
        src = re.sub(r"//[^\n]*", " ", src)                     # line comments
        h.update(" ".join(src.split()).encode())
    return h.hexdigest()[:16]


STAMP = LIB + ".digest"   # source_digest() of the build, so a change of FLAGS alone also rebuilds


def _stale():
    if not os.path.exists(LIB):
        return True
    try:
        with open(STAMP) as fh:
            if fh.read().strip() != source_digest():
                return True
    except OSError:
        return True
    t = os.path.getmtime(LIB)
    deps = [os.path.join(CSRC, f) for f in SOURCES + HEADERS]
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=False):
    if not force and not _stale():
        return LIB
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    # -ffp-contract=off: every fused multiply-add is an explicit fma() in the source, so the
    # oracle twin reproduces the device arithmetic bit for bit (qsp_fp.hpp)
    cmd = [hipcc, f"--offload-arch={ARCH}"] + FLAGS + ["-I", os.path.join(PKG, "..", "include")]
    cmd += [os.path.join(CSRC, f) for f in SOURCES]
    cmd += ["-o", LIB + ".tmp"]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.check_call(cmd)
    os.replace(LIB + ".tmp", LIB)
    with open(STAMP, "w") as fh:
        fh.write(source_digest() + "\n")
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
