"""The stand-alone host programs of tests/stubs (a helper module, no tests): a product header compiled by g++ into a
program with its own main.  Nothing is loaded into Python or set in the environment: the sanitizers link statically."""
import os
import subprocess

from conftest import ROOT

FP = ["-O1", "-ffp-contract=off"]                               # contraction off, as the library
HIP_HOST = ["-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"]    # for headers that include hip_runtime.h
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"]


def build(name, out, flags=FP, sanitize=True):
    """tests/stubs/NAME.cpp compiled to `out` against csrc with `flags`; sanitize: with the address and
    undefined-behaviour sanitizers (every CPU test; a GPU test that only needs the program's bits goes without)."""
    subprocess.check_call(["g++", "-std=c++17", *flags, "-I", os.path.join(ROOT, "uclv_qs_pushing_matlab_amd", "csrc")] +
                          (SANITIZE if sanitize else []) +
                          ["-g", "-w", os.path.join(ROOT, "tests", "stubs", name + ".cpp"), "-o", str(out)])
    return str(out)
