"""CPU: the C ABI's typed device buffers and array shapes (csrc/qsp_devbuf.hpp), in a program of their own.

tests/stubs/devbuf_main.cpp includes the header, stands in for hipMalloc / hipFree / hipMemcpyAsync /
hipMemsetAsync with counting versions over malloc, and is built with the address and undefined-behaviour
sanitizers: ensure() keeps or replaces with one free, every destructor path ends with nothing live, a copy or
fill above the capacity is an error that touches nothing, and Dims equals the shapes of qsp_kernels.h's comments
at (B, N) = (5, 10) and (3, 32).  Nothing is loaded into Python."""
import subprocess

import host_program


def test_devbuf_program(tmp_path):
    exe = tmp_path / "devbuf_main"
    host_program.build("devbuf_main", exe, flags=host_program.HIP_HOST)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("devbuf ok:"), r.stdout
