"""CPU: csrc/qsp_noise.hpp itself, compiled for the host in a program of its own (tests/stubs/noise_main.cpp; the
header's functions are __host__ __device__): its Philox4x32-10 gives the published known answers, and its noise
equals the numpy restatement within the bound the GPU test uses, 1e-13 sigma scale -- the argument rounding of
cos(2 pi u) is <= 7e-16, the libm errors a few ulp, times |r| <= 6.76: about 1e-14.  Built with the address and
undefined-behaviour sanitizers, as tests/test_devbuf.py builds its program.  Nothing is loaded into Python."""
import subprocess

import numpy as np

import host_program
from sim_noise_ref import sim_noise


def test_header_on_the_host(tmp_path):
    exe = tmp_path / "noise_main"
    host_program.build("noise_main", exe, flags=host_program.FP + host_program.HIP_HOST)
    seed, stream, step0, lane0, T, B = 0x9E3779B97F4A7C15, 3, 2 ** 32 - 2, 2 ** 31 + 5, 5, 7
    r = subprocess.run([str(exe)] + [str(v) for v in (seed, stream, step0, lane0, T, B)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.split("\n")
    assert lines[0] == "noise ok", r.stdout
    got = np.array([[float.fromhex(v) for v in ln.split()] for ln in lines[1:1 + T * B]]).reshape(T, B, 4)
    sigma, scale = np.array([1.0, 2.0, 3.0, 4.0]), np.arange(B) % 3
    ref = sim_noise(seed, T, B, sigma=sigma, lane_scale=scale, stream=stream, step_offset=step0, lane_offset=lane0)
    bound = 1e-13 * sigma[None, None, :] * scale[None, :, None]
    err = np.abs(got - ref)
    print("max |n - n_ref| / (sigma scale) = %.2e" % (err[:, scale > 0] / bound[:, scale > 0] * 1e-13).max())
    assert np.all(err <= bound)
    assert np.all(got[:, scale == 0] == 0.0) and np.abs(got).max() > 1.0
