"""CPU: tests/sim_noise_ref.py, the numpy restatement of the device generator (csrc/qsp_noise.hpp), against the
published Philox4x32-10 known answers, the counter layout of include/qsp_nmpc.h, and the moments of what it draws.
The GPU tests compare the device against this file (tests/test_gpu_sim_noise.py)."""
import numpy as np

from sim_noise_ref import normals, philox4x32_10, sim_noise, words


def _hex(s):
    return np.array([int(v, 16) for v in s.split()], np.uint64)


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32-10: zeros, all ones, the digits of pi."""
    kat = [("00000000 00000000 00000000 00000000", "00000000 00000000", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for ctr, key, out in kat:
        np.testing.assert_array_equal(philox4x32_10(_hex(ctr), _hex(key)), _hex(out).astype(np.uint32))
    # vectorised: the three at once
    got = philox4x32_10(np.stack([_hex(c) for c, _, _ in kat]), np.stack([_hex(k) for _, k, _ in kat]))
    np.testing.assert_array_equal(got, np.stack([_hex(o) for _, _, o in kat]).astype(np.uint32))


def test_counter_layout():
    seed = 0x0123456789ABCDEF
    base = words(seed, 1, 1, stream=2, step_offset=5, lane_offset=7)[0, 0]
    # the layout itself: counter (lane, step low, step high, stream), key (seed low, seed high)
    np.testing.assert_array_equal(base, philox4x32_10(np.array([7, 5, 0, 2]), np.array([0x89ABCDEF, 0x01234567])))
    big = words(seed, 1, 1, stream=2, step_offset=5 + (3 << 32), lane_offset=7)[0, 0]
    np.testing.assert_array_equal(big, philox4x32_10(np.array([7, 5, 3, 2]), np.array([0x89ABCDEF, 0x01234567])))
    # every field moves the words
    others = [words(seed, 1, 1, stream=2, step_offset=5, lane_offset=8)[0, 0],             # lane
              big,                                                                          # step across 2^32
              words(seed, 1, 1, stream=3, step_offset=5, lane_offset=7)[0, 0],             # stream
              words(seed ^ 1, 1, 1, stream=2, step_offset=5, lane_offset=7)[0, 0],         # seed, low half
              words(seed ^ (1 << 32), 1, 1, stream=2, step_offset=5, lane_offset=7)[0, 0]]  # seed, high half
    for o in others:
        assert not np.any(o == base)      # four 32-bit words: a chance equality is 1e-9 per word
    assert len({tuple(o) for o in others}) == len(others)
    # lanes and steps of one table are the lane and step fields
    w = words(seed, 3, 4, stream=2, step_offset=5, lane_offset=7)
    np.testing.assert_array_equal(w[2, 3], words(seed, 1, 1, stream=2, step_offset=7, lane_offset=10)[0, 0])
    # step_offset = a, t = b is step_offset = 0, t = a + b; across the word boundary too
    for a, b in ((4, 2), (2 ** 32 - 2, 3)):
        np.testing.assert_array_equal(words(seed, b + 1, 2, step_offset=a)[b],
                                      words(seed, 1, 2, step_offset=a + b)[0])
    np.testing.assert_array_equal(words(seed, 7, 2)[4:7], words(seed, 3, 2, step_offset=4))


def test_uniforms_and_normals_at_the_extremes():
    """u = (w + 0.5) 2^-32 is never 0 or 1: the normals stay finite, |z| <= sqrt(2 ln 2^33) = 6.76."""
    w = np.array([[0, 0, 0xFFFFFFFF, 0xFFFFFFFF], [0xFFFFFFFF, 0, 0, 0x80000000]], np.uint32)
    z = normals(w)
    assert np.all(np.isfinite(z))
    bound = np.sqrt(2.0 * np.log(2.0 ** 33))
    assert abs(bound - 6.76) < 0.01 and np.abs(z).max() <= bound
    assert abs(np.abs(z[0, :2]).max() - bound) < 1e-9      # w0 = 0: the largest radius


def test_moments():
    """64 lanes x 64 steps, seed 20250303: |mean| < 4 / sqrt(n), std within 4 / sqrt(2 n) of 1, |corr| < 4 / sqrt(n)
    between components, all finite.  (Measured on this file alone: max |mean| 0.0124, std 0.981 to 1.021,
    max |corr| 0.024, max |z| 4.19.)"""
    n = 64 * 64
    z = normals(words(20250303, 64, 64)).reshape(n, 4)
    assert np.all(np.isfinite(z))
    mean, std = z.mean(0), z.std(0)
    corr = np.corrcoef(z.T) - np.eye(4)
    print("max |mean| %.4f, std %.3f to %.3f, max |corr| %.3f, max |z| %.2f"
          % (np.abs(mean).max(), std.min(), std.max(), np.abs(corr).max(), np.abs(z).max()))
    assert np.abs(mean).max() < 4.0 / np.sqrt(n)             # 0.0625
    assert np.abs(std - 1.0).max() < 4.0 / np.sqrt(2.0 * n)  # 4.4 %
    assert np.abs(corr).max() < 4.0 / np.sqrt(n)


def test_scaling():
    sigma = np.array([2.0, 0.0, 1e-3, 5.0])
    scale = np.array([1.0, 0.0, 0.25])
    n = sim_noise(9, 4, 3, sigma=sigma, lane_scale=scale, stream=1)
    z = normals(words(9, 4, 3, stream=1))
    np.testing.assert_array_equal(n, (sigma[None, None, :] * scale[None, :, None]) * z)
    assert np.all(n[:, 1] == 0.0) and np.all(n[..., 1] == 0.0)
    # the defaults: the reference's sigma (helper.m:241), scale 1
    np.testing.assert_array_equal(sim_noise(9, 4, 3), np.array([1e-5, 1e-5, 1e-3, 1e-4]) * normals(words(9, 4, 3)))
