"""numpy restatement of csrc/qsp_noise.hpp (include/qsp_nmpc.h, "sim_noise generated on the device"), vectorised
over (step, lane): Philox4x32-10 bits, uniforms (w + 0.5) 2^-32, Box-Muller normals, n = (sigma * scale) * z."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
SIGMA = np.array([1e-5, 1e-5, 1e-3, 1e-4])        # helper.m:241


def philox4x32_10(ctr, key):
    """ctr (..., 4), key (..., 2) of 32-bit words (any integer dtype) -> (..., 4) uint32."""
    c = [np.asarray(ctr)[..., j].astype(np.uint64) & MASK for j in range(4)]
    k = [np.asarray(key)[..., j].astype(np.uint64) & MASK for j in range(2)]
    for r in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]               # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + np.uint64(W0)) & MASK, (k[1] + np.uint64(W1)) & MASK]
    return np.stack(c, -1).astype(np.uint32)


def words(seed, n_steps, B, stream=0, step_offset=0, lane_offset=0):
    """The four output words of every (step t, lane i): (n_steps, B, 4) uint32.  Counter (uint32(lane_offset + i),
    step low, step high, stream) with step = step_offset + t; key (seed low, seed high)."""
    step = np.array([int(step_offset) + t for t in range(n_steps)], dtype=object)
    lo = np.array([int(v) & 0xFFFFFFFF for v in step], np.uint64)
    hi = np.array([(int(v) >> 32) & 0xFFFFFFFF for v in step], np.uint64)
    lane = np.array([(int(lane_offset) + i) & 0xFFFFFFFF for i in range(B)], np.uint64)
    ctr = np.empty((n_steps, B, 4), np.uint64)
    ctr[..., 0] = lane[None, :]
    ctr[..., 1] = lo[:, None]
    ctr[..., 2] = hi[:, None]
    ctr[..., 3] = int(stream) & 0xFFFFFFFF
    key = np.array([int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF], np.uint64)
    return philox4x32_10(ctr, np.broadcast_to(key, (n_steps, B, 2)))


def normals(w):
    """(..., 4) uint32 words -> (..., 4) standard normals."""
    u = (w.astype(np.float64) + 0.5) * 2.0 ** -32
    z = np.empty(u.shape)
    for j in (0, 2):
        r = np.sqrt(-2.0 * np.log(u[..., j]))
        a = (2.0 * np.pi) * u[..., j + 1]
        z[..., j] = r * np.cos(a)
        z[..., j + 1] = r * np.sin(a)
    return z


def sim_noise(seed, n_steps, B, sigma=None, lane_scale=None, stream=0, step_offset=0, lane_offset=0):
    """The table qsp_gen_sim_noise writes: (n_steps, B, 4)."""
    sigma = SIGMA if sigma is None else np.asarray(sigma, np.float64).reshape(4)
    scale = np.ones(B) if lane_scale is None else np.broadcast_to(np.asarray(lane_scale, np.float64), (B,))
    z = normals(words(seed, n_steps, B, stream, step_offset, lane_offset))
    return (sigma[None, None, :] * scale[None, :, None]) * z
