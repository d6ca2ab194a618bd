"""The closed-loop lane walks as pipelines under one exec mask (riccati_solve<1, ...> in qsp_solver.hip), modelled
in numpy on the 64 lanes of a wavefront.  A step forms n = M v + c in every enabled lane from the lane's own M, c
and its current v, and hands n to the neighbour: the destination takes it only where source and destination are
both enabled, and keeps its old value otherwise (a DPP move from a disabled or missing lane).  The kernels used
to run step j under its own mask (lig <= j backwards for j = L - 2 .. 1, j <= lig < L - 1 forwards for
j = 0 .. L - 2); they now run L - 2 steps under the first of those masks.  Both must leave the same bits in every
lane with lig <= L - 2, for every L = 2 .. 64 and both directions, with the masks read from qsp_layout.h itself by
a small C++ program (in the manner of test_lane_masks.py).

Every lane has data of its own, so the instances of a wave differ.  With NaN in every lane of one whole instance
(its terminal lane included) and in the padding lanes behind the last instance, the other instances keep the bits
of the clean wave: nothing crosses an instance boundary.
"""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "uclv_qs_pushing_matlab_amd", "csrc")
WAVE = 64
LS = list(range(2, 65))

PROG = r"""
#include <cstdio>
#include "qsp_layout.h"
using namespace qsp;
int main() {
    for (int L = 2; L <= 64; ++L) {
        const int N = L - 1;
        if (lanes_per_instance(N, 1) != L) return 1;
        for (int j = 0; j < L; ++j)
            std::printf("%d %d %llx %llx\n", L, j, lane_mask_lig_le(N, 1, j), lane_mask_walk_fwd(N, 1, j));
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def masks(tmp_path_factory):
    """(L, j) -> (lig <= j, j <= lig < L - 1) as boolean lane vectors, from the header."""
    d = tmp_path_factory.mktemp("walk_pipeline")
    src, exe = d / "masks.cpp", d / "masks"
    src.write_text(PROG)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    lanes = np.arange(WAVE, dtype=np.uint64)
    res = {}
    for ln in out.splitlines():
        L, j, le, fwd = ln.split()
        res[int(L), int(j)] = tuple(((np.uint64(int(m, 16)) >> lanes) & np.uint64(1)).astype(bool) for m in (le, fwd))
    assert len(res) == sum(LS)
    return res


def wave_data(L, seed, nan_lanes=()):
    """Per-lane M (a contraction, so 62 steps stay finite), c and the start value v."""
    rng = np.random.default_rng(seed)
    M = rng.uniform(-0.4, 0.4, (WAVE, 4, 4))
    c = rng.uniform(-1.0, 1.0, (WAVE, 4))
    v = rng.uniform(-1.0, 1.0, (WAVE, 4))
    for a in (M, c, v):
        a[list(nan_lanes)] = np.nan
    return M, c, v


def step(M, c, v, mask, shift):
    """One step under `mask`: lane i takes lane i + shift's n where both are enabled."""
    with np.errstate(invalid="ignore"):
        n = c + np.einsum("lij,lj->li", M, v)
    out = v.copy()
    for i in range(WAVE):
        s = i + shift
        if mask[i] and 0 <= s < WAVE and mask[s]:
            out[i] = n[s]
    return out


def walk(masks, L, data, backward, one_mask):
    M, c, v = data
    if backward:
        js = range(L - 2, 0, -1)
        ms = [masks[L, L - 2][0] if one_mask else masks[L, j][0] for j in js]
    else:
        js = range(0, L - 2) if one_mask else range(0, L - 1)
        ms = [masks[L, 0][1] if one_mask else masks[L, j][1] for j in js]
    for m in ms:
        v = step(M, c, v, m, +1 if backward else -1)
    return v


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def read_lanes(L):
    """The lanes whose walk value the kernels read: lig <= L - 2."""
    return (np.arange(WAVE) % L) <= L - 2


@pytest.mark.parametrize("backward", [False, True], ids=["forward", "backward"])
def test_one_mask_gives_the_bits_of_the_per_step_masks(masks, backward):
    for L in LS:
        data = wave_data(L, 1000 + L)
        old = walk(masks, L, data, backward, one_mask=False)
        new = walk(masks, L, data, backward, one_mask=True)
        rd = read_lanes(L)
        assert np.isfinite(old[rd]).all(), L
        assert np.array_equal(bits(old)[rd], bits(new)[rd]), (L, np.argwhere(bits(old) != bits(new))[:4])
        # the terminal lanes never move, the chain's first lane is pinned at its start value
        term = ~rd
        pinned = (np.arange(WAVE) % L) == (L - 2 if backward else 0)
        for w in (old, new):
            assert np.array_equal(bits(w)[term], bits(data[2])[term]), L
            assert np.array_equal(bits(w)[pinned], bits(data[2])[pinned]), L


@pytest.mark.parametrize("backward", [False, True], ids=["forward", "backward"])
def test_a_nan_instance_stays_in_its_lanes(masks, backward):
    for L in LS:
        G = WAVE // L
        grp = np.arange(WAVE) // L
        clean = wave_data(L, 2000 + L)
        ref = walk(masks, L, clean, backward, one_mask=True)
        for g in sorted({0, G // 2, G - 1}):
            nan_lanes = np.flatnonzero((grp == g) | (grp >= G))     # one whole instance, and the padding lanes
            data = wave_data(L, 2000 + L, nan_lanes)
            healthy = np.ones(WAVE, bool)
            healthy[nan_lanes] = False
            old = walk(masks, L, data, backward, one_mask=False)
            new = walk(masks, L, data, backward, one_mask=True)
            rd = read_lanes(L)
            assert np.array_equal(bits(old)[rd], bits(new)[rd]), (L, g)
            for w in (old, new):
                assert np.array_equal(bits(w)[healthy], bits(ref)[healthy]), (L, g)
                assert np.isfinite(w[healthy]).all(), (L, g)
