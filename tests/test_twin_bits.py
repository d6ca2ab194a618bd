"""CPU: the twin's outputs against tests/golden/twin_bits.npz, in every bit.

The twin calls the kernels' own lane arithmetic (csrc/qsp_fp.hpp, qsp_math.hpp, qsp_riccati.hpp, qsp_ipm.hpp), so
the GPU-vs-twin comparison no longer notices a change of rounding order made there: both sides move
together.  This fixture, each case written by the last twin that restated that arithmetic by hand, does.  Every operation on
the path is one the host rounds deterministically (+ - * / sqrt fma, fmod, floor, rint; sin_cos and
rcp are the project's own sequences), so the bits depend neither on the machine nor on the OpenMP
thread count."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from twin_bits_cases import CASES, as_bits, run_cases


@pytest.fixture(scope="module")
def computed():
    return run_cases()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "twin_bits.npz"))


def test_fixture_covers_the_cases(computed, golden):
    assert sorted(golden.files) == sorted(computed)
    assert {k.split("/")[0] for k in golden.files} == set(CASES)


@pytest.mark.parametrize("case", sorted(CASES))
def test_twin_bits(case, computed, golden):
    keys = [k for k in golden.files if k.split("/")[0] == case]
    assert keys
    for k in keys:
        got, want = as_bits(computed[k]), golden[k]
        assert got.dtype == want.dtype and got.shape == want.shape, k
        assert np.array_equal(got, want), (
            f"{k}: {int((got != want).sum())} of {want.size} words differ from tests/golden/twin_bits.npz. "
            "The lane arithmetic shared by the kernels and the twin (csrc/qsp_fp.hpp, qsp_math.hpp, "
            "qsp_riccati.hpp, qsp_ipm.hpp) or the twin's orchestration changed its bits.  Regenerate the fixture "
            "(tests/golden/make_twin_bits.py) only if that change was the intent.")
