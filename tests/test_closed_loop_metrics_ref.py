"""CPU: the numpy reference of the closed-loop metrics (tests/closed_loop_metrics_ref.py) on a hand-made
trajectory of three steps whose ten metrics are written out by hand.  Every number is a small dyadic
rational, so each product and sum below is exact and the expected values are plain decimals."""
import numpy as np

from closed_loop_metrics_ref import NAMES, closed_loop_metrics_ref, ref_rows

# reference table, 3 columns of [x y theta s u_n u_t]
TRAJ = np.array([[0.0, 0.0, 0.0, 0, 0, 0],
                 [1.0, 0.0, 0.0, 0, 0, 0],
                 [2.0, 0.0, 0.5, 0, 0, 0]])
S_LO, S_HI = -0.06, 0.011

# lane 0 starts at column 2: steps read columns 2, 3, 3 (clamped), the final state column 5 -> 3
# lane 1 starts at column 1: steps read columns 1, 2, 3, the final state column 4 -> 3
X = np.array([[[1.5, 0.5, 0.25, 0.0], [2.0, 1.0, 0.5, -0.1], [3.0, 0.0, 1.5, 0.02], [2.5, 0.5, 0.0, 0.0]],
              [[0.0, 0.0, 0.0, 0.0], [1.0, 2.0, 0.0, 0.0], [2.0, 0.0, 0.5, 0.011], [4.0, 0.0, 9.0, 9.0]]])
U = np.array([[[0.5, 0.25], [1.0, 0.0], [0.0, 0.5]],
              [[0.0, 0.0], [0.0, 0.0], [0.0, 0.0]]])
STATUS = np.array([[0, 4, 0], [0, 0, 0]])
MODES = np.array([[1, 0, 3], [2, 2, 2]])
INDEX0 = np.array([2, 1])

# lane 0: e = (.5, .5, .25), (0, 1, 0), (1, 0, 1); final (2.5, .5) - (2, 0)
#         e_xy^2 = .5, 1, 1; e_th^2 = .0625, 0, 1; u^2 = .3125, 1, .25; s = 0 in, -0.1 out, 0.02 out
# lane 1: e = (0, 0, 0), (0, 2, 0), (0, 0, 0); final (4, 0) - (2, 0); s = 0.011 is on the bound: inside
EXPECT = np.array([[2.5, 1.0, 1.0625, 0.5, 1.5625, 1.0, 1.0, 0.0, 1.0, 2.0],
                   [4.0, 4.0, 0.0, 4.0, 0.0, 0.0, 0.0, 3.0, 0.0, 0.0]])


def test_names_cover_the_ten_columns():
    assert len(NAMES) == 10 == EXPECT.shape[1]


def test_hand_made_three_steps():
    m = closed_loop_metrics_ref(X, U, STATUS, MODES, TRAJ, INDEX0, S_LO, S_HI)
    np.testing.assert_array_equal(m, EXPECT)


def test_per_lane_tables_and_clamp():
    """The same run with one table per lane: lane 1's table shifted by one column reads the same rows from
    index0 = 2; columns past the end and before the start clamp to the last and the first."""
    per = np.stack([TRAJ, np.concatenate([TRAJ[:1], TRAJ[:2]])])     # lane 1: columns (c1, c1, c2)
    np.testing.assert_array_equal(ref_rows(per, [2, 2], 0, 2), np.stack([TRAJ[1], TRAJ[0]]))
    np.testing.assert_array_equal(ref_rows(TRAJ, [2, 1], 3, 2), np.stack([TRAJ[2], TRAJ[2]]))
    np.testing.assert_array_equal(ref_rows(TRAJ, [-4, 0], 0, 2), np.stack([TRAJ[0], TRAJ[0]]))
    m = closed_loop_metrics_ref(X[:1], U[:1], STATUS[:1], MODES[:1], np.stack([TRAJ]), 2, S_LO, S_HI)
    np.testing.assert_array_equal(m, EXPECT[:1])


def test_nan_step_counts_as_outside_and_does_not_enter_the_max():
    Xn = X.copy()
    Xn[0, 1, 0] = np.nan      # e_x of step 2
    Xn[0, 0, 3] = np.nan      # s of step 1
    m = closed_loop_metrics_ref(Xn, U, STATUS, MODES, TRAJ, INDEX0, S_LO, S_HI)
    assert np.isnan(m[0, 0]) and m[0, 1] == 1.0 and m[0, 9] == 3.0
    np.testing.assert_array_equal(m[1], EXPECT[1])
