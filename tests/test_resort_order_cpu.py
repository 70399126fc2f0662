"""tests/common.next_sorted_keys, the numpy model of the order a step sorts its particles into (tests/test_resort_features_gpu.py holds
the device to it), against a brute-force Python sort on a hand-built grid: 4 x 2 x 8 cells of 0.5 from (-1, 0.25, -2), particles that
share a cell (ties keep their array order), that lie on cell faces, and that lie outside the grid on either side (their cell
coordinates wrap by the power-of-two mask, negative ones included).  No GPU.
"""
import numpy as np
import pytest

from tests.common import next_sorted_keys, small_dam_break

ORIGIN, CELL, GRID = (-1.0, 0.25, -2.0), (0.5, 0.5, 0.5), (4, 2, 8)


def grid_params(double):
    p = small_dam_break(double=double)[0].copy()
    for a in range(3):
        p["worldOrigin"][0][a] = ORIGIN[a]
        p["cellSize"][0][a] = CELL[a]
        p["gridSize"][0][a] = GRID[a]
    return p


def hand_points(real):
    rows = [
        (-0.9, 0.3, -1.9),     # cell (0, 0, 0)
        (0.9, 1.2, 1.9),       # cell (3, 1, 7): the last cell
        (-0.6, 0.4, -1.6),     # cell (0, 0, 0) again: a tie behind row 0
        (-0.5, 0.75, -1.5),    # on three faces: belongs to the upper cell, (1, 1, 1)
        (1.1, 0.3, -1.9),      # x = 4: wraps to 0 -> cell (0, 0, 0), the third of the tie
        (-1.2, 0.3, -1.9),     # x = -1: wraps to 3
        (-0.9, -0.1, -1.9),    # y = -1: wraps to 1
        (-0.9, 1.3, -1.9),     # y = 2: wraps to 0 -> cell (0, 0, 0), the fourth
        (-0.9, 0.3, -2.3),     # z = -1: wraps to 7
        (-0.9, 0.3, 2.1),      # z = 8: wraps to 0 -> cell (0, 0, 0), the fifth
        (-3.3, -7.1, 9.9),     # far outside on every axis: (-5, -15, 23) wraps to the last cell
        (0.9, 1.2, 1.9),       # the last cell again: a tie at the end
        (0.0, 0.75, 0.0),      # faces again, mid-grid
        (-0.9, 0.3, -1.9),     # a copy of row 0
    ]
    pos = np.ones((len(rows), 4), real)
    pos[:, :3] = np.array(rows, np.float64).astype(real)
    return pos


def brute_force(pos, real):
    keys = []
    for row in pos:
        c = []
        for a in range(3):
            q = (real(row[a]) - real(ORIGIN[a])) / real(CELL[a])   # the quotient in SReal, as calcGridPos forms it
            # the device's (int): NaN -> 0, saturating at the ends of int32
            g = 0 if np.isnan(q) else 2 ** 31 - 1 if q >= 2.0 ** 31 else -2 ** 31 if q < -2.0 ** 31 else int(np.floor(q))
            c.append(g % GRID[a])                                  # Python's % wraps negatives as the two's-complement mask does
        keys.append((c[2] * GRID[1] + c[1]) * GRID[0] + c[0])
    order = sorted(range(len(pos)), key=lambda i: (keys[i], i))
    return [keys[i] for i in order], order


@pytest.mark.parametrize("double", [False, True], ids=["f32", "f64"])
def test_hand_grid_against_a_brute_force_sort(double):
    real = np.float64 if double else np.float32
    p, pos = grid_params(double), hand_points(real)
    keys, index = next_sorted_keys(p, pos, real)
    want_keys, want_index = brute_force(pos, real)
    assert keys.dtype == np.uint32 and index.dtype == np.uint32
    assert keys.tolist() == want_keys and index.tolist() == want_index
    # what the hand cases are there for: the five-fold tie in cell 0 in array order, the wraps, the faces
    assert index[:6].tolist() == [0, 2, 4, 7, 9, 13] and keys[:6].tolist() == [0] * 6
    assert keys[index.tolist().index(5)] == 3 and keys[index.tolist().index(6)] == 4 and keys[index.tolist().index(8)] == 7 * 8
    assert keys[index.tolist().index(3)] == (1 * 2 + 1) * 4 + 1
    assert index[-3:].tolist() == [1, 10, 11] and keys[-3:].tolist() == [63] * 3   # (row 10 wraps to (3, 1, 7) from (-5, -15, 23))


@pytest.mark.parametrize("double", [False, True], ids=["f32", "f64"])
def test_non_finite_and_huge_coordinates_convert_as_the_device_does(double):
    """NaN -> cell coordinate 0; +inf and anything beyond int32 -> INT_MAX, whose low bits are all ones: the last cell of the axis;
    -inf -> INT_MIN, whose low bits are zero: the first"""
    real = np.float64 if double else np.float32
    pos = hand_points(real)
    pos[2, 0] = np.nan
    pos[3, :3] = np.nan
    pos[5, 1] = np.inf
    pos[6, 2] = -np.inf
    pos[8, 0] = 3e12
    pos[9, 2] = -3e12
    keys, index = next_sorted_keys(grid_params(double), pos, real)
    want_keys, want_index = brute_force(pos, real)
    assert keys.tolist() == want_keys and index.tolist() == want_index
    by_row = dict(zip(index.tolist(), keys.tolist()))
    assert by_row[3] == 0 and by_row[2] == 0          # (row 2: x becomes 0, y and z were 0)
    assert by_row[5] == (0 * 2 + 1) * 4 + 3           # x = -1 wraps to 3, y saturates to the last of 2, z = 0
    assert by_row[6] == (0 * 2 + 1) * 4 + 0 and by_row[8] == 7 * 8 + 3 and by_row[9] == 0


def test_random_points_against_a_brute_force_sort():
    rng = np.random.default_rng(11)
    pos = np.ones((500, 4), np.float32)
    pos[:, :3] = rng.uniform(-6.0, 6.0, (500, 3)).astype(np.float32)   # three grids wide: most points wrap
    pos[100:200] = pos[:100]                                            # ties
    keys, index = next_sorted_keys(grid_params(False), pos, np.float32)
    want_keys, want_index = brute_force(pos, np.float32)
    assert keys.tolist() == want_keys and index.tolist() == want_index
    assert len(set(want_keys)) == 64   # every cell is hit
