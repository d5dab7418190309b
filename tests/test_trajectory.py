"""thesis_amd/trajectory.py: what is made of trajectories on the host.  No GPU."""
import numpy as np
import pytest

from thesis_amd import trajectory


def spiral(n=50):
    t = np.linspace(0, 4, n)
    return np.stack([t * np.cos(t), t * np.sin(t), t], axis=1)


def test_ate_is_zero_for_a_rigidly_moved_copy():
    a = spiral()
    c, s = np.cos(0.7), np.sin(0.7)
    b = a.copy()
    b[:, :2] = a[:, :2] @ np.array([[c, -s], [s, c]]).T + [3.0, -1.5]
    assert trajectory.ate(a, b) < 1e-12
    assert trajectory.ate(b, a) < 1e-12
    R, t = trajectory.rigid_fit(a, b)
    assert np.allclose(R, [[c, -s], [s, c]], atol=1e-12) and np.allclose(t, [3.0, -1.5], atol=1e-12)


def test_ate_without_alignment_is_the_offset():
    a = spiral()
    b = a.copy()
    b[:, 0] += 3.0
    b[:, 1] -= 4.0
    assert abs(trajectory.ate(a, b, align=False) - 5.0) < 1e-12
    assert trajectory.ate(a, b) < 1e-12
    with pytest.raises(ValueError):
        trajectory.ate(a, b[:-1])


def test_coalescence():
    assert trajectory.coalescence([1, 1, 1, 2, 5, 9]) == 2
    assert trajectory.coalescence([3, 4]) == -1
    assert trajectory.coalescence([1]) == 0

    class S:
        n_alive = np.array([1, 1, 4], dtype=np.int32)
    assert trajectory.coalescence(S()) == 1


def test_path_length():
    assert trajectory.path_length([[0, 0, 0], [3, 4, 1], [3, 5, 2]]) == 6.0
    assert trajectory.path_length([[1, 1, 0]]) == 0.0
