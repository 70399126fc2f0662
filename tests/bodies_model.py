"""Float64 restatement of the kinematic boundary bodies (DESIGN.md "Kinematic boundary bodies"), for the tests: the pose integration
of the host, the table the kernels get, the transform, the wall velocity u_b, and DFSPH's A launch with the term (u_i - u_b) . g_ib
(on top of tests/dfsph_model.py).

Pose integration per step, in double: x += dt v; q = exp(dt omega / 2) q, the exact exponential map (identity when |omega| = 0),
renormalised.  The table is rounded to SReal before the kernels see it, so the transform of the model takes the rounded table:
p = x_k + R_k (r - c_k), evaluated here in float64.  The device evaluates it in SReal as d = r - c, p_i = x_i + ((R_i0 d_0 + R_i1 d_1)
+ R_i2 d_2): four roundings of relative size eps / 2 on the sum and one on the result, well inside the bound the GPU test uses,
6 eps (|x_i| + sum_j |R_ij| |d_j|) per coordinate.
"""
import numpy as np

from tests import dfsph_model


def quat_mul(a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw])


def exp_half(omega, dt):
    """exp(dt omega / 2) as a unit quaternion (w, x, y, z)"""
    omega = np.asarray(omega, np.float64)
    wn = float(np.sqrt(omega @ omega))
    if wn == 0.0:
        return np.array([1.0, 0.0, 0.0, 0.0])
    half = 0.5 * dt * wn
    return np.concatenate([[np.cos(half)], np.sin(half) / wn * omega])


def advance(x, q, v, omega, dt):
    """one step of the pose integration; omega = 0 returns q itself, untouched"""
    x = np.asarray(x, np.float64) + dt * np.asarray(v, np.float64)
    omega = np.asarray(omega, np.float64)
    if not omega.any():
        return x, q
    r = quat_mul(exp_half(omega, dt), np.asarray(q, np.float64))
    return x, r / np.sqrt(r @ r)


def rotation(q):
    w, x, y, z = q
    return np.array([[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)],
                     [2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x)],
                     [2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)]])


def origin(rest):
    """c_k: the mean of the rest positions, summed one after the other in double as the host does"""
    rest = np.asarray(rest, np.float64)[:, :3]
    return np.cumsum(rest, axis=0)[-1] / len(rest)


class Body:
    def __init__(self, rest, v=(0, 0, 0), omega=(0, 0, 0)):
        self.rest = np.asarray(rest)[:, :3]
        self.c = origin(self.rest)
        self.x = self.c.copy()
        self.q = np.array([1.0, 0.0, 0.0, 0.0])
        self.v = np.asarray(v, np.float64)
        self.omega = np.asarray(omega, np.float64)

    def step(self, dt):
        if self.v.any() or self.omega.any():
            self.x, self.q = advance(self.x, self.q, self.v, self.omega, dt)

    def table(self, real):
        """(R, x, c, v, omega) rounded to SReal, as float64 arrays"""
        r = lambda a: np.asarray(a, np.float64).astype(real).astype(np.float64)
        return r(rotation(self.q)), r(self.x), r(self.c), r(self.v), r(self.omega)

    def world(self, real):
        """world positions of the body's particles and the rounding bound of the device's evaluation, per coordinate"""
        R, x, c, _, _ = self.table(real)
        d = np.asarray(self.rest, np.float64) - c
        p = x + d @ R.T
        bound = 6.0 * np.finfo(real).eps * (np.abs(x) + np.abs(d) @ np.abs(R).T)
        return p, bound


def wall_velocity(p, x, v, omega):
    """u_b = v + omega x (p - x)"""
    return np.asarray(v, np.float64) + np.cross(np.asarray(omega, np.float64), np.asarray(p, np.float64) - np.asarray(x, np.float64))


# ---- DFSPH with moving walls: div_i = sum_j (u_i - u_j) . g_ij + sum_b (u_i - u_b) . g_ib ----------------------------------------
_plain_divergence = dfsph_model.divergence


def divergence_moving(pairs, u, ub):
    div = _plain_divergence(pairs, u)
    if len(pairs.bi):
        div = div - np.bincount(pairs.bi, np.sum(np.asarray(ub, np.float64)[pairs.bj] * pairs.gb, axis=1), pairs.n)
    return div


def solve_moving(params, pairs, ub, alpha, u, K_prev=None, **kw):
    """dfsph_model.solve with the A launch of a moving context (ub: the wall velocity per sorted boundary particle)"""
    plain = dfsph_model.divergence
    dfsph_model.divergence = lambda prs, vel: divergence_moving(prs, vel, ub)
    try:
        return dfsph_model.solve(params, pairs, alpha, u, K_prev, **kw)
    finally:
        dfsph_model.divergence = plain
