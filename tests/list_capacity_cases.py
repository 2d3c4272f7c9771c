"""
Inputs of tests/test_gpu_list_capacity.py: windows and clouds whose chunks list more non-trivial triangles than the
triangle list of phase d holds (csrc/rips.hip, LCAP: 416 entries with a 32-bit class word, 277 with a 64-bit one, 166 /
92 / 48 with two / four / eight 64-bit words; it was 255 for one word), so that a prefix of the list is reduced and the
chunk is listed again.

ball_circle: a circle of radius 1 and a small ball at its centre.  The circle's class is alive when the edges between
ball and circle enter, all of them within 2 rho of length 1, i.e. in a few chunks; the first triangle ball point -
circle point - circle point kills the class, and every other such triangle of the chunk is non-zero under the table of
the chunk start and is listed.  The list grows with (ball points) x (circle points).

The sizes below were chosen with the diagnostic build (make PROFILE=1, tools/phase_profile.py counters 11-13 and 46) on
an MI355X, one cloud per run; the counts it gave are in CASES.
"""
import numpy as np


def ball_circle(n, n_circle, seed, rho=0.02):
    rng = np.random.default_rng(seed)
    ang = 2 * np.pi * (np.arange(n_circle) + 0.2 * rng.random(n_circle)) / n_circle
    circle = np.stack([np.cos(ang), np.sin(ang), np.zeros(n_circle)], 1)
    v = rng.standard_normal((n - n_circle, 3))
    v /= np.linalg.norm(v, axis=1)[:, None]
    ball = rho * v * (rng.random(n - n_circle) ** (1.0 / 3.0))[:, None]
    return np.concatenate([circle, ball])


# name: (points, circle points).  Measured with the diagnostic build, narrow first pass (capacity 416; 255 before):
#   name      listing rounds  entries listed  rounds over 416  rounds over 832   (with a capacity of 255: rounds over it)
#   twice60         2             2380              2                2                      8 of 10
#   once60          2             1332              1                1                     13 of 15
#   twice124        3             1244              1                1                      8 of 11
#   over124         3             1030              2                0                      6 of 8
#   between124      3              613              0                0                      2 of 5
# between124: no round over 416, two over 255 -- its longest list lies between the two capacities.
CASES = {
    "twice60": (60, 30),
    "once60": (60, 20),
    "twice124": (124, 84),
    "over124": (124, 62),
    "between124": (124, 40),
}


def clouds(name, copies=4):
    """the measured cloud (seed 1) and copies - 1 more of the same make (other seeds: their lists differ a little)"""
    n, c = CASES[name]
    return np.stack([ball_circle(n, c, 1 + k) for k in range(copies)])
