"""
The trimming of the equal-birth (1-D) Wasserstein recurrence (csrc/wasserstein.hip, ws_solve), restated in numpy: the
recurrence over the live rows and columns alone must return the bits the full recurrence returns.

    F[i][j] = min(F[i-1][j], F[i][j-1], F[i-1][j-1] + g_ij),   zero boundaries,   g_ij = min(0, C_ij - s_i - t_j)

The gains are sklearn's expansion as the kernel evaluates it, except for its one fma (numpy has none: r_d * c_d + b0^2 is
rounded twice here, once there; the margin's derivation counts a rounding per product either way).  The rule is the
kernel's, operation for operation: with p = d - b0 of a row and q of a column, c = cos(pi/4), X the largest |coordinate|
and m = 1e-6 X + 1e-150, a column is dead if q (1+c) <= p_min (1-c) - m or q (1-c) >= p_max (1+c) + m, then a row
against the range of the live columns in the same way.

Bars: results equal as bits on every pair (no tolerance: the argument of DESIGN 3.3 is that the same operations run on
the same operands); every cell the rule leaves out has a computed gain of exactly 0; the cases built with dead points
lose at least those points; the row-by-row form used here equals a literal cell-by-cell loop on the small pairs.
"""
import numpy as np

CP = 0.7071067811865476        # np.cos(np.pi / 4)
SP = 0.7071067811865475        # np.sin(np.pi / 4)
REL, ABS, MAXC = 1e-6, 1e-150, 1e150


def _gains(b0, dr, dc, a_is_row):
    """(R, C) computed gains of rows (b0, dr) against columns (b0, dc)."""
    rs = dr * CP - b0 * SP
    ct = dc * CP - b0 * SP
    rn = b0 * b0 + dr * dr
    cn = b0 * b0 + dc * dc
    dot = dr[:, None] * dc[None, :] + b0 * b0
    d2 = -2.0 * dot
    d2 = (d2 + (rn[:, None] if a_is_row else cn[None, :])) + (cn[None, :] if a_is_row else rn[:, None])
    d2 = np.where(d2 > 0.0, d2, 0.0)
    g = (np.sqrt(d2) - rs[:, None]) - ct[None, :]
    return np.where(g < 0.0, g, 0.0)


def _recurrence(g):
    """F[R-1][C-1]; 0.0 for an empty range.  Row by row: min is exact, so the running minimum along a row has the
    bits of the cell-by-cell order."""
    R, C = g.shape
    if R == 0 or C == 0:
        return 0.0
    prev = np.zeros(C)
    for i in range(R):
        diag = np.concatenate([[0.0], prev[:-1]]) + g[i]
        prev = np.minimum.accumulate(np.minimum(prev, diag))     # (the zero boundary on the left: every entry is <= 0)
    return float(prev[-1])


def _recurrence_cells(g):
    """The kernel's cell: m = min(up, left); m = min(diag + g, m)."""
    R, C = g.shape
    F = np.zeros((R + 1, C + 1))
    for i in range(1, R + 1):
        for j in range(1, C + 1):
            up, left, dg = F[i - 1][j], F[i][j - 1], F[i - 1][j - 1] + g[i - 1][j - 1]
            m = up if up < left else left
            F[i][j] = dg if dg < m else m
    return float(F[R][C])


def _live(b0, dr, dc):
    """(ilo, ihi, jlo, jhi) by the kernel's rule; deaths sorted ascending."""
    R, C = len(dr), len(dc)
    mx = max(abs(b0), abs(dr[0]), abs(dr[-1]), abs(dc[0]), abs(dc[-1]))
    if not mx < MAXC:
        return 0, R, 0, C
    m = REL * mx + ABS
    c1p, c1m = 1.0 + CP, 1.0 - CP
    p, q = dr - b0, dc - b0
    lo_c, hi_c = p[0] * c1m - m, p[-1] * c1p + m
    jlo = int(np.count_nonzero(q * c1p <= lo_c))
    jhi = max(C - int(np.count_nonzero(q * c1m >= hi_c)), jlo)
    if jhi == jlo:
        return 0, 0, jlo, jhi
    lo_r, hi_r = q[jlo] * c1m - m, q[jhi - 1] * c1p + m
    ilo = int(np.count_nonzero(p * c1p <= lo_r))
    ihi = max(R - int(np.count_nonzero(p * c1m >= hi_r)), ilo)
    return ilo, ihi, jlo, jhi


def _check(b0, pr, qc, a_is_row=True, min_trim=0):
    dr, dc = np.sort(b0 + np.asarray(pr, float)), np.sort(b0 + np.asarray(qc, float))
    if len(dr) > len(dc):
        dr, dc = dc, dr                                      # rows = the smaller diagram
    assert 1 <= len(dr) <= 64 and 1 <= len(dc) <= 128
    g = _gains(b0, dr, dc, a_is_row)
    ilo, ihi, jlo, jhi = _live(b0, dr, dc)
    dead = np.ones(g.shape, bool)
    dead[ilo:ihi, jlo:jhi] = False
    assert (g[dead] == 0.0).all(), "a trimmed cell has a computed gain != 0"
    full, trimmed = _recurrence(g), _recurrence(g[ilo:ihi, jlo:jhi])
    assert np.float64(full).tobytes() == np.float64(trimmed).tobytes(), (full, trimmed, b0, len(dr), len(dc))
    n_trim = len(dr) - (ihi - ilo) + len(dc) - (jhi - jlo)
    assert n_trim >= min_trim, (n_trim, min_trim)
    if g.size <= 400:
        assert np.float64(_recurrence_cells(g)).tobytes() == np.float64(full).tobytes()
    return n_trim, g.size - int(dead.sum())


def test_trimmed_recurrence_is_bit_identical_random():
    rng = np.random.default_rng(11)
    n, trimmed, live = 0, 0, 0
    for k in range(260):
        R, C = int(rng.integers(1, 65)), int(rng.integers(1, 129))
        kind = k % 5
        if kind == 0:                                        # the workload: EEG deaths 0.48 .. 1.04, half the audio < 0.08
            p = rng.uniform(0.48, 1.04, R)
            q = np.where(rng.random(C) < 0.5, rng.uniform(1e-4, 0.08, C), rng.uniform(0.08, 0.9, C))
            b0 = 0.0
        elif kind == 1:                                      # log-uniform over six decades: prefix, suffix, dead rows
            p, q, b0 = 10.0 ** rng.uniform(-3, 3, R), 10.0 ** rng.uniform(-3, 3, C), 0.0
        elif kind == 2:                                      # tied deaths on a coarse grid
            p, q, b0 = rng.integers(1, 40, R) / 8.0, rng.integers(1, 400, C) / 64.0, 0.0
        elif kind == 3:                                      # a common birth != 0, also one far larger than the persistences
            b0 = float(rng.choice([0.3, -2.0, 37.5, 1000.0]))
            p, q = 10.0 ** rng.uniform(-4, 1, R), 10.0 ** rng.uniform(-4, 1, C)
        else:                                                # near each other: (almost) everything live
            p, q, b0 = rng.uniform(0.5, 1.0, R), rng.uniform(0.4, 1.2, C), 0.0
        t, l = _check(b0, p, q, a_is_row=bool(k & 1))
        n, trimmed, live = n + 1, trimmed + t, live + l
    assert n >= 200 and trimmed > 0 and live > 0


def test_all_dead_and_all_live_and_edges():
    rng = np.random.default_rng(12)
    for R, C in [(1, 1), (1, 128), (64, 128), (64, 64), (7, 90), (33, 34)]:
        p = rng.uniform(0.5, 1.0, R)
        # all live: ratios below 2.4 < 5.83, nothing may go
        t, _ = _check(0.0, p, rng.uniform(0.5, 1.2, C))
        assert t == 0
        # all dead, a factor 2 beyond the cut on either side: every row and every column goes
        _check(0.0, p, rng.uniform(1e-3, 0.5 / 5.83 / 2, C), min_trim=R + C)
        _check(0.0, p, rng.uniform(2 * 5.83, 40.0, C), min_trim=R + C)
        # dead prefix and suffix around live columns
        nd = C // 3
        q = np.concatenate([rng.uniform(1e-3, 0.04, nd), rng.uniform(0.5, 1.0, C - 2 * nd), rng.uniform(12.0, 20.0, nd)])
        _check(0.0, p, q, min_trim=2 * nd)
        _check(0.25, p, q, min_trim=2 * nd)
        # dead rows on both sides of live ones, against columns in one cluster
        if R >= 3:
            pp = np.concatenate([[1e-3], rng.uniform(0.5, 1.0, R - 2), [30.0]])
            _check(0.0, pp, rng.uniform(0.5, 1.0, C), min_trim=2)


def test_ratios_at_the_cut():
    """Columns within ulps of the cut, and on either side of the margin: whichever side they fall on, same bits."""
    cut = (1.0 - CP) / (1.0 + CP)                            # q / p below which a column is dead: 1 / (3 + 2 sqrt 2)
    rel = [0.0, 5e-7, 9.9e-7, 1e-6, 1.01e-6, 2e-6, 1e-5, 1e-3]
    for p0 in (1.0, 0.7310585786300049, 3.0):
        for side in (cut, 1.0 / cut):
            base = p0 * side
            qs = [np.nextafter(base, np.inf if k > 0 else -np.inf) if abs(k) == 1 else base for k in (-1, 0, 1)]
            qs += [base * (1.0 + s * r) for r in rel for s in (-1.0, 1.0)]
            for q in qs:
                _check(0.0, [p0], [q])
                _check(0.0, [p0, p0], [q, p0])
                _check(0.5, [p0] * 3, [q] * 2 + [p0] * 2)
    # huge coordinates switch the rule off instead of overflowing
    assert _live(0.0, np.array([1e200]), np.array([1.0, 1e200])) == (0, 1, 0, 2)
