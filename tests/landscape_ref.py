"""
The persistence landscape, the Betti curve and their group mean in numpy: the definition of include/tdaeeg.h, written
with the operations it names and nothing else.  Every value is one correctly rounded float64 operation or a selection, so
the kernel (csrc/landscape.hip) has to give these bits.
"""
import numpy as np


def diagram_vector(rows, grid, levels):
    """V = [lambda_1 .. lambda_K, beta], (K + 1, n_grid), of one diagram: rows (k, 2) float64 (already cut to
    min(cnt, cap) rows), grid (n_grid,) float64."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 2)
    grid = np.asarray(grid, dtype=np.float64)
    b, d = rows[:, 0:1], rows[:, 1:2]
    fin = (np.isfinite(b) & np.isfinite(d))[:, 0]
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.minimum(grid[None, :] - b[fin], d[fin] - grid[None, :])      # (|F|, n_grid): one subtraction each
        t = np.where(t > 0, t, 0.0)
        t = np.concatenate([t, np.zeros((levels, grid.shape[0]))], axis=0)  # padded with K zero rows
        lam = -np.sort(-t, axis=0)[:levels]
        beta = ((b <= grid[None, :]) & (grid[None, :] < d)).sum(axis=0).astype(np.float64)
    return np.concatenate([lam, beta[None, :]], axis=0)


def cut(rows, cnt, cap=None):
    """The rows of a diagram buffer the definition sees: i < min(cnt, cap)."""
    rows = np.asarray(rows, dtype=np.float64)
    cap = rows.shape[0] if cap is None else cap
    return rows[:max(0, min(int(cnt), cap))]


def group_mean(vectors):
    """np.mean over the kept diagrams of a group, in order; NaN without one."""
    if not len(vectors):
        return None
    return np.mean(np.stack(vectors), axis=0)


def sequential_mean(vectors):
    """The group mean as the definition words it: s = V(first), s = s + V(next) ..., s / n."""
    s = vectors[0].copy()
    for v in vectors[1:]:
        s = s + v
    return s / float(len(vectors))


def landscape_mean(rows, cnt, grid, levels, seg_off=None, status=None, skip_mask=0):
    """rows (n, cap, 2), cnt (n,) -> (n_seg, levels + 1, n_grid): what tda_landscape_mean_dev computes."""
    rows = np.asarray(rows, dtype=np.float64)
    n, cap = rows.shape[0], rows.shape[1]
    seg_off = np.arange(n + 1) if seg_off is None else np.asarray(seg_off)
    grid = np.asarray(grid, dtype=np.float64)
    out = np.full((len(seg_off) - 1, levels + 1, grid.shape[0]), np.nan)
    for g in range(len(seg_off) - 1):
        kept = [diagram_vector(cut(rows[w], cnt[w], cap), grid, levels) for w in range(seg_off[g], seg_off[g + 1])
                if status is None or not (int(status[w]) & skip_mask)]
        if kept:
            out[g] = group_mean(kept)
    return out


def lists_mean(dgms, grid, levels, seg_off, status=None, skip_mask=0):
    """The same from a list of (k, 2) diagrams (DeviceDiagrams.to_lists())."""
    out = np.full((len(seg_off) - 1, levels + 1, len(grid)), np.nan)
    for g in range(len(seg_off) - 1):
        kept = [diagram_vector(dgms[w], grid, levels) for w in range(seg_off[g], seg_off[g + 1])
                if status is None or not (int(status[w]) & skip_mask)]
        if kept:
            out[g] = group_mean(kept)
    return out


# ---- restatements used by the model test ---------------------------------------------------------------------------
def diagram_vector_brute(rows, grid, levels):
    """For each grid point a Python list of tents, sorted, padded: no numpy selection."""
    rows = [(float(b), float(d)) for b, d in np.asarray(rows, dtype=np.float64).reshape(-1, 2)]
    out = np.zeros((levels + 1, len(grid)))
    for j, t in enumerate(np.asarray(grid, dtype=np.float64)):
        tents = []
        for b, d in rows:
            if np.isfinite(b) and np.isfinite(d):
                v = min(t - b, d - t)
                tents.append(v if v > 0 else 0.0)
        tents = sorted(tents, reverse=True) + [0.0] * levels
        out[:levels, j] = tents[:levels]
        out[levels, j] = float(sum(1 for b, d in rows if b <= t < d))
    return out


def diagram_vector_insertion(rows, grid, levels):
    """The kernel's route: per grid point K sorted registers, every tent inserted by K (max, min) pairs; the Betti count
    an integer counter."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 2)
    grid = np.asarray(grid, dtype=np.float64)
    top = np.zeros((levels, grid.shape[0]))
    beta = np.zeros(grid.shape[0], np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for b, d in rows:
            beta += (b <= grid) & (grid < d)
            if not (np.isfinite(b) and np.isfinite(d)):
                continue
            v = np.fmin(grid - b, d - grid)
            v = np.where(v > 0, v, 0.0)
            for k in range(levels):
                hi = np.fmax(top[k], v)
                v = np.fmin(top[k], v)
                top[k] = hi
    return np.concatenate([top, beta[None, :].astype(np.float64)], axis=0)


def random_diagram(rng, k, kind="f64", h0=False, n_inf=0):
    """k rows with d >= b in [0, 2]; kind "f32": float32-exact values widened, as Rips emits them."""
    b = rng.uniform(0.0, 1.5, k)
    d = b + rng.uniform(0.0, 0.6, k)
    if h0:
        b[:] = 0.0
    rows = np.stack([b, d], axis=1)
    if kind == "f32":
        rows = rows.astype(np.float32).astype(np.float64)
    if n_inf:
        rows[rng.choice(k, size=min(n_inf, k), replace=False), 1] = np.inf
    return rows
