"""Point sets for the scoring tests (tests/test_score_host.py, tests/test_gpu_score.py) and an independent form of the
Procrustes error to hold the rule against: the Umeyama alignment through np.linalg.svd (LAPACK), float64."""
import numpy as np

KINDS = ('exact', 'noisy', 'planar', 'collinear', 'mirrored', 'identical')


def rotation(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def make_row(rng, n, kind, noise=0.005):
    """One row of n points of a hand's size (errors stay far below 0.5 m) -> (P, G) float32 [n,3]."""
    P = rng.normal(0, 0.05, (n, 3))
    if kind == 'planar':
        P[:, 2] = 0.0
    if kind == 'collinear':
        P = np.outer(rng.normal(0, 0.05, n), rng.normal(size=3))
    G = rng.uniform(0.7, 1.4) * P @ rotation(rng).T + rng.normal(0, 0.1, 3)
    if kind in ('noisy', 'planar', 'mirrored'):
        G = G + rng.normal(0, noise, (n, 3))
    if kind == 'mirrored':
        G[:, 0] = -G[:, 0]
    if kind == 'identical':
        G = P.copy()
    return P.astype(np.float32), G.astype(np.float32)


def make_rows(seed, N, n, kinds=KINDS, noise=0.005):
    """N rows, the kinds in turn -> (pred, gt) float32 [N,n,3] and the kind of every row."""
    rng = np.random.default_rng(seed)
    rows = [make_row(rng, n, kinds[r % len(kinds)], noise) for r in range(N)]
    return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]), [kinds[r % len(kinds)] for r in range(N)]


def umeyama_errors(P, G, on=None):
    """The per-point error after the best similarity transform of P onto G over the points `on`, by the SVD (Umeyama 1991, with
    the determinant correction: a proper rotation).  float64 [n]; nan where a point is not counted."""
    P, G = np.asarray(P, np.float64), np.asarray(G, np.float64)
    on = np.ones(P.shape[0], bool) if on is None else np.asarray(on, bool)
    p, g = P[on], G[on]
    mp, mg = p.mean(0), g.mean(0)
    pc, gc = p - mp, g - mg
    U, D, Vt = np.linalg.svd(gc.T @ pc)
    d = np.ones(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        d[2] = -1.0
    R = U @ np.diag(d) @ Vt
    scale = (D * d).sum() / (pc * pc).sum()
    out = np.full(P.shape[0], np.nan)
    out[on] = np.linalg.norm(scale * pc @ R.T + mg - g, axis=1)
    return out
