"""Plain-NumPy reference of the spatial correlogram (utils/correlogram.py), the coordinate sets and value generators its tests
share, and the tolerances of tests/test_gpu_spatial_stats.py restated per band.

Reference: a brute-force pass over all ordered pairs in row chunks.  The distance is formed in separate NumPy operations -
``xx = dx * dx``, ``yy = dy * dy``, ``zz = dz * dz``, ``d2 = (xx + yy) + zz``, ``d = sqrt(d2)``, each rounded once - and the band
is ``np.searchsorted(radii, d, side="left")``: band 0 holds d <= r_1 (d = 0 among them), band b holds r_b < d <= r_{b+1}, and
``B`` means outside.  The diagonal is left out.

Tolerances (u = 2^-53, aZ = |Z|, s_b = (A_b aZ).sum(0), vmax = |V|.max(0)), worst-case bounds of float64 summation in any order on
both sides (the factor 4), as in tests/test_gpu_spatial_stats.py:
    C_b    4 (W_b + n) u (aZ' A_b aZ + outer(vmax, s_b) + outer(s_b, vmax))
    m2     4 n u (sum Z^2 + 2 vmax sum |Z|)
    mean   4 n u vmax
    m4     4 n u (sum Z^4 + 4 vmax sum |Z|^3)      (m2's bound with the derivative of Z^4 in place of that of Z^2)
    cross  to first order: (n / W_b) tol_C_b / sqrt(m2_a m2_b) + |cross_ab| (tol_m2_a / m2_a + tol_m2_b / m2_b)

``candidate_count`` restates the guard's number on the host: the grid of the device binning where the largest radius sets the
cell edge (edge r_B (1 + 2^-16), cell = floor((x - min) / edge) per axis, an axis without extent has one cell), then the sum
over cells of count(cell) x count(the 3^dim block around it).
"""
import numpy as np
from scipy import sparse

U = 2.0 ** -53


def band_reference(V, coords, radii, chunk=256):
    """deg (n, B) int64, W, sum_deg_sq (B,) int64, A (list of B scipy CSR), C (B, K, K), mean, m2, m4 (K,), n, and tol."""
    V = np.asarray(V, dtype=np.float64)
    c = np.asarray(coords, dtype=np.float64)
    r = np.asarray(radii, dtype=np.float64)
    n, K = V.shape
    B = r.size
    c3 = np.zeros((n, 3))
    c3[:, :c.shape[1]] = c
    rows = [[] for _ in range(B)]
    cols = [[] for _ in range(B)]
    for i0 in range(0, n, chunk):
        i1 = min(n, i0 + chunk)
        dx = c3[None, :, 0] - c3[i0:i1, None, 0]
        dy = c3[None, :, 1] - c3[i0:i1, None, 1]
        dz = c3[None, :, 2] - c3[i0:i1, None, 2]
        xx = dx * dx
        yy = dy * dy
        zz = dz * dz
        d2 = xx + yy
        d2 = d2 + zz
        d = np.sqrt(d2)
        band = np.searchsorted(r, d.ravel(), side="left").reshape(d.shape)
        band[np.arange(i1 - i0), np.arange(i0, i1)] = B                     # i != j
        for b in range(B):
            ii, jj = np.nonzero(band == b)
            rows[b].append(ii + i0)
            cols[b].append(jj)
    A = []
    for b in range(B):
        ii, jj = np.concatenate(rows[b]), np.concatenate(cols[b])
        A.append(sparse.csr_matrix((np.ones(ii.size), (ii, jj)), shape=(n, n)))
    deg = np.stack([np.asarray(a.sum(1)).ravel().astype(np.int64) for a in A], axis=1)
    mean = V.sum(0) / n
    Z = V - mean
    m2 = (Z * Z).sum(0)
    m4 = (Z * Z * Z * Z).sum(0)
    C = np.stack([Z.T @ (a @ Z) for a in A])
    W = deg.sum(0)
    aZ, vmax = np.abs(Z), np.abs(V).max(0)
    tol_C = []
    for b in range(B):
        AaZ = A[b] @ aZ
        s = AaZ.sum(0)
        tol_C.append(4 * (W[b] + n) * U * (aZ.T @ AaZ + np.outer(vmax, s) + np.outer(s, vmax)))
    tol = {"C": np.stack(tol_C), "m2": 4 * n * U * ((Z * Z).sum(0) + 2 * vmax * aZ.sum(0)), "mean": 4 * n * U * vmax,
           "m4": 4 * n * U * ((Z ** 4).sum(0) + 4 * vmax * (aZ ** 3).sum(0))}
    return {"deg": deg, "W": W, "sum_deg_sq": (deg * deg).sum(0), "A": A, "C": C, "mean": mean, "m2": m2, "m4": m4, "n": n,
            "Z": Z, "tol": tol}


def cross_tol(ref, b, cross_b):
    """First-order bound of |cross_b - reference| from the bounds of C_b and m2; inf where it is not finite."""
    n, W, m2 = ref["n"], ref["W"][b], ref["m2"]
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = ref["tol"]["m2"] / m2
        t = (np.float64(n) / np.float64(W)) * ref["tol"]["C"][b] / np.sqrt(np.outer(m2, m2)) + np.abs(cross_b) * (rel[:, None] + rel[None, :])
    return np.where(np.isfinite(t), t, np.inf)


def candidate_count(coords, r_max):
    """(candidates, cells per axis) for coordinate sets whose density edge sqrt_dim(volume / n) is below the radius' edge (asserted)."""
    c = np.asarray(coords, dtype=np.float64)
    n, dim = c.shape
    mn, mx = c.min(0), c.max(0)
    ext = mx - mn
    eff = int((ext > 0).sum())
    h = r_max * (1.0 + 1.0 / 65536.0)
    assert eff == 0 or (np.prod(ext[ext > 0]) / n) ** (1.0 / eff) < 0.99 * h
    nc = np.ones(3, dtype=np.int64)
    nc[:dim] = np.where(ext > 0, np.floor(ext / h) + 1.0, 1.0).astype(np.int64)
    assert nc.prod() <= max(4 * n, 4096)
    inv_h = 1.0 / h
    cell = np.zeros((n, 3), dtype=np.int64)
    cell[:, :dim] = np.clip(np.floor((c - mn) * inv_h).astype(np.int64), 0, nc[:dim] - 1)
    counts = np.zeros(tuple(nc + 2), dtype=np.int64)
    np.add.at(counts, (cell[:, 0] + 1, cell[:, 1] + 1, cell[:, 2] + 1), 1)
    inner = counts[1:-1, 1:-1, 1:-1]
    around = np.zeros_like(inner)
    for dx in (0, 1, 2):
        for dy in (0, 1, 2):
            for dz in (0, 1, 2):
                around += counts[dx:dx + nc[0], dy:dy + nc[1], dz:dz + nc[2]]
    return int((inner * around).sum()), tuple(int(v) for v in nc)


# ---------------------------------------------------------------- values
def exact_values(n, K, seed):
    """Integers in [-8, 8) over 16, about 60 % zeros, for n // 2 rows, stacked with their negation and shuffled; one zero row
    more when n is odd.  Every column sums to exactly zero, so mean = 0 and Z = V on any machine."""
    rs = np.random.RandomState(seed)
    h = n // 2
    half = rs.randint(-8, 8, size=(h, K)).astype(np.float64) / 16.0
    half[rs.rand(h, K) < 0.6] = 0.0
    V = np.concatenate([half, -half] + ([np.zeros((1, K))] if n % 2 else []), axis=0)
    return V[rs.permutation(n)]


def dirichlet_values(n, K, seed):
    return np.random.RandomState(seed).dirichlet(np.full(K, 0.3), n)


# ---------------------------------------------------------------- coordinate sets: name -> (coords, radii)
def square_lattice(m):
    y, x = np.divmod(np.arange(m * m), m)
    return np.stack([x, y], axis=1).astype(np.float64)


def cube_lattice(m):
    i = np.arange(m * m * m)
    return np.stack([i % m, (i // m) % m, i // (m * m)], axis=1).astype(np.float64)


def chain(n):
    return np.arange(n, dtype=np.float64)[:, None]


def integer_cloud(n, seed=5):
    return np.random.RandomState(seed + n).randint(0, 6, size=(n, 2)).astype(np.float64)


def ragged(dim, seed=11):
    """n = 2000: half uniform in the unit square, half in a 0.05-wide cluster (cells with more than 64 points), the last spot at
    (10, 10) with no neighbour; dim = 3 adds a z column in [0, 0.02)."""
    rs = np.random.RandomState(seed)
    n = 2000
    xy = np.concatenate([rs.rand(n // 2, 2), 0.4 + 0.05 * rs.rand(n - n // 2 - 1, 2), np.array([[10.0, 10.0]])], axis=0)
    if dim == 3:
        z = 0.02 * rs.rand(n, 1)
        z[-1] = 10.0
        xy = np.concatenate([xy, z], axis=1)
    return xy


def strip(x_extent, seed=17):
    """150 spots in a strip along y, half a unit apart, x uniform in [0, x_extent): the x axis has one cell, the y axis many."""
    rs = np.random.RandomState(seed)
    return np.stack([x_extent * rs.rand(150), 0.5 * np.arange(150)], axis=1)


def slab(seed=19):
    """400 spots in a 0.5 x 10 x 6 slab: the thin axis comes first, so it shares its stride in the cell id with another axis."""
    rs = np.random.RandomState(seed)
    return rs.rand(400, 3) * np.array([0.5, 10.0, 6.0])


def fit_coords():
    """The coordinates of the model-surface tests (datagen.count_like(200, 300, 5, 0.1, seed=9))."""
    import datagen
    return datagen.count_like(200, 300, 5, 0.1, seed=9)[2]


def anndata_coords():
    """The coordinates of the AnnData-surface tests (datagen.anndata_case())."""
    import datagen
    return datagen.anndata_case()["coords"]


def host_grid_radius(coords):
    """1.5 x the median nearest-neighbour distance (utils.graph.grid_radius), by scipy."""
    from scipy.spatial import cKDTree
    return 1.5 * float(np.median(cKDTree(coords).query(coords, k=2)[0][:, 1]))


def uniform_cloud(n=3000, seed=3):
    return np.random.RandomState(seed).rand(n, 2)


SIZE_EDGES = (1, 2, 3, 63, 64, 65, 257)
SIZE_EDGE_RADII = np.array([1.0, 2.5, 4.0, 100.0])
B_EDGES = (1, 2, 10, 32)


def coord_sets():
    sets = {"square32": (square_lattice(32), np.array([1.0, 1.5, 2.0, 5.0])),
            "cube8": (cube_lattice(8), np.array([1.0, 1.5, 1.8, 3.0])),
            "chain257": (chain(257), np.array([1.0, 2.0, 7.0])),
            "ragged2": (ragged(2), 0.01 * np.arange(1, 7)),
            "ragged3": (ragged(3), 0.01 * np.arange(1, 7)),
            "uniform3000": (uniform_cloud(), 0.02 * np.arange(1, 9)),
            "checker32": (square_lattice(32), np.array([1.0, 1.5, 2.0])),
            "square23": (square_lattice(23), 1.5 * np.arange(1, 4)),
            "strip0": (strip(0.0), np.array([1.0, 2.5])),
            "strip_thin": (strip(0.3), np.array([1.0, 2.0])),
            "slab": (slab(), np.array([0.8, 1.5])),
            "fit200": (fit_coords(), host_grid_radius(fit_coords()) * np.array([1.0, 2.0, 3.5])),
            "anndata120": (anndata_coords(), host_grid_radius(anndata_coords()) * np.arange(1, 4))}
    for B in B_EDGES:
        sets[f"square32_B{B}"] = (square_lattice(32), 0.75 * np.arange(1, B + 1))
    for n in SIZE_EDGES:
        sets[f"cloud{n}"] = (integer_cloud(n), SIZE_EDGE_RADII)
    return sets


# the sets on which the guard's candidate count is restated exactly (candidate_count's precondition holds)
CANDIDATE_SETS = ("square32", "square32_B2", "cube8", "chain257", "strip0", "strip_thin", "slab", "cloud257")

# the cases whose sums must be exact: (coordinate set, K, seed of exact_values)
K_EDGES = (1, 3, 8, 9, 30, 33, 65)


def exact_cases():
    cases = [(name, K, 100 * (i + 1) + K) for i, name in enumerate(("square32", "cube8", "chain257")) for K in K_EDGES]
    cases += [(f"square32_B{B}", 5, 600 + B) for B in B_EDGES]
    cases += [(f"cloud{n}", 4, 400 + n) for n in SIZE_EDGES]
    cases += [("ragged2", 9, 501), ("ragged3", 9, 502)]
    cases += [("strip0", 4, 701), ("strip_thin", 4, 702), ("slab", 4, 703)]
    return cases
