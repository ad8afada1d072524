"""CPU: the numpy restatement of the closest point on an indexed mesh (tests/closest_ref.py) held to things that do not come from any code
under test: an independent float64 point-triangle distance, planted points with known regions, closest points and barycentrics, an analytic
sphere, and the barycentric interpolation of `mesh.interpolate`."""
import numpy as np
import torch

from di_fusion_amd.system import mesh as M
from tests import closest_ref as R
from tests import closest_slack as K
from tests import simplify_ref as S

F32, F64 = np.float32, np.float64
U = 2.0 ** -24


def comps(x):
    return tuple(np.ascontiguousarray(x[:, k], dtype=F32) for k in range(3))


# ---- against float64 -------------------------------------------------------------------------------------------------------------------
L_MIN, L_MAX, MIN_ANGLE_DEG, OFFSET, M_MAX = 0.5, 1.0, 30.0, 0.8, 2.0
P_MAX = OFFSET + L_MAX                       # query to any vertex: the offset from the centroid plus at most two thirds of a median (< L_MAX)


def d2_bound():
    """The bound on |d2 (float32 sequence) - d2 (exact)| for the stated shapes, from the sequence itself (u = 2^-24, L = an edge, P = query to
    vertex).  A dot of two differences is off by 6 u L P (two input roundings, three products, two sums); a product of two dots by 13 u (L P)^2;
    va, vb, vc (a difference of two products) by 27 u (L P)^2.  den = |ab x ac|^2 >= L_MIN^4 sin^2(min angle); v = vb / den carries the
    numerator's error over den plus den's relative error (three such terms) times v <= 1, plus the division and the clamp: dv.  The edge
    parameters have smaller errors.  The computed point is off, inside the triangle's plane (or along the edge's line), by dx <= 2 dv L_MAX; a
    region chosen wrongly happens only within that error of the region's border, where two formulas differ by as much: 2 dx.  The true
    closest point is the foot of a perpendicular, so d2 grows by at most (2 dx)^2 (Pythagoras), and the last subtraction and the squares
    (the point left the exact one by 10 u M_MAX per axis more; three roundings of d2) add 2 P sqrt(3) 10 u M_MAX + 4 u P^2."""
    lp2 = (L_MAX * P_MAX) ** 2
    den_min = L_MIN ** 4 * np.sin(np.radians(MIN_ANGLE_DEG)) ** 2
    dv = 4 * 27 * U * lp2 / den_min + 2 * U
    dx = 2 * dv * L_MAX
    return (2 * dx) ** 2 + 2 * P_MAX * np.sqrt(3.0) * 10 * U * M_MAX + 4 * U * P_MAX ** 2


def well_shaped(n, seed):
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1, 1, size=(40 * n, 3))
    b = a + rng.normal(size=a.shape) * 0.45
    c = a + rng.normal(size=a.shape) * 0.45
    e = [np.linalg.norm(x, axis=1) for x in (b - a, c - b, a - c)]
    longest, shortest = np.max(e, axis=0), np.min(e, axis=0)
    area2 = np.linalg.norm(np.cross(b - a, c - a), axis=1)
    # the smallest angle lies opposite the shortest edge: sin = 2 area / (product of the other two)
    sin_min = area2 * shortest / (e[0] * e[1] * e[2])
    keep = (shortest >= L_MIN) & (longest <= L_MAX) & (sin_min >= np.sin(np.radians(MIN_ANGLE_DEG))) & (np.abs(np.stack([a, b, c])).max(axis=(0, 2)) <= 1.0)
    a, b, c = (x[keep][:n].astype(F32) for x in (a, b, c))
    d = rng.normal(size=a.shape)
    q = ((a.astype(F64) + b + c) / 3 + d / np.linalg.norm(d, axis=1)[:, None] * rng.uniform(0, OFFSET, size=(a.shape[0], 1))).astype(F32)
    return a, b, c, q


def test_restatement_against_float64():
    a, b, c, q = well_shaped(2000, 7)
    assert a.shape[0] == 2000
    # the stated conditions hold for the float32 inputs
    A, B, C, Q = (x.astype(F64) for x in (a, b, c, q))
    e = [np.linalg.norm(x, axis=1) for x in (B - A, C - B, A - C)]
    assert np.min(e) >= L_MIN * (1 - 1e-6) and np.max(e) <= L_MAX * (1 + 1e-6)
    sin_min = np.linalg.norm(np.cross(B - A, C - A), axis=1) * np.min(e, axis=0) / (e[0] * e[1] * e[2])
    assert sin_min.min() >= np.sin(np.radians(MIN_ANGLE_DEG)) * (1 - 1e-6)
    assert max(np.linalg.norm(Q - X, axis=1).max() for X in (A, B, C)) <= P_MAX and max(np.abs(x).max() for x in (a, b, c, q)) <= M_MAX
    d2, region, pts, bary = R.evaluate(comps(q), comps(a), comps(b), comps(c))
    assert d2.dtype == F32 and all(p.dtype == F32 for p in pts)
    want = R.distance64(Q, A, B, C) ** 2
    err = np.abs(d2.astype(F64) - want)
    bound = d2_bound()
    print(f"float64: max |d2 - d2_64| = {err.max():.3e}, bound {bound:.3e}; regions {np.bincount(region, minlength=7).tolist()}")
    assert bound < 1e-4 and err.max() <= bound
    assert (np.bincount(region, minlength=7) > 20).all()                       # every region is exercised
    # barycentrics: in [0, 1], and they sum to one within two roundings
    bs = np.stack(bary, axis=1).astype(F64)
    assert bs.min() >= 0.0 and bs.max() <= 1.0 and np.abs(bs.sum(axis=1) - 1.0).max() <= 4 * U


# ---- planted points --------------------------------------------------------------------------------------------------------------------
TRI_V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, -1, 0]], dtype=F32)


def planted_points():
    """(query, region, closest point, barycentrics, d2) on the triangle (0,0,0) (1,0,0) (0,1,0): every number is a dyadic fraction, so the
    float32 sequence is exact."""
    return [
        ((-1, -1, 1), "A", (0, 0, 0), (1, 0, 0), 3.0),
        ((2, -1, 0.5), "B", (1, 0, 0), (0, 1, 0), 2.25),
        ((-1, 2, 0.25), "C", (0, 1, 0), (0, 0, 1), 2.0625),
        ((0.25, -1, 0.5), "AB", (0.25, 0, 0), (0.75, 0.25, 0), 1.25),
        ((-1, 0.25, 0.5), "AC", (0, 0.25, 0), (0.75, 0, 0.25), 1.25),
        ((1, 1, 0.5), "BC", (0.5, 0.5, 0), (0, 0.5, 0.5), 0.75),
        ((0.25, 0.25, 2), "IN", (0.25, 0.25, 0), (0.5, 0.25, 0.25), 4.0),
        ((1, 0, 0), "B", (1, 0, 0), (0, 1, 0), 0.0),                            # on a vertex
        ((0.5, 0, 0), "AB", (0.5, 0, 0), (0.5, 0.5, 0), 0.0),                    # on an edge
        ((0.25, 0.25, 0), "IN", (0.25, 0.25, 0), (0.5, 0.25, 0.25), 0.0),        # in the plane
    ]


def test_planted_points_in_all_seven_regions():
    rows = planted_points()
    q = np.array([r[0] for r in rows], dtype=F32)
    got = R.closest(TRI_V, np.array([[0, 1, 2]], np.int32), q, 10.0, 1.0)
    assert [R.REGIONS[r] for r in got["region"]] == [r[1] for r in rows]
    assert set(r[1] for r in rows) == set(R.REGIONS)
    assert np.array_equal(got["point"], np.array([r[2] for r in rows], dtype=F32))
    assert np.array_equal(got["barycentric"], np.array([r[3] for r in rows], dtype=F32))
    assert np.array_equal(got["d2"], np.array([r[4] for r in rows], dtype=F32))
    assert (got["triangle"] == 0).all() and got["counts"] == [len(rows), 0, 0, 0]


def test_ties_go_to_the_lower_index():
    q = np.array([[0.5, 0, 1], [0.25, 0, 0]], dtype=F32)                       # above the shared edge; on it
    for tris in ([[0, 1, 2], [0, 1, 3]], [[0, 1, 3], [0, 1, 2]], [[0, 1, 2], [0, 1, 2]], [[1, 2, 0], [0, 1, 2], [0, 1, 3]]):
        got = R.closest(TRI_V, np.array(tris, np.int32), q, 10.0, 0.5)
        assert got["triangle"].tolist() == [0, 0] and got["d2"].tolist() == [1.0, 0.0], tris


def test_classes_and_limits():
    nan = np.nan
    v = np.concatenate([TRI_V, [[nan, 0, 0], [2, 0, 0], [3, 0, 0], [1e30, 0, 0]]]).astype(F32)
    tris = np.array([[0, 1, 2], [0, 1, 4], [0, 1, 8], [-1, 0, 1], [0, 5, 6], [1, 1, 2], [0, 1, 7]], np.int32)
    cls, _, _ = R.classify(v, tris, 0.5)
    assert cls.tolist() == [R.USABLE, R.TRI_SKIPPED, R.TRI_BAD_INDEX, R.TRI_BAD_INDEX, R.TRI_DEGENERATE, R.TRI_DEGENERATE, R.TRI_SKIPPED]
    assert R.registration(v, tris, 0.5)[:5] == [1, 0, 2, 2, 2] and R.registration(v, tris, 0.5)[7] == R.BAD_INDEX
    assert R.registration(v, tris, 0.5, max_cells=-1)[:2] == [0, 1] and R.registration(v, tris, 0.01)[:2] == [0, 1]
    q = np.array([[0.25, 0.25, 2], [0.25, 0.25, np.nextafter(F32(2), F32(3))], [nan, 0, 0], [np.inf, 0, 0], [1e9, 0, 0]], dtype=F32)
    got = R.closest(v, tris, q, 2.0, 0.5)                                      # exactly at max_distance: inside; one ulp beyond: far
    assert got["triangle"].tolist() == [0, -1, -1, -1, -1] and got["counts"] == [1, 1, 3, 0]
    assert got["d2"].tolist()[0] == 4.0 and np.isinf(got["d2"][1:]).all() and np.isnan(got["point"][1:]).all() and np.isnan(got["barycentric"][1:]).all()


# ---- the sphere ------------------------------------------------------------------------------------------------------------------------
def test_sphere_distances_lie_within_the_sag():
    radius = 0.5
    v, tris = S.uv_sphere(radius)
    assert tris.shape[0] == 1984
    V64 = v.astype(F64)
    a, b, c = (V64[tris[:, k]] for k in range(3))
    sag = float((radius - R.distance64(np.zeros_like(a), a, b, c)).max())        # the deepest point of any facet below the sphere
    assert 0 < sag < 0.01
    rng = np.random.default_rng(3)
    d = rng.normal(size=(900, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    r = np.repeat([0.3, 0.5, 0.7], 300)
    q = (d * r[:, None]).astype(F32)
    got = R.closest(v, tris, q, 1.0, R.default_cell(v, tris))
    assert got["counts"] == [900, 0, 0, 0]
    dist = np.sqrt(got["d2"].astype(F64))
    rq = np.linalg.norm(q.astype(F64), axis=1)
    eps = 64 * U                                                               # float32 coordinates of magnitude below 1, a handful of roundings
    lo, hi = np.abs(rq - radius) - sag - eps, np.abs(rq - radius) + sag + eps
    print(f"sphere: sag {sag:.6f}, distance - |r - R| in [{(dist - np.abs(rq - radius)).min():.6f}, {(dist - np.abs(rq - radius)).max():.6f}]")
    assert (dist >= lo).all() and (dist <= hi).all()
    # the closest point is on the named triangle: its barycentrics reproduce it
    p = (got["barycentric"][:, :, None].astype(F64) * V64[tris[got["triangle"]]]).sum(axis=1)
    assert np.abs(p - got["point"]).max() <= 8 * U


# ---- interpolate -----------------------------------------------------------------------------------------------------------------------
def test_interpolate_reproduces_the_point():
    v, tris = S.uv_sphere(0.5)
    rng = np.random.default_rng(5)
    q = rng.uniform(-0.7, 0.7, size=(500, 3)).astype(F32)
    q[::50] = 5.0                                                              # far
    got = R.closest(v, tris, q, 0.8, 0.1)                                      # (the cube's corners lie 0.72 from the sphere)
    assert got["counts"][1] == 10
    T = torch.from_numpy
    out = M.interpolate(T(tris), T(got["triangle"]), T(got["barycentric"]), T(v)).numpy()
    found = got["triangle"] >= 0
    assert out.dtype == F32 and np.isnan(out[~found]).all() and np.abs(out[found].astype(F64) - got["point"][found]).max() <= 8 * U * 0.5 * 2
    std = rng.random(v.shape[0]).astype(F32)
    one = M.interpolate(T(tris), T(got["triangle"]), T(got["barycentric"]), T(std)).numpy()
    b, x = got["barycentric"][found], std[tris[got["triangle"][found]]]
    assert one.shape == (500,) and np.isnan(one[~found]).all()
    assert np.array_equal(one[found], (b[:, 0] * x[:, 0] + b[:, 1] * x[:, 1]) + b[:, 2] * x[:, 2])


def test_default_cell_is_a_float32_and_positive():
    v, tris = S.uv_sphere(0.5)
    c = R.default_cell(v, tris)
    assert c == float(F32(c)) and 0.05 < c < 0.3
    assert R.default_cell(v, np.zeros((0, 3), np.int32)) == 1.0 and R.default_cell(np.zeros((0, 3), F32), tris) == 1.0


# ---- the margins of the grid search ------------------------------------------------------------------------------------------------------
def test_planted_slack_cases_fail_without_the_margins():
    """The cases of tests/closest_slack.py, on the CPU: the search as the kernel states it (box test, ring bound, slack, widening) gives the
    all-pairs answer on every one of them, and with both margins off it gives a WRONG answer on most (not all: a T whose sideways extent
    crosses a cell border sits in a second cell with a box test of its own; at least half is asserted) — so the GPU test that holds the
    kernel to the all-pairs answer on these cases does discriminate.  Either margin alone covers the other here (printed; closest_slack.py
    says why), and at three cells: the cases are built for the cell they are searched with."""
    for cell in (0.05, 0.05 * 0.37, 0.05 * 2.9):
        v, tris, q = K.planted_cases(cell)
        r = 2.4 * cell
        assert q.shape[0] >= 40, cell
        want = R.closest(v, tris, q, r, cell)
        assert want["counts"] == [q.shape[0], 0, 0, 0]
        wrong = {}
        for slack, widen in ((True, True), (False, True), (True, False), (False, False)):
            d2, t = K.search(v, tris, q, r, cell, slack, widen)
            wrong[(slack, widen)] = int(((t != want["triangle"]) | (d2.view(np.uint32) != want["d2"].view(np.uint32))).sum())
        print(f"cell {cell:.4f}: {q.shape[0]} cases; wrong answers with (slack, widening) = " + ", ".join(f"{k}: {n}" for k, n in wrong.items()))
        assert wrong[(True, True)] == 0 and wrong[(False, False)] >= q.shape[0] // 2
