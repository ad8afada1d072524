"""CPU: the numpy restatement of the mesh simplification (tests/simplify_ref.py) held to properties that follow from the contract of
`dif_mesh_simplify` (include/difusion.h) and from geometry, not from any code under test — on a UV sphere, a flat grid and a tetrahedron built
here.  tests/test_gpu_simplify.py then holds the kernels to the restatement byte for byte.  The last test needs the built library's binding
only (no GPU): the public names the feature adds."""
import numpy as np
import pytest

from tests import simplify_ref as S

F32, F64 = np.float32, np.float64
RADIUS = 0.5
ORIGIN = (-2.0, -2.0, -2.0)
MESHES = {"sphere": lambda: S.uv_sphere(RADIUS), "grid": S.flat_grid, "tetrahedron": S.tetrahedron}
CELLS = [0.03, 0.0625, 0.11, 0.17, 0.3]


def run(v, tris, cell, origin=ORIGIN, seed=0, **kw):
    std, ids = S.attributes(v.shape[0], tris.shape[0], seed)
    return S.simplify(v, std, tris, ids, cell, origin, **kw), std, ids


def own_cells(v, cell, origin):
    """The cell triple of every vertex, straight from the definition."""
    return np.floor((v.astype(F64) - np.asarray(origin, dtype=F32).astype(F64)) / F64(F32(cell))).astype(np.int64)


def check_structure(res, v, tris, cell, origin):
    V, K = v.shape[0], tris.shape[0]
    c = dict(zip(S.COUNT_NAMES, res["counts"]))
    out_t, vc, kept = res["triangles"], res["vertex_cluster"], res["kept"]
    bad = int((~((tris >= 0) & (tris < V)).all(axis=1)).sum())
    # the classes partition K
    assert c["triangles"] + bad + c["collapsed"] + c["duplicate"] == K and c["triangles"] == out_t.shape[0] == int(kept.sum())
    assert c["vertices"] == res["vertices"].shape[0] == res["normals"].shape[0] == res["vertex_std"].shape[0]
    # no output triangle repeats an index or a canonical triple; every output vertex is named
    assert (out_t[:, 0] != out_t[:, 1]).all() and (out_t[:, 1] != out_t[:, 2]).all() and (out_t[:, 0] != out_t[:, 2]).all()
    assert np.unique(S.canonical(out_t.astype(np.int64)), axis=0).shape[0] == out_t.shape[0]
    assert out_t.size == 0 or (out_t.min() >= 0 and out_t.max() < c["vertices"])
    assert np.array_equal(np.unique(out_t), np.arange(c["vertices"]))
    # vertex_cluster is consistent with the triangles, which keep their order and their ids
    assert np.array_equal(vc[tris[kept]], out_t)
    assert np.array_equal(res["triangle_flatten_id"], S.attributes(V, K)[1][kept])
    # two vertices share an output vertex exactly when they share a cell (all vertices of these meshes are keyed)
    cells = own_cells(v, cell, origin)
    named = vc >= 0
    _, cell_id = np.unique(cells, axis=0, return_inverse=True)
    cell_id = cell_id.reshape(-1)
    pairs = np.unique(np.stack([cell_id[named], vc[named]], axis=1), axis=0)
    assert np.unique(pairs[:, 0]).size == pairs.shape[0] == np.unique(pairs[:, 1]).size == c["vertices"]
    assert not np.isin(cell_id[~named], cell_id[named]).any()                     # a cell is named as a whole or not at all
    # numbering follows the lowest member id
    lowest = np.full((c["vertices"],), V, dtype=np.int64)
    np.minimum.at(lowest, vc[named], np.nonzero(named)[0])
    assert (np.diff(lowest) > 0).all()
    assert c["isolated"] == np.unique(cell_id).size - c["vertices"] and c["unkeyed"] == 0 and c["status"] == (1 if bad else 0)
    return c


@pytest.mark.parametrize("name", list(MESHES))
@pytest.mark.parametrize("cell", CELLS)
def test_output_structure_and_partition(name, cell):
    v, tris = MESHES[name]()
    res, _, _ = run(v, tris, cell)
    c = check_structure(res, v, tris, cell, ORIGIN)
    print(name, cell, c)
    # unit normals (or zero), finite positions inside the input's bounding box up to the rounding of test_nothing_merges
    n = np.linalg.norm(res["normals"].astype(F64), axis=1)
    assert ((np.abs(n - 1) < 1e-6) | (n == 0)).all()
    tol = cell * 2.0 ** -17 + np.spacing(np.abs(v).max().astype(F32))
    assert c["vertices"] == 0 or ((res["vertices"] >= v.min(axis=0) - tol).all() and (res["vertices"] <= v.max(axis=0) + tol).all())


@pytest.mark.parametrize("name", list(MESHES))
def test_nothing_merges(name):
    """A cell's diagonal is sqrt(3) cell: with every pair of vertices further apart than that, no two share a cell.  A lone member comes back as
    origin + (c + s / 65536) cell with |s / 65536 - f| <= 2^-17: off by at most cell 2^-17, half a float32 ulp of the result (at most one ulp of
    the coordinate, should the result sit in the next binade) and the float64 roundings of the five operations (8 x 2^-53 of the magnitudes)."""
    v, tris = MESHES[name]()
    cell = S.smallest_distance(v) / np.sqrt(3.0) * 0.99
    res, std, ids = run(v, tris, cell)
    assert res["counts"] == [v.shape[0], tris.shape[0], 0, 0, 0, 0, 0, 0, 0]
    assert np.array_equal(res["triangles"], tris) and np.array_equal(res["triangle_flatten_id"], ids)
    assert np.array_equal(res["vertex_cluster"], np.arange(v.shape[0]))
    bound = cell * 2.0 ** -17 + np.spacing(np.abs(v)).astype(F64) + 8 * 2.0 ** -53 * (np.abs(np.asarray(ORIGIN)) + np.abs(v.astype(F64)) + cell)
    moved = np.abs(res["vertices"].astype(F64) - v.astype(F64))
    print(name, "cell", cell, "largest move", moved.max(), "bound there", bound.reshape(-1)[moved.argmax()])
    assert (moved <= bound).all()
    # a lone member's std: llrint(std 2^24) / 2^24, rounded to float32 — exact for a float32 in [2^-1, 1), within 2^-25 below
    assert (np.abs(res["vertex_std"].astype(F64) - std.astype(F64)) <= 2.0 ** -25 + np.spacing(std).astype(F64)).all()


@pytest.mark.parametrize("cell", [0.03, 0.0625, 0.11, 0.17, 0.25])
def test_radius_bounds_on_the_sphere(cell):
    """m = the mean of members p_i with |p_i| in [r - delta, r + delta] (delta: the float32 rounding of the input, sqrt(3) half ulps).
    |m| <= max |p_i| (the ball is convex), and |m|^2 = mean |p_i|^2 - mean_ij |p_i - p_j|^2 / 2 >= (r - delta)^2 - d^2 / 2 since two points of one
    cell are less than d = sqrt(3) cell apart.  The output adds, per axis, cell 2^-17 (the fixed point: every s is within half a unit of f 65536),
    half a float32 ulp, and float64 roundings far below both (bounded here by another half ulp)."""
    v, tris = S.uv_sphere(RADIUS)
    res, _, _ = run(v, tris, cell)
    d = np.sqrt(3.0) * cell
    ulp = float(np.spacing(F32(RADIUS)))
    delta = np.sqrt(3.0) * 0.5 * ulp
    eps = np.sqrt(3.0) * (cell * 2.0 ** -17 + ulp)
    r = np.linalg.norm(res["vertices"].astype(F64), axis=1)
    lower = np.sqrt((RADIUS - delta) ** 2 - d * d / 2)
    print(f"cell {cell}: {r.size} vertices, |m| in [{r.min():.6f}, {r.max():.6f}], bounds [{lower - eps:.6f}, {RADIUS + delta + eps:.6f}]")
    assert r.size > 0 and (r >= lower - eps).all() and (r <= RADIUS + delta + eps).all()


@pytest.mark.parametrize("name", list(MESHES))
def test_everything_collapses(name):
    v, tris = MESHES[name]()
    res, _, _ = run(v, tris, 8.0, (-4.0, -4.0, -4.0))
    assert res["counts"] == [0, 0, 0, tris.shape[0], 0, 1, 0, 0, 0]
    assert res["vertices"].shape == (0, 3) and res["triangles"].shape == (0, 3) and (res["vertex_cluster"] == -1).all()


@pytest.mark.parametrize("cell", [0.0625, 0.17])
def test_permuting_the_triangles_moves_only_which_copy_stays(cell):
    """Duplicates on purpose: every triangle twice, the copy rotated.  The vertices do not depend on the triangle order; of each triple the
    triangle with the lowest NEW index stays."""
    v, tris = S.uv_sphere(RADIUS)
    tris = np.concatenate([tris, tris[:, [1, 2, 0]]])
    rng = np.random.default_rng(5)
    perm = rng.permutation(tris.shape[0])
    a, _, _ = run(v, tris, cell)
    b, _, _ = run(v, tris[perm], cell)
    assert a["counts"][3] > 0 and a["counts"][4] >= a["counts"][1] and a["counts"] == b["counts"]
    for name in ("vertices", "vertex_std", "vertex_cluster"):
        assert a[name].tobytes() == b[name].tobytes(), name
    # (not the normals: the kept copy may start at another corner, and its float32 cross product then rounds differently)
    canon = lambda t: {tuple(x) for x in S.canonical(t.astype(np.int64)).tolist()}
    assert canon(a["triangles"]) == canon(b["triangles"])
    # the kept copy: lowest position in the permuted order among the triangles of its triple
    triple = [tuple(x) for x in S.canonical(a["vertex_cluster"][tris].astype(np.int64)).tolist()]
    first = {}
    for new, old in enumerate(perm):
        t = triple[old]
        if len(set(t)) == 3 and t not in first:
            first[t] = new
    assert sorted(first.values()) == np.nonzero(b["kept"])[0].tolist()


def test_colours_of_a_cluster():
    """One colour per cell: every cluster keeps it exactly.  Weights are multiples of 1/16, so their sums are exact."""
    v, tris = S.uv_sphere(RADIUS)
    cell = 0.11
    cells = own_cells(v, cell, ORIGIN)
    colors = np.stack([(cells[:, 0] * 37 + 11) % 256, (cells[:, 1] * 91 + 5) % 256, (cells[:, 2] * 53 + 200) % 256], axis=1).astype(np.uint8)
    rng = np.random.default_rng(1)
    weight = (rng.integers(1, 64, size=v.shape[0]) / 16.0).astype(F32)
    res, _, _ = run(v, tris, cell, colors=colors, color_weight=weight)
    vc = res["vertex_cluster"]
    named = vc >= 0
    assert np.array_equal(res["colors"][vc[named]], colors[named])
    total = np.zeros((res["counts"][0],), dtype=F64)
    np.add.at(total, vc[named], weight[named].astype(F64))
    assert np.array_equal(res["color_weight"].astype(F64), total) and res["coloured"] == res["counts"][0]
    # two colours in one cluster: the weighted mean, rounded to nearest
    v2 = np.array([[0.01, 0.01, 0.01], [0.02, 0.01, 0.01], [0.3, 0.01, 0.01], [0.01, 0.3, 0.01]], dtype=F32)
    r2 = S.simplify(v2, np.zeros(4, F32), np.array([[0, 2, 3], [1, 2, 3]], np.int32), np.arange(2), 0.1, (0, 0, 0),
                    colors=np.array([[10, 0, 255], [20, 1, 0], [7, 7, 7], [9, 9, 9]], np.uint8), color_weight=np.array([1.0, 3.0, 0.0, np.inf], F32))
    assert r2["counts"][:5] == [3, 1, 0, 0, 1]
    assert r2["colors"].tolist() == [[18, 1, 64], [128, 128, 128], [128, 128, 128]] and r2["color_weight"].tolist() == [4.0, 0.0, 0.0] and r2["coloured"] == 1


def test_the_public_names_exist():
    from di_fusion_amd import _lib
    from di_fusion_amd.system import mesh as M
    from di_fusion_amd.system.map import DenseIndexedMap
    import inspect
    assert M.SIMPLIFY_COUNT_NAMES == S.COUNT_NAMES and _lib.SIMPLIFY_COUNT == 16 and _lib.SIMPLIFY_STATUS == 8
    assert {"dif_mesh_simplify", "dif_mesh_simplify_workspace_bytes"} <= set(_lib.SIGNATURES)
    assert inspect.signature(DenseIndexedMap.indexed_mesh).parameters["simplify_cell"].default == 0.0
    assert callable(M.simplify) and callable(M.IndexedMesh.simplify)
    a = M.simplify_args(0.25, (1.0, 2.0, 3.0))
    assert a.cell == 0.25 and list(a.origin) == [1.0, 2.0, 3.0]
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            M.simplify_args(bad)
    with pytest.raises(ValueError):
        M.simplify_args(1.0, (0.0, float("nan"), 0.0))
