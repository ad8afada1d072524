"""GPU: `dif_mesh_simplify` against its numpy restatement (tests/simplify_ref.py), byte for byte — every array, every count — on an analytic
sphere, on planted vertices and triangles at every edge of the contract, on random soups around the scan and wave boundaries with hot
clusters, on 4,097 vertices in one cell; its refusals; colours carried; and through `DenseIndexedMap.indexed_mesh(simplify_cell=...)` on the
two-sphere scene."""
import ctypes

import numpy as np
import pytest
import torch

from di_fusion_amd import _lib, synthetic as syn
from di_fusion_amd.system import mesh as M
from di_fusion_amd.system.map import DenseIndexedMap
from tests import components_ref as C
from tests import simplify_ref as S
from tests import weld_ref as W
from tests.test_weld_cpu import read_ply

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F32 = np.float32
RADIUS = 0.5
ORIGIN = (-2.0, -2.0, -2.0)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def gpu_simplify(v, std, tris, ids, cell, origin, colors=None, weight=None):
    return M.simplify(dev(v), dev(std), dev(tris), dev(ids), cell, origin, None if colors is None else dev(colors), None if weight is None else dev(weight))


def assert_same(got: M.IndexedMesh, want: dict, what):
    """`test_gpu_components.py:assert_same_mesh` over all nine counts, plus vertex_cluster (and the colours when there are any)."""
    assert [got.counts[k] for k in S.COUNT_NAMES] == want["counts"], (what, got.counts, want["counts"])
    g = got.cpu()
    assert g.triangles.dtype == torch.int32 and g.triangle_flatten_id.dtype == torch.int64 and g.vertex_cluster.dtype == torch.int32
    names = S.MESH_NAMES + ("vertex_cluster",) + (("colors", "color_weight") if "colors" in want else ())
    for name in names:
        a, b = getattr(g, name).numpy(), want[name]
        assert a.shape == b.shape and np.array_equal(a.view(np.uint8), np.ascontiguousarray(b).view(np.uint8)), (what, name)
    if "colors" in want:
        assert got.counts["coloured"] == want["coloured"], what
    else:
        assert g.colors is None and g.color_weight is None


def check(v, std, tris, ids, cell, origin, what, colors=None, weight=None):
    want = S.simplify(v, std, tris, ids, cell, origin, colors, weight)
    got = gpu_simplify(v, std, tris, ids, cell, origin, colors, weight)
    assert_same(got, want, what)
    return got, dict(zip(S.COUNT_NAMES, want["counts"]))


# ---- the sphere ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sphere():
    v, tris = S.uv_sphere(RADIUS)
    return (v, tris) + S.attributes(v.shape[0], tris.shape[0])


@pytest.mark.parametrize("cell,share", [(0.085, 1 / 2), (0.18, 1 / 8), (0.6, 1 / 64)])
def test_sphere(sphere, cell, share):
    v, tris, std, ids = sphere
    got, c = check(v, std, tris, ids, cell, ORIGIN, f"sphere {cell}")
    print(f"sphere, cell {cell}: {c}, {c['vertices'] / v.shape[0]:.4f} of the vertices")
    assert 0.6 * share < c["vertices"] / v.shape[0] < 1.5 * share
    assert got.counts["cell"] == float(F32(cell)) and got.counts["origin"] == ORIGIN


def test_sphere_nothing_merges_and_everything_collapses(sphere):
    v, tris, std, ids = sphere
    cell = S.smallest_distance(v) / np.sqrt(3.0) * 0.99
    got, c = check(v, std, tris, ids, cell, ORIGIN, "nothing merges")
    assert [c[k] for k in S.COUNT_NAMES] == [v.shape[0], tris.shape[0], 0, 0, 0, 0, 0, 0, 0]
    assert np.array_equal(got.triangles.cpu().numpy(), tris) and np.array_equal(got.vertex_cluster.cpu().numpy(), np.arange(v.shape[0]))
    got, c = check(v, std, tris, ids, 8.0, (-4.0, -4.0, -4.0), "everything collapses")
    assert [c[k] for k in S.COUNT_NAMES] == [0, 0, 0, tris.shape[0], 0, 1, 0, 0, 0]
    assert got.vertices.shape == (0, 3) and got.triangles.shape == (0, 3) and (got.vertex_cluster.cpu().numpy() == -1).all()


# ---- planted vertices and triangles ----------------------------------------------------------------------------------------------------
CELL, PORIGIN = 0.25, (-1.0, -1.0, -1.0)


def planted():
    """origin -1, cell 0.25: p = -1 + k / 4 is representable for every k used here."""
    up, down = (lambda x: np.nextafter(F32(x), F32(np.inf))), (lambda x: np.nextafter(F32(x), F32(-np.inf)))
    edge = F32(-1.0 + 3 * 0.25)                                    # the boundary between cells 2 and 3
    last = F32(-1.0 + (2 ** 21 - 1 + 0.5) * 0.25)                  # the middle of cell 2^21 - 1
    past = F32(-1.0 + 2 ** 21 * 0.25)                              # the start of cell 2^21: not keyed
    assert float(edge) == -0.25 and float(last) == 524286.875 and float(past) == 524287.0
    v = np.array([
        [edge, 0.1, 0.1], [up(edge), 0.1, 0.1], [down(edge), 0.1, 0.1],            # 0-2: on the boundary (cell 3), above it (3), below it (2)
        [0.1, edge, 0.15], [0.1, down(edge), 0.15], [0.12, 0.12, down(edge)],      # 3-5: the same on the other axes
        [last, 0.1, 0.1], [past, 0.1, 0.1], [0.1, last, 0.1], [0.1, 0.1, past],    # 6-9: the last cell and past it
        [-1.5, 0.1, 0.1], [down(-1.0), 0.1, 0.1], [-1.0, -1.0, -1.0],              # 10-12: below the origin (twice), the origin itself (cell 0)
        [np.nan, 0.1, 0.1], [0.1, np.inf, 0.1], [0.1, 0.1, -np.inf],               # 13-15
        [0.6, 0.6, 0.6], [0.61, 0.62, 0.63], [0.7, 0.7, 0.7], [0.74, 0.6, 0.7],    # 16-19: one cell, for the stds
        [0.3, 0.3, 0.3], [0.31, 0.3, 0.3], [0.3, 0.3, 0.31],                       # 20-22: one cell whose stds are all invalid
        [-0.6, -0.6, -0.6], [-0.3, -0.6, -0.6], [-0.6, -0.3, -0.6], [-0.6, -0.6, -0.3], [-0.59, -0.6, -0.6],   # 23-27: a tetrahedron's cells, 27 with 23
    ], dtype=F32)
    std = np.full(v.shape[0], 0.5, dtype=F32)
    std[[16, 17, 18, 19]] = [np.nan, -1.0, 100.0, 0.25]            # one valid member and one clamped to 64
    std[[20, 21, 22]] = [np.nan, -np.inf, np.inf]
    std[13] = np.array([0x7FC12345], dtype=np.uint32).view(F32)[0]      # a NaN with a payload on a vertex that is copied
    std[12] = -0.0                                                  # (>= 0: valid)
    V = v.shape[0]
    tris = np.array([
        [0, 2, 16], [1, 2, 16], [2, 16, 0],                       # 0 and 1 share a cell: the second is a duplicate, the third the first rotated
        [0, 16, 2],                                                # the other orientation: stays
        [3, 4, 5], [6, 7, 8], [7, 9, 8],                           # across boundaries; with unkeyed corners
        [6, 8, 12],                                                # FLAT: two edges of 2^21 cells
        [10, 11, 12], [13, 14, 15], [13, 14, 15], [15, 13, 14], [14, 13, 15],       # unkeyed corners: each its own cluster; exact and rotated duplicates, one flipped
        [16, 17, 20], [18, 19, 21],                                # collapsed
        [16, 20, 23], [19, 22, 27], [17, 21, 23],                  # duplicates by cluster
        [0, 1, V], [0, -1, 3], [V, V, V], [2 ** 31 - 1, 0, 1], [-2 ** 31, 0, 1],     # bad indices
        [23, 25, 24], [23, 24, 26], [24, 25, 26], [25, 23, 26], [27, 24, 26],       # the tetrahedron and a duplicate by cluster
        [5, 5, 6], [7, 7, 7],                                      # a repeated index
    ], dtype=np.int32)
    ids = (np.arange(tris.shape[0], dtype=np.int64) << 33) + 5
    return v, std, tris, ids


def test_planted_vertices_and_triangles():
    v, std, tris, ids = planted()
    got, c = check(v, std, tris, ids, CELL, PORIGIN, "planted")
    print("planted:", c)
    vc = got.vertex_cluster.cpu().numpy()
    # what the contract says about them, spelled out (the byte comparison above covers the values)
    assert vc[0] == vc[1] != vc[2] and vc[3] != vc[4] and c["unkeyed"] == 7 and c["flat"] >= 1 and c["status"] == _lib.MESH_STATUS_BAD_INDEX
    assert c["bad_std"] == 5 and c["triangles"] + 5 + c["collapsed"] + c["duplicate"] == tris.shape[0]
    g = got.cpu()
    assert np.isnan(g.vertex_std.numpy()[vc[20]]) and g.vertex_std.numpy()[vc[16]] == F32((64.0 + 0.25) / 2)
    assert g.vertex_std.numpy()[vc[13]].view(np.uint32) == 0x7FC12345 and np.isnan(g.vertices.numpy()[vc[13], 0])
    kept_ids = set(((g.triangle_flatten_id.numpy() - 5) >> 33).tolist())
    assert {0, 3, 9, 12}.issubset(kept_ids) and not {1, 2, 10, 11, 16, 17}.intersection(kept_ids)
    # the same without the bad triangles: status 0, everything else unchanged
    ok = ((tris >= 0) & (tris < v.shape[0])).all(axis=1)
    got2, c2 = check(v, std, tris[ok], ids[ok], CELL, PORIGIN, "planted, valid only")
    assert c2["status"] == 0 and dict(c2, status=1) == c
    assert got2.cpu().vertices.numpy().tobytes() == g.vertices.numpy().tobytes()


# ---- soups -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("K", [1, 63, 64, 65, 4096, 4097, 20000])
def test_random_soup(K, seed):
    """5,000 vertices from 400 cells: hot slots; K either side of a wave, of the single-workgroup scan's limit, and several scan blocks."""
    v, tris = S.soup(5000, K, 400, seed, CELL, PORIGIN)
    rng = np.random.default_rng(seed + 10)
    std = rng.random(5000).astype(F32) * 70.0                       # some above the clamp
    ids = rng.integers(0, 2 ** 40, size=K).astype(np.int64)
    got, c = check(v, std, tris, ids, CELL, PORIGIN, f"soup {K} / {seed}")
    print(f"soup {K} / {seed}: {c}")
    if K == 20000:
        assert c["duplicate"] > 5000 and c["collapsed"] > 0 and c["vertices"] == 400
        again = gpu_simplify(v, std, tris, ids, CELL, PORIGIN)
        g, a = got.cpu(), again.cpu()
        for name in S.MESH_NAMES + ("vertex_cluster",):
            assert getattr(g, name).numpy().tobytes() == getattr(a, name).numpy().tobytes(), name
        assert got.counts == again.counts


@pytest.mark.parametrize("V", [4097, 5000])
def test_vertex_scan_seams(V):
    """Nothing merges on a soup of V vertices, one per cell: the vertex scan across its single-workgroup limit, every vertex a cluster."""
    rng = np.random.default_rng(V)
    cells = rng.choice(24 ** 3, size=V, replace=False)
    v = (np.asarray(PORIGIN) + (np.stack([cells // 576, (cells // 24) % 24, cells % 24], axis=1) + rng.random((V, 3)) * 0.9 + 0.05) * CELL).astype(F32)
    tris = rng.integers(0, V, size=(3000, 3)).astype(np.int32)
    got, c = check(v, rng.random(V).astype(F32), tris, np.arange(3000, dtype=np.int64), CELL, PORIGIN, f"one vertex per cell, {V}")
    assert c["isolated"] > 0 and c["vertices"] + c["isolated"] == V


def test_one_cell_of_4097_vertices():
    """The worst contention: every vertex adds to one row, every triangle has the same triple."""
    rng = np.random.default_rng(3)
    n = 4097
    v = np.concatenate([(np.asarray(PORIGIN) + (np.array([5, 6, 7]) + rng.random((n, 3))) * CELL), [[0.9, 0.9, 0.9], [-0.9, 0.9, 0.1]]]).astype(F32)
    tris = np.stack([np.arange(n), np.full(n, n), np.full(n, n + 1)], axis=1).astype(np.int32)
    tris[1::2] = tris[1::2][:, [2, 0, 1]]                           # every other one rotated
    colors = rng.integers(0, 256, size=(n + 2, 3), dtype=np.uint8)
    weight = rng.random(n + 2).astype(F32)
    got, c = check(v, rng.random(n + 2).astype(F32), tris, np.arange(n, dtype=np.int64), CELL, PORIGIN, "one cell", colors, weight)
    assert [c[k] for k in ("vertices", "triangles", "collapsed", "duplicate", "isolated")] == [3, 1, 0, n - 1, 0]
    assert got.triangles.cpu().tolist() == [[0, 1, 2]] and got.triangle_flatten_id.cpu().tolist() == [0]


@pytest.mark.parametrize("V,K", [(0, 0), (5, 0), (0, 3)])
def test_empty_inputs(V, K):
    rng = np.random.default_rng(0)
    v = rng.random((V, 3)).astype(F32)
    v[:, 0] = np.arange(V) * 0.3                                    # a cell each
    tris = np.zeros((K, 3), dtype=np.int32)
    got, c = check(v, np.ones(V, dtype=F32), tris, np.arange(K, dtype=np.int64), CELL, PORIGIN, f"V {V}, K {K}")
    assert c["vertices"] == 0 and c["triangles"] == 0 and c["isolated"] == V and c["status"] == (1 if K else 0)
    assert got.vertices.shape == (0, 3) and got.triangles.shape == (0, 3) and got.vertex_cluster.shape == (V,)


# ---- colours ---------------------------------------------------------------------------------------------------------------------------
def test_colours_are_carried(sphere):
    v, tris, std, ids = sphere
    rng = np.random.default_rng(2)
    colors = rng.integers(0, 256, size=(v.shape[0], 3), dtype=np.uint8)
    weight = (rng.random(v.shape[0]) * 40.0).astype(F32)
    weight[::7] = 0.0
    weight[3::50] = [np.nan, np.inf, -np.inf, -3.0, 1e30] * 4
    for cell in (0.0055, 0.085, 0.6):
        got, c = check(v, std, tris, ids, cell, ORIGIN, f"colours {cell}", colors, weight)
        print(f"colours, cell {cell}: {c}, coloured {got.counts['coloured']}")
    # through the mesh object: colors / color_weight go in, the resolved cluster colours come out; without them nothing is invented
    m = M.IndexedMesh(dev(v), dev(np.zeros_like(v)), dev(std), dev(tris), dev(ids), {}, dev(colors), dev(weight))
    assert_same(m.simplify(0.085, ORIGIN), S.simplify(v, std, tris, ids, 0.085, ORIGIN, colors, weight), "IndexedMesh.simplify, coloured")
    plain = M.IndexedMesh(dev(v), dev(np.zeros_like(v)), dev(std), dev(tris), dev(ids), {})
    assert_same(plain.simplify(0.085, ORIGIN), S.simplify(v, std, tris, ids, 0.085, ORIGIN), "IndexedMesh.simplify")


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def raw_call(**over):
    """`dif_mesh_simplify` on a valid small mesh with some arguments replaced; returns the code."""
    lib = _lib.load()
    v, tris = S.tetrahedron()
    V, K = 4, 4
    ws_bytes = int(lib.dif_mesh_simplify_workspace_bytes(V, K))
    t = dict(vertices=dev(v), vertex_std=dev(np.ones(V, F32)), triangles=dev(tris), triangle_id=dev(np.arange(K, dtype=np.int64)), rgb=None, weight=None,
             ws=torch.empty((ws_bytes + 16,), dtype=torch.uint8, device=DEV), out_v=torch.empty((V, 3), device=DEV), out_n=torch.empty((V, 3), device=DEV),
             out_s=torch.empty((V,), device=DEV), out_t=torch.empty((K, 3), dtype=torch.int32, device=DEV), out_i=torch.empty((K,), dtype=torch.int64, device=DEV),
             accum=None, cluster=torch.empty((V,), dtype=torch.int32, device=DEV), counts=torch.zeros((_lib.SIMPLIFY_COUNT,), dtype=torch.int32, device=DEV))
    s = dict(V=V, K=K, ws_bytes=ws_bytes, ws_offset=0, cell=0.5, origin=(0.0, 0.0, 0.0), args=True)
    for k, x in over.items():
        (t if k in t else s)[k] = x
    a = _lib.DifSimplifyArgs()
    a.cell = s["cell"]
    for k in range(3):
        a.origin[k] = s["origin"][k]
    P = _lib.ptr
    ws = ctypes.c_void_p(t["ws"].data_ptr() + s["ws_offset"]) if t["ws"] is not None else ctypes.c_void_p(0)
    rc = lib.dif_mesh_simplify(P(t["vertices"]), P(t["vertex_std"]), P(t["triangles"]), P(t["triangle_id"]), s["V"], s["K"], P(t["rgb"]), P(t["weight"]),
                               ctypes.byref(a) if s["args"] else None, ws, s["ws_bytes"], P(t["out_v"]), P(t["out_n"]), P(t["out_s"]), P(t["out_t"]), P(t["out_i"]),
                               P(t["accum"]), P(t["cluster"]), P(t["counts"]), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc


def test_every_refusal():
    assert raw_call() == 0
    rgb, weight, accum = dev(np.zeros((4, 3), np.uint8)), dev(np.ones(4, F32)), M.colour_accumulator(4, DEV)
    assert raw_call(rgb=rgb, weight=weight, accum=accum) == 0
    refused = [dict(cell=0.0), dict(cell=-1.0), dict(cell=float("nan")), dict(cell=float("inf")), dict(origin=(0.0, float("nan"), 0.0)),
               dict(origin=(float("inf"), 0.0, 0.0)), dict(V=2 ** 31), dict(K=(2 ** 31 + 2) // 3), dict(V=-1), dict(K=-1),
               dict(rgb=rgb, accum=accum), dict(weight=weight, accum=accum), dict(rgb=rgb, weight=weight),
               dict(vertices=None), dict(vertex_std=None), dict(triangles=None), dict(triangle_id=None), dict(out_v=None), dict(out_n=None),
               dict(out_s=None), dict(out_t=None), dict(out_i=None), dict(cluster=None), dict(counts=None), dict(args=False),
               dict(ws=None), dict(ws_offset=8), dict(ws_bytes=int(_lib.load().dif_mesh_simplify_workspace_bytes(4, 4)) - 1)]
    for kw in refused:
        rc = raw_call(**kw)
        assert rc == -1, (kw.keys(), rc)
        with pytest.raises(RuntimeError, match="DIF_EINVAL"):
            _lib.check(rc, "dif_mesh_simplify")
    lib = _lib.load()
    assert lib.dif_mesh_simplify_workspace_bytes(2 ** 31, 0) == -1 and lib.dif_mesh_simplify_workspace_bytes(0, (2 ** 31 + 2) // 3) == -1
    assert lib.dif_mesh_simplify_workspace_bytes(-1, 0) == -1 and lib.dif_mesh_simplify_workspace_bytes(0, 0) > 0
    # and what the Python operator refuses before it calls
    v, tris = S.tetrahedron()
    std, ids = S.attributes(4, 4)
    for cell, origin in ((0.0, ORIGIN), (-0.5, ORIGIN), (float("nan"), ORIGIN), (float("inf"), ORIGIN), (1e-50, ORIGIN), (0.5, (0.0, float("nan"), 0.0)),
                         (0.5, (0.0, 1e39, 0.0))):
        with pytest.raises((RuntimeError, ValueError)):
            gpu_simplify(v, std, tris, ids, cell, origin)
    with pytest.raises((RuntimeError, ValueError)):
        gpu_simplify(v, std, tris, ids, 0.5, ORIGIN, colors=np.zeros((4, 3), np.uint8))
    with pytest.raises((RuntimeError, ValueError)):
        gpu_simplify(v, std, tris, ids, 0.5, ORIGIN, weight=np.ones(4, F32))
    with pytest.raises(RuntimeError):
        M.simplify(torch.from_numpy(v), dev(std), dev(tris), dev(ids), 0.5)                       # a host tensor
    with pytest.raises(RuntimeError):
        M.simplify(dev(v), dev(std), dev(tris.astype(np.int64)), dev(ids), 0.5)
    with pytest.raises(RuntimeError):
        M.simplify(dev(v), dev(std[:3]), dev(tris), dev(ids), 0.5)


# ---- through the map -------------------------------------------------------------------------------------------------------------------
VIEW = (48, 64, (60.0, 60.0, 32.0, 24.0))


@pytest.fixture(scope="module")
def two_sphere_map(gpu_model):
    b = W.SPHERE_BOUND
    cfg = syn.MapConfig((-b, -b, -b), (b, b, b), W.SPHERE_VOXEL)
    m = DenseIndexedMap(gpu_model, cfg.namespace(), 29, DEV, initial_capacity=1024)
    xyz, nrm = C.two_sphere_cloud()
    m.integrate_keyframe(dev(xyz), dev(nrm))
    m.extract_mesh_arrays(W.SPHERE_RES, int(4e6), fast=True, max_std=2000.0, to_host=False)
    return m


def mesh_bytes(m: M.IndexedMesh):
    g = m.cpu()
    return [getattr(g, name).numpy().tobytes() for name in S.MESH_NAMES]


def test_through_the_map(two_sphere_map, tmp_path):
    m = two_sphere_map
    full = m.indexed_mesh()
    off = m.indexed_mesh(simplify_cell=0)
    assert mesh_bytes(off) == mesh_bytes(full) and off.counts == full.counts and off.vertex_cluster is None
    culled = m.indexed_mesh(min_component_triangles=500)
    step = F32(W.SPHERE_VOXEL) / F32(W.SPHERE_RES)
    cell = 2.0 * float(step)
    small = m.indexed_mesh(min_component_triangles=500, simplify_cell=cell)
    origin = small.counts["origin"]
    assert origin == tuple(float(F32(-W.SPHERE_BOUND) - step / F32(2)) for _ in range(3)) and small.counts["cell"] == float(F32(cell))
    h = culled.cpu()
    want = S.simplify(h.vertices.numpy(), h.vertex_std.numpy(), h.triangles.numpy(), h.triangle_flatten_id.numpy(), cell, origin)
    assert_same(small, want, "through the map")
    print(f"two spheres at 2 lattice steps: {culled.counts['vertices']} -> {small.counts['vertices']} vertices, "
          f"{culled.counts['triangles']} -> {small.counts['triangles']} triangles; {small.counts}")
    assert 0 < small.counts["vertices"] < culled.counts["vertices"] < full.counts["vertices"] and small.counts["status"] == 0
    # the other operators take it as it is
    topo = small.topology()
    assert topo.count >= 1 and topo.status == 0
    small.write_ply(tmp_path / "small.ply")
    vert, face = read_ply(tmp_path / "small.ply")
    g = small.cpu()
    ref = np.concatenate([g.vertices.numpy(), g.normals.numpy(), g.vertex_std.numpy()[:, None]], axis=1)
    assert np.array_equal(np.stack([vert[k] for k in vert.dtype.names], axis=1).view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(face["v"], g.triangles.numpy())
    # the render: a cluster mean lies within d = sqrt(3) cell of each of its members, so the surface cannot move further
    H, Wd, intr = VIEW
    pose = np.eye(4)
    pose[:3, 3] = np.array([0.013, -0.021, 0.007]) + np.array([0.0, 0.0, -2.0])
    a, b = culled.render(pose, intr, H, Wd).depth.cpu().numpy(), small.render(pose, intr, H, Wd).depth.cpu().numpy()
    both = np.isfinite(a) & np.isfinite(b)
    median = float(np.median(np.abs(a[both] - b[both])))
    d = np.sqrt(3.0) * cell
    print(f"render: {int(both.sum())} pixels hit by both, median depth difference {median:.6f} m, d = {d:.6f} m")
    assert both.sum() > 400 and median < d
