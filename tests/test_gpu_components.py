"""GPU: `dif_mesh_components`, `dif_mesh_select` and `dif_mesh_edge_census` against their numpy restatement (tests/components_ref.py), bit for
bit — every array, every count, status 0 — on strips, fans, disjoint triangles and random meshes around the scan and wave boundaries; then
through `DenseIndexedMap.indexed_mesh()` on the two-sphere scene, where the census must find the two closed surfaces and
`remove_small_components` must leave exactly them."""
import numpy as np
import pytest
import torch

from di_fusion_amd import _lib, synthetic as syn
from di_fusion_amd.system import mesh as M
from di_fusion_amd.system.map import DenseIndexedMap
from tests import components_ref as C
from tests import weld_ref as W
from tests.test_weld_cpu import read_ply

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F32 = np.float32
SIZES = [1, 63, 64, 65, 4096, 4097]          # either side of a wave, a workgroup chunk and the single-workgroup scan's limit


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def check_topology(tris, V, what, want_status=0):
    """components + edge census on the GPU == the restatement; returns the restatement's answer"""
    want = C.topology(tris, V)
    t = dev(tris.astype(np.int32).reshape(-1, 3))
    got = M.components(t, V)
    assert got.count == want["count"] and got.status == want["status"] == want_status, (what, got.count, got.status)
    for name in ("vertex_component", "triangle_component", "n_vertices", "n_triangles"):
        g = getattr(got, name)
        assert g.dtype == torch.int32 and np.array_equal(g.cpu().numpy(), want[name]), (what, name)
    ne, nb, max_use, status = M.edge_census(t, got.vertex_component, got.count)
    assert np.array_equal(ne.cpu().numpy(), want["n_edges"]) and np.array_equal(nb.cpu().numpy(), want["n_boundary"]), what
    assert max_use == want["max_edge_use"] and status == want_status, (what, max_use, status)
    return want


# ---- components and edge census --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", SIZES)
def test_strips(K):
    tris, V = C.strip(K)
    want = check_topology(tris, V, f"strip {K}")
    assert want["count"] == 1 and want["n_edges"].tolist() == [2 * K + 1]
    check_topology((V - 1 - tris).astype(np.int32), V, f"strip {K}, ids reversed")       # every hook goes under a lower id: the longest parent chains
    check_topology(*C.relabel(tris, V, K), f"strip {K}, shuffled and relabelled")


@pytest.mark.parametrize("hub_high", [False, True])
def test_fans(hub_high):
    """One root under the most contention: every triangle names the hub."""
    want = check_topology(*C.fan(4097, hub_high), f"fan, hub {'highest' if hub_high else 'lowest'}")
    assert want["count"] == 1 and want["n_triangles"].tolist() == [4097]


@pytest.mark.parametrize("extra", [0, 700])
def test_disjoint_triangles(extra):
    """C = 1,366 (+ 700 unused vertices, each a component): the numbering scan across 4,096 vertices."""
    tris, V = C.disjoint(1366, extra)
    want = check_topology(tris, V, f"disjoint, {extra} unused")
    assert V == 4098 + extra and want["count"] == 1366 + extra


@pytest.mark.parametrize("K,seed", [(3000, 0), (3000, 1), (3000, 2), (850, 0)])
def test_random_meshes(K, seed):
    """K = 3,000: one giant component beside single triangles and unused vertices; K = 850 (V / 6, the percolation threshold): sizes of every order."""
    want = check_topology(*C.random_mesh(5000, K, seed), f"random {K} / {seed}")
    print(f"random {seed}: {want['count']} components, largest {int(want['n_triangles'].max())} triangles, max edge use {want['max_edge_use']}")


def test_tetrahedra_and_a_triple_used_edge():
    assert check_topology(C.TETRAHEDRON, 4, "tetrahedron")["euler"].tolist() == [2]
    want = check_topology(C.TETRAHEDRON[:3], 4, "tetrahedron minus a face")
    assert want["n_boundary"].tolist() == [3] and want["euler"].tolist() == [1]
    assert check_topology(np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]], dtype=np.int32), 5, "triple edge")["max_edge_use"] == 3
    check_topology(np.array([[0, 0, 1], [2, 2, 2]], dtype=np.int32), 4, "repeated indices")


def test_an_index_out_of_range_is_reported_and_never_followed():
    """The index V: the word past the end of every (V,) array lies inside the same allocation (they are 256-byte aligned), so a missing
    check shows as a wrong answer, never as a fault."""
    V = 100
    tris, _ = C.strip(V - 2)
    bad = np.concatenate([tris[:40], np.array([[7, V, 8]], dtype=np.int32), tris[40:]])
    want = check_topology(bad, V, "index V", want_status=C.BAD_INDEX)
    assert want["triangle_component"][40] == -1 and want["status"] == _lib.MESH_STATUS_BAD_INDEX
    rest = C.topology(tris, V)
    assert np.array_equal(want["vertex_component"], rest["vertex_component"]) and np.array_equal(want["n_triangles"], rest["n_triangles"])
    assert np.array_equal(want["n_edges"], rest["n_edges"])
    check_topology(np.array([[0, 1, -1]], dtype=np.int32), 3, "negative index", want_status=C.BAD_INDEX)


@pytest.mark.parametrize("V", [0, 5])
def test_empty_inputs(V):
    want = check_topology(np.zeros((0, 3), dtype=np.int32), V, f"no triangles, {V} vertices")
    assert want["count"] == V


# ---- select ----------------------------------------------------------------------------------------------------------------------------
def attributed(tris, V, seed=0):
    """An indexed mesh with random BITS for attributes (NaN payloads and all) on the host and on the GPU."""
    rng = np.random.default_rng(seed)
    v, n = (rng.integers(0, 2 ** 32, size=(V, 3), dtype=np.uint32).view(F32) for _ in range(2))
    s = rng.integers(0, 2 ** 32, size=(V,), dtype=np.uint32).view(F32)
    ids = rng.integers(0, 2 ** 40, size=(tris.shape[0],)).astype(np.int64)
    host = (v, n, s, tris.astype(np.int32).reshape(-1, 3), ids)
    return host, M.IndexedMesh(*(dev(a) for a in host), {})


def assert_same_mesh(got: M.IndexedMesh, want: dict, what):
    assert [got.counts[k] for k in ("vertices", "triangles", "status")] == want["counts"], (what, got.counts)
    g = got.cpu()
    assert g.triangles.dtype == torch.int32 and g.triangle_flatten_id.dtype == torch.int64
    for name in ("vertices", "normals", "vertex_std", "triangles", "triangle_flatten_id"):
        a, b = getattr(g, name).numpy(), want[name]
        assert a.shape == b.shape and np.array_equal(a.view(np.uint8), np.ascontiguousarray(b).view(np.uint8)), (what, name)


@pytest.mark.parametrize("K", [4096, 4097])
def test_select_masks(K):
    tris, V = C.relabel(*C.strip(K), seed=3)
    host, m = attributed(tris, V)
    everything = m.select(torch.ones(K, dtype=torch.bool, device=DEV))
    assert_same_mesh(everything, C.select(*host, np.ones(K, dtype=bool)), "all")
    assert_same_mesh(everything, dict(zip(("vertices", "normals", "vertex_std", "triangles", "triangle_flatten_id"), host), counts=[V, K, 0]), "all = the mesh")
    nothing = m.select(torch.zeros(K, dtype=torch.uint8, device=DEV))
    assert nothing.counts["vertices"] == 0 and nothing.counts["triangles"] == 0 and nothing.vertices.shape == (0, 3) and nothing.triangles.shape == (0, 3)
    for phase in (0, 1):
        keep = (np.arange(K) % 2) == phase
        assert_same_mesh(m.select(dev(keep)), C.select(*host, keep), f"alternating {phase}")


def test_select_by_component_keeps_ids_ascending(tmp_path):
    tris, V = C.random_mesh(5000, 3000, 1)
    host, m = attributed(tris, V, seed=4)
    c = m.components()
    keep = (c.n_triangles >= 3)[c.triangle_component.long()]
    want = C.select(*host, keep.cpu().numpy())
    got = m.select(keep)
    assert_same_mesh(got, want, "by component")
    assert 0 < got.counts["triangles"] < 3000
    # new vertex ids ascend with the old ones: the kept vertices are the used ones, in order
    used = np.zeros(V, dtype=bool)
    used[tris[keep.cpu().numpy()].reshape(-1)] = True
    assert np.array_equal(got.vertices.cpu().numpy().view(np.uint32), host[0][used].view(np.uint32))
    # flat function, and a kept triangle with a bad index is dropped and reported
    assert_same_mesh(M.select(m.vertices, m.normals, m.vertex_std, m.triangles, m.triangle_flatten_id, keep), want, "flat")
    bad = tris.copy()
    bad[5, 1] = V
    host_b, mb = attributed(bad, V, seed=4)
    ones = np.ones(3000, dtype=bool)
    want_b = C.select(*host_b, ones)
    assert want_b["counts"][1:] == [2999, C.BAD_INDEX]
    assert_same_mesh(mb.select(dev(ones)), want_b, "bad index")
    # PLY of a selection (finite attributes)
    tris, V = C.strip(65)
    rng = np.random.default_rng(0)
    host = (rng.standard_normal((V, 3)).astype(F32), rng.standard_normal((V, 3)).astype(F32), rng.random(V).astype(F32), tris, np.arange(65, dtype=np.int64))
    sel = M.IndexedMesh(*(dev(a) for a in host), {}).select(dev(np.arange(65) >= 32))
    sel.write_ply(tmp_path / "sel.ply")
    vert, face = read_ply(tmp_path / "sel.ply")
    g = sel.cpu()
    ref = np.concatenate([g.vertices.numpy(), g.normals.numpy(), g.vertex_std.numpy()[:, None]], axis=1)
    assert np.array_equal(np.stack([vert[k] for k in vert.dtype.names], axis=1).view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(face["v"], g.triangles.numpy()) and face["v"].shape == (33, 3) and face["v"].min() == 0 and face["v"].max() == 34


def test_remove_small_components_and_keep_largest():
    tris, V = C.random_mesh(5000, 3000, 2)
    host, m = attributed(tris, V, seed=5)
    for kw in (dict(min_triangles=4), dict(keep_largest=3), dict(min_triangles=2, keep_largest=1000), dict(), dict(min_triangles=10 ** 6), dict(keep_largest=0)):
        want, removed = C.remove_small_components(*host, **kw)
        got = m.remove_small_components(**kw)
        assert_same_mesh(got, want, str(kw))
        assert got.counts["components_removed"] == removed, kw
    # ties go to the lower component id
    tris, V = C.disjoint(1366)
    host, m = attributed(tris, V)
    got = m.remove_small_components(keep_largest=2)
    assert_same_mesh(got, C.remove_small_components(*host, keep_largest=2)[0], "ties")
    assert got.triangles.cpu().tolist() == [[0, 1, 2], [3, 4, 5]] and got.triangle_flatten_id.cpu().tolist() == host[4][:2].tolist()
    # an empty mesh
    empty = M.IndexedMesh(*(dev(a[:0]) for a in host), {}).remove_small_components(5)
    assert empty.counts == dict(vertices=0, triangles=0, status=0, components_removed=0)


def test_arguments_are_checked():
    tris, V = C.strip(4)
    with pytest.raises(RuntimeError):
        M.components(torch.from_numpy(tris), V)                              # host tensor
    with pytest.raises(RuntimeError):
        M.components(dev(tris.astype(np.int64)), V)
    host, m = attributed(tris, V)
    with pytest.raises(RuntimeError):
        m.select(torch.ones(3, dtype=torch.bool, device=DEV))
    with pytest.raises(RuntimeError, match="DIF_EINVAL"):
        M.edge_census(m.triangles, torch.zeros(V, dtype=torch.int32, device=DEV), V + 1)       # more components than vertices


# ---- through the map -------------------------------------------------------------------------------------------------------------------
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
    return [getattr(g, name).numpy().tobytes() for name in ("vertices", "normals", "vertex_std", "triangles", "triangle_flatten_id")]


def topology_arrays(t: M.MeshTopology):
    return {k: getattr(t, k).cpu().numpy() for k in ("vertex_component", "triangle_component", "n_vertices", "n_triangles", "n_edges", "n_boundary", "euler")}


def test_map_two_spheres(two_sphere_map):
    m = two_sphere_map
    a = m.indexed_mesh()
    V, tris = a.counts["vertices"], a.triangles.cpu().numpy()
    t = a.topology()
    want = C.topology(tris, V)
    got = topology_arrays(t)
    for name, g in got.items():
        assert np.array_equal(g, want[name]), name
    assert t.count == want["count"] and t.max_edge_use == want["max_edge_use"] and t.status == 0
    nt, closed = got["n_triangles"], (got["n_boundary"] == 0) & (got["euler"] == 2) & (got["n_triangles"] > 0)
    print("two-sphere map:", sorted(zip(nt.tolist(), got["n_boundary"].tolist(), got["euler"].tolist()), reverse=True)[:8], "components:", t.count)
    assert closed.sum() == 2 and (nt[closed] > 1000).all() and (nt[~closed] < 200).all()
    # the fragments go, the two surfaces stay
    r = a.remove_small_components(500)
    rt = r.topology()
    assert rt.count == 2 and rt.n_boundary.tolist() == [0, 0] and rt.euler.tolist() == [2, 2] and sorted(rt.n_triangles.tolist()) == sorted(nt[closed].tolist())
    W.assert_closed_surface(r.counts["vertices"], r.triangles.cpu().numpy())
    assert r.counts["components_removed"] == t.count - 2 and r.counts["triangles"] == int(nt[closed].sum())
    host = tuple(getattr(a.cpu(), name).numpy() for name in ("vertices", "normals", "vertex_std", "triangles", "triangle_flatten_id"))
    assert mesh_bytes(r) == [np.ascontiguousarray(x).tobytes() for x in (C.remove_small_components(*host, min_triangles=500)[0][k] for k in
                                                                        ("vertices", "normals", "vertex_std", "triangles", "triangle_flatten_id"))]
    one = a.remove_small_components(keep_largest=1)
    ot = one.topology()
    assert ot.count == 1 and ot.n_triangles.tolist() == [int(nt.max())] and one.counts["components_removed"] == t.count - 1
    # the keyword is the same path
    k = m.indexed_mesh(min_component_triangles=500)
    assert mesh_bytes(k) == mesh_bytes(r) and k.counts == r.counts
    # the default is what indexed_mesh() was before the keyword existed: the weld of the cache, nothing else
    tri, tid, tstd = m.mesh_cache_tensors()
    w = M.weld(tri, tstd, tid, list(m._cmap.bound_min), float(m._cmap.voxel_size), W.SPHERE_RES, m.n_xyz)
    assert mesh_bytes(a) == mesh_bytes(w) and a.counts == w.counts and list(a.counts) == list(M.COUNT_NAMES)
    assert mesh_bytes(m.indexed_mesh(min_component_triangles=0)) == mesh_bytes(w)
    # twice the same
    t2 = m.indexed_mesh().topology()
    for name, g in topology_arrays(t2).items():
        assert np.array_equal(g, got[name]), name
    assert mesh_bytes(m.indexed_mesh().remove_small_components(500)) == mesh_bytes(r)
    assert mesh_bytes(m.indexed_mesh().remove_small_components(keep_largest=1)) == mesh_bytes(one)
