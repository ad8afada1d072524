"""CPU: components, selection and edge census of an indexed mesh without a GPU — the ABI on its three sides, the numpy restatement
(tests/components_ref.py) on hand-made meshes against written-out answers, and on the oracle's two-sphere scene, where it must find the two
closed surfaces and the fragments beside them."""
import ctypes
import re

import numpy as np
import pytest

from tests import components_ref as C
from tests import weld_ref as W
from tests.conftest import ROOT

F32 = np.float32


# ---- ABI -------------------------------------------------------------------------------------------------------------------------------
ENTRY_POINTS = (("dif_mesh_components_workspace_bytes", "int64_t", 2), ("dif_mesh_components", "int", 11),
                ("dif_mesh_select_workspace_bytes", "int64_t", 2), ("dif_mesh_select", "int", 17),
                ("dif_mesh_edge_census_workspace_bytes", "int64_t", 1), ("dif_mesh_edge_census", "int", 11))


def test_header_binding_and_library_agree_on_the_component_symbols():
    from di_fusion_amd import _build, _lib
    src = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "difusion.h").read_text(), flags=re.S)
    h = ctypes.CDLL(str(_build.build()))
    for name, ret, n_args in ENTRY_POINTS:
        m = re.search(r"\b" + ret + r"\s+" + name + r"\s*\(([^)]*)\)", src)
        assert m, f"{name} is not declared in difusion.h"
        assert len(m.group(1).split(",")) == n_args == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(h, name), f"{name} is not exported"
    for prefix in ("COMP", "SELECT", "EDGE", "MESH_STATUS"):
        found = re.findall(r"DIF_" + prefix + r"_(\w+)\s*=\s*(\d+)", src)
        assert found, prefix
        for name, val in found:
            assert getattr(_lib, f"{prefix}_{name}") == int(val)


def test_workspace_sizes_are_answered_on_the_host():
    from di_fusion_amd import _build
    h = ctypes.CDLL(str(_build.build()))
    for name in ("dif_mesh_components_workspace_bytes", "dif_mesh_select_workspace_bytes"):
        f = getattr(h, name)
        f.restype, f.argtypes = ctypes.c_int64, [ctypes.c_int64, ctypes.c_int64]
        assert f(0, 0) > 0
        assert f(1000, 2000) >= 2 * 4 * 1000                              # two int arrays over the vertices
        assert f(-1, 0) == -1 and f(0, -1) == -1
        assert f(2 ** 31 - 1, 0) > 0 and f(2 ** 31, 0) == -1              # V < 2^31
        assert f(0, (2 ** 31 - 1) // 3) > 0 and f(0, (2 ** 31 + 2) // 3) == -1      # 3 K < 2^31
    f = h.dif_mesh_edge_census_workspace_bytes
    f.restype, f.argtypes = ctypes.c_int64, [ctypes.c_int64]
    assert f(0) > 0
    assert f(1000) >= 8192 * 12                                            # a table of >= 6 K slots (key, uses)
    assert f(-1) == -1
    assert f(2 ** 31 // 6) > 0 and f(2 ** 31 // 6 + 1) == -1               # 6 K <= 2^31: slots are indexed with 32 bits


# ---- hand-made meshes against written-out answers --------------------------------------------------------------------------------------
def topo(tris, V):
    t = C.topology(np.asarray(tris, dtype=np.int32).reshape(-1, 3), V)
    return {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in t.items()}


def test_two_disjoint_triangles():
    t = topo([[0, 1, 2], [3, 4, 5]], 6)
    assert t["count"] == 2 and t["status"] == 0
    assert t["vertex_component"] == [0, 0, 0, 1, 1, 1] and t["triangle_component"] == [0, 1]
    assert t["n_vertices"] == [3, 3] and t["n_triangles"] == [1, 1]
    assert t["n_edges"] == [3, 3] and t["n_boundary"] == [3, 3] and t["euler"] == [1, 1] and t["max_edge_use"] == 1


def test_numbering_follows_the_lowest_vertex_not_the_triangle_order():
    t = topo([[3, 4, 5], [0, 1, 2]], 6)
    assert t["vertex_component"] == [0, 0, 0, 1, 1, 1] and t["triangle_component"] == [1, 0]


def test_two_triangles_sharing_one_vertex_are_one_component():
    t = topo([[0, 1, 2], [2, 3, 4]], 5)
    assert t["count"] == 1 and t["vertex_component"] == [0] * 5 and t["triangle_component"] == [0, 0]
    assert t["n_vertices"] == [5] and t["n_triangles"] == [2] and t["n_edges"] == [6] and t["n_boundary"] == [6] and t["euler"] == [1]


def test_vertices_without_a_triangle_are_components_of_their_own():
    t = topo(np.zeros((0, 3)), 5)
    assert t["count"] == 5 and t["vertex_component"] == [0, 1, 2, 3, 4] and t["triangle_component"] == []
    assert t["n_vertices"] == [1] * 5 and t["n_triangles"] == [0] * 5 and t["n_edges"] == [0] * 5 and t["euler"] == [1] * 5
    assert t["max_edge_use"] == 0
    assert topo(np.zeros((0, 3)), 0)["count"] == 0


def test_a_repeated_index_triangle():
    t = topo([[0, 0, 1], [2, 2, 2]], 4)                                     # the first is one edge, the second joins nothing
    assert t["count"] == 3 and t["vertex_component"] == [0, 0, 1, 2] and t["triangle_component"] == [0, 1]
    assert t["n_vertices"] == [2, 1, 1] and t["n_triangles"] == [1, 1, 0]
    assert t["n_edges"] == [1, 0, 0] and t["n_boundary"] == [0, 0, 0] and t["max_edge_use"] == 2       # (0,1) is named by two sides


def test_a_tetrahedron_is_closed():
    t = topo(C.TETRAHEDRON, 4)
    assert t["count"] == 1 and t["n_vertices"] == [4] and t["n_triangles"] == [4] and t["n_edges"] == [6]
    assert t["n_boundary"] == [0] and t["euler"] == [2] and t["max_edge_use"] == 2


def test_a_tetrahedron_minus_a_face_has_a_boundary():
    t = topo(C.TETRAHEDRON[:3], 4)
    assert t["count"] == 1 and t["n_triangles"] == [3] and t["n_edges"] == [6] and t["n_boundary"] == [3] and t["euler"] == [1]


def test_an_index_out_of_range_joins_nothing():
    t = topo([[0, 1, 2], [2, 3, 4], [5, 6, 7], [-1, 5, 6]], 4)
    assert t["status"] == C.BAD_INDEX and t["triangle_component"] == [0, -1, -1, -1]
    assert t["count"] == 2 and t["vertex_component"] == [0, 0, 0, 1] and t["n_triangles"] == [1, 0] and t["n_edges"] == [3, 0]


def test_a_triple_used_edge():
    t = topo([[0, 1, 2], [1, 0, 3], [0, 1, 4]], 5)
    assert t["max_edge_use"] == 3 and t["n_edges"] == [7] and t["n_boundary"] == [6] and t["euler"] == [5 - 7 + 3]


def test_select_written_out():
    v = np.arange(18, dtype=F32).reshape(6, 3)
    n, s = -v, np.arange(6, dtype=F32) + F32(0.5)
    tris = np.array([[0, 1, 2], [5, 3, 1], [2, 1, 0]], dtype=np.int32)
    ids = np.array([7, 8, 9], dtype=np.int64)
    o = C.select(v, n, s, tris, ids, [False, True, False])
    assert o["counts"] == [3, 1, 0] and o["triangles"].tolist() == [[2, 1, 0]] and o["triangle_flatten_id"].tolist() == [8]
    assert np.array_equal(o["vertices"], v[[1, 3, 5]]) and np.array_equal(o["normals"], n[[1, 3, 5]]) and o["vertex_std"].tolist() == [1.5, 3.5, 5.5]
    o = C.select(v, n, s, tris, ids, [True, True, True])
    assert o["counts"] == [5, 3, 0] and o["triangles"].tolist() == [[0, 1, 2], [4, 3, 1], [2, 1, 0]]                # vertex 4 goes: no triangle uses it
    assert C.select(v, n, s, tris, ids, [False] * 3)["counts"] == [0, 0, 0]
    o, removed = C.remove_small_components(v, n, s, np.array([[0, 1, 2], [1, 2, 3], [4, 5, 4]], dtype=np.int32), ids, keep_largest=1)
    assert removed == 1 and o["counts"] == [4, 2, 0]
    o, removed = C.remove_small_components(v, n, s, np.array([[0, 1, 2], [3, 4, 5]], dtype=np.int32), ids[:2], keep_largest=1)
    assert removed == 1 and o["triangles"].tolist() == [[0, 1, 2]] and o["triangle_flatten_id"].tolist() == [7]     # the tie goes to the lower id


def test_the_test_inputs_are_what_they_say():
    t, V = C.strip(65)
    assert C.topology(t, V)["n_edges"].tolist() == [2 * 65 + 1]
    for hub_high in (False, True):
        t, V = C.fan(10, hub_high)
        o = C.topology(t, V)
        assert o["count"] == 1 and o["n_edges"].tolist() == [21] and np.bincount(t.reshape(-1)).max() == 10 and (t[:, 0] == (V - 1 if hub_high else 0)).all()
    t, V = C.disjoint(1366)
    assert V == 4098 and C.components(t, V)["count"] == 1366
    t, V = C.disjoint(1366, 700)
    assert V == 4798 and C.components(t, V)["count"] == 2066
    sizes = C.components(*C.random_mesh(5000, 3000, 0))["n_triangles"]
    assert sizes.max() > 2000 and (sizes == 1).sum() > 3 and (sizes == 0).sum() > 500       # one giant, a few single triangles, unused vertices
    sizes = C.components(*C.random_mesh(5000, 850, 0))["n_triangles"]
    assert len(np.unique(sizes)) > 8                           # K = V / 6, where a triangle meets one other on average: components of every order


# ---- the oracle's two spheres ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def two_sphere_mesh(oracle_net):
    from oracle import difusion_oracle as O
    b = W.SPHERE_BOUND
    om = O.OracleMap(oracle_net, (-b, -b, -b), (b, b, b), W.SPHERE_VOXEL)
    om.integrate_keyframe(*C.two_sphere_cloud())
    tri, tid, tstd = om.extract_mesh(W.SPHERE_RES, int(4e6), 2000.0, fast=True)
    o = W.weld(tri, tstd, tid, om.bound_min, om.voxel_size, W.SPHERE_RES)
    assert o["counts"][3] == 0 and o["counts"][4] == 0
    return o, C.topology(o["triangles"], int(o["counts"][0]))


def test_two_spheres_census_equals_the_union_find_of_the_weld_tests(two_sphere_mesh):
    o, t = two_sphere_mesh
    w = W.topology(int(o["counts"][0]), o["triangles"])
    with_tris = t["n_triangles"] > 0
    mine = sorted(zip(*(t[k][with_tris].tolist() for k in ("n_vertices", "n_edges", "n_triangles", "n_boundary", "euler"))))
    theirs = sorted((c["V"], c["E"], c["F"], c["boundary"], c["euler"]) for c in w["comps"])
    print("two spheres:", sorted(mine, key=lambda c: -c[2]))
    assert mine == theirs
    assert t["max_edge_use"] == w["max_edge_use"] and int(t["n_boundary"].sum()) == w["n_boundary"] and t["status"] == 0
    assert int(t["n_triangles"].sum()) == o["triangles"].shape[0] and int(t["n_vertices"].sum()) == o["counts"][0]


def test_two_spheres_are_two_closed_surfaces_and_fragments(two_sphere_mesh):
    o, t = two_sphere_mesh
    closed = (t["n_boundary"] == 0) & (t["euler"] == 2) & (t["n_triangles"] > 0)
    assert closed.sum() == 2 and (t["n_triangles"][closed] > 1000).all()
    assert (t["n_triangles"][~closed] < 200).all()
    a = (o["vertices"], o["normals"], o["vertex_std"], o["triangles"], o["triangle_flatten_id"])
    kept, removed = C.remove_small_components(*a, min_triangles=500)
    k = C.topology(kept["triangles"], kept["counts"][0])
    assert k["count"] == 2 and removed == t["count"] - 2
    assert sorted(k["n_triangles"].tolist()) == sorted(t["n_triangles"][closed].tolist()) and k["n_boundary"].tolist() == [0, 0] and k["euler"].tolist() == [2, 2]
    one, removed = C.remove_small_components(*a, keep_largest=1)
    k1 = C.topology(one["triangles"], one["counts"][0])
    assert k1["count"] == 1 and removed == t["count"] - 1 and k1["n_triangles"].tolist() == [int(t["n_triangles"].max())]
    # normals and positions of what stays are copies
    big = int(np.argmax(t["n_triangles"]))
    assert np.array_equal(one["vertices"].view(np.uint32), o["vertices"][t["vertex_component"] == big].view(np.uint32))
