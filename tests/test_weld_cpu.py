"""CPU: the indexed-mesh weld without a GPU — its ABI on the three sides, the PLY writer, and the numpy restatement (tests/weld_ref.py) on
hand-made soups and on the oracle's sphere soup, where it must produce the closed surface an exact-position weld does not."""
import ctypes
import re

import numpy as np
import pytest

from tests import weld_ref as W
from tests.conftest import ROOT

F32 = np.float32
BM, VS, R = (-0.8, -0.8, -0.8), 0.1, 4
CELL = VS / R


def lattice(*p):
    """lattice coordinates -> float32 world position"""
    return (np.asarray(BM, dtype=np.float64) + np.asarray(p, dtype=np.float64) * CELL).astype(F32)


def read_ply(path):
    """Reader for what `IndexedMesh.write_ply` writes (binary little-endian, float vertex properties, uchar/int face lists)."""
    data = open(path, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    nv = nf = 0
    props = []
    element = None
    for ln in lines:
        w = ln.split()
        if w[:1] == ["element"]:
            element = w[1]
            if element == "vertex":
                nv = int(w[2])
            elif element == "face":
                nf = int(w[2])
        elif w[:1] == ["property"] and element == "vertex":
            assert w[1] == "float"
            props.append(w[2])
        elif w[:1] == ["property"] and element == "face":
            assert w[1:] == ["list", "uchar", "int", "vertex_indices"]
    vert = np.frombuffer(data, dtype=[(n, "<f4") for n in props], count=nv, offset=end)
    face = np.frombuffer(data, dtype=[("n", "u1"), ("v", "<i4", (3,))], count=nf, offset=end + vert.nbytes)
    assert end + vert.nbytes + face.nbytes == len(data)
    return vert, face


# ---- ABI -------------------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree_on_the_weld_symbols():
    from di_fusion_amd import _build, _lib
    src = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "difusion.h").read_text(), flags=re.S)
    h = ctypes.CDLL(str(_build.build()))
    for name, ret, n_args in (("dif_mesh_weld_workspace_bytes", "int64_t", 1), ("dif_mesh_weld", "int", 14)):
        m = re.search(r"\b" + ret + r"\s+" + name + r"\s*\(([^)]*)\)", src)
        assert m, f"{name} is not declared in difusion.h"
        assert len(m.group(1).split(",")) == n_args == len(_lib.SIGNATURES[name][1])
        assert hasattr(h, name), f"{name} is not exported"
    fields = re.search(r"typedef struct dif_weld_args \{(.*?)\} dif_weld_args_t;", src, flags=re.S).group(1)
    assert re.findall(r"(\w+)(?:\[\d+\])?;", fields) == [f[0] for f in _lib.DifWeldArgs._fields_]
    assert ctypes.sizeof(_lib.DifWeldArgs) == 32
    for name, val in re.findall(r"DIF_WELD_(\w+)\s*=\s*(\d+)", src):
        assert getattr(_lib, f"WELD_{name}") == int(val)
    # sizes the host can answer without a GPU
    h.dif_mesh_weld_workspace_bytes.restype = ctypes.c_int64
    h.dif_mesh_weld_workspace_bytes.argtypes = [ctypes.c_int64]
    assert h.dif_mesh_weld_workspace_bytes(0) > 0
    assert h.dif_mesh_weld_workspace_bytes(1000) >= 8192 * 16 + 3000 * 32          # table of >= 6 T slots (key, minimum, vertex) + per-corner arrays
    assert h.dif_mesh_weld_workspace_bytes(-1) == -1
    assert h.dif_mesh_weld_workspace_bytes((2 ** 31 + 2) // 3) == -1               # 3 T >= 2^31


# ---- PLY -------------------------------------------------------------------------------------------------------------------------------
def test_ply_round_trips_bit_for_bit(tmp_path):
    import torch
    from di_fusion_amd.system.mesh import IndexedMesh
    rng = np.random.default_rng(3)
    v = rng.standard_normal((7, 3)).astype(F32)
    v[2, 1] = np.nextafter(F32(1), F32(2))
    v[3, 0] = F32(-0.0)
    n = rng.standard_normal((7, 3)).astype(F32)
    s = rng.random(7).astype(F32)
    t = np.array([[0, 1, 2], [2, 1, 3], [6, 5, 4], [0, 6, 3]], dtype=np.int32)
    ids = np.array([5, 5, 9, 1], dtype=np.int64)
    m = IndexedMesh(*(torch.from_numpy(a) for a in (v, n, s, t, ids)), dict(vertices=7, triangles=4, dropped=0, unkeyed=0, status=0))
    m.write_ply(tmp_path / "m.ply")
    vert, face = read_ply(tmp_path / "m.ply")
    assert vert.dtype.names == ("x", "y", "z", "nx", "ny", "nz", "quality")
    got = np.stack([vert[k] for k in vert.dtype.names], axis=1)
    want = np.concatenate([v, n, s[:, None]], axis=1)
    assert got.view(np.uint32).tolist() == want.view(np.uint32).tolist()
    assert (face["n"] == 3).all() and np.array_equal(face["v"], t)
    # an empty mesh is a valid file
    e = IndexedMesh(*(torch.from_numpy(a[:0]) for a in (v, n, s, t, ids)), {})
    e.write_ply(tmp_path / "e.ply")
    vert, face = read_ply(tmp_path / "e.ply")
    assert vert.shape == (0,) and face.shape == (0,)


# ---- hand-made soups (shared with tests/test_gpu_weld.py) ------------------------------------------------------------------------------
def soup_reversed_edge():
    """Two triangles that share an edge, given in opposite directions, whose two end points differ in the last bit between the copies."""
    a, b = lattice(3.3, 2, 5), lattice(4, 2.6, 5)
    c, d = lattice(3, 2.5, 5), lattice(4.5, 2, 5)
    a2, b2 = a.copy(), b.copy()
    a2[0] = np.nextafter(a2[0], F32(np.inf))
    b2[1] = np.nextafter(b2[1], F32(-np.inf))
    b2[2] = np.nextafter(b2[2], F32(np.inf))
    tri = np.array([[a, b, c], [b2, a2, d]], dtype=F32)
    return tri, np.arange(6, dtype=F32).reshape(2, 3), np.array([7, 8], dtype=np.int64)


def soup_corner_from_three_edges():
    """A vertex exactly on a lattice corner, reached as the end of an x, a y and a z edge (the early-outs of the interpolation), a few ulps apart."""
    c = lattice(6, 7, 8)
    c1, c2 = c.copy(), c.copy()
    c1[0] = np.nextafter(c1[0], F32(np.inf))
    c2[2] = np.nextafter(np.nextafter(c2[2], F32(-np.inf)), F32(-np.inf))
    tri = np.array([[c, lattice(6.5, 7, 8), lattice(6, 7.5, 8)], [c1, lattice(6, 7.5, 8), lattice(6, 7, 8.5)], [c2, lattice(6, 7, 8.5), lattice(6.5, 7, 8)]],
                   dtype=F32)
    return tri, np.linspace(0, 1, 9, dtype=F32).reshape(3, 3), np.array([1, 2, 3], dtype=np.int64)


def soup_off_lattice():
    """One corner in the middle of a cell face (two axes off the lattice), twice: unkeyed, so the two copies are NOT welded."""
    off = lattice(2.5, 3.5, 4)
    tri = np.array([[off, lattice(3, 3.5, 4), lattice(2, 3.25, 4)], [off, lattice(2, 3.25, 4), lattice(3, 3.5, 4)]], dtype=F32)
    return tri, np.ones((2, 3), dtype=F32), np.array([4, 4], dtype=np.int64)


def soup_collapsed():
    """The middle triangle has two corners on one lattice edge: it collapses; its neighbours stay."""
    e, e2 = lattice(5.25, 5, 5), lattice(5.75, 5, 5)
    tri = np.array([[lattice(5, 5, 5), e, lattice(5, 5.5, 5)], [e, e2, lattice(5, 5.5, 5)], [e2, lattice(6, 5.5, 5), lattice(5, 5.5, 5)]], dtype=F32)
    return tri, np.full((3, 3), 0.5, dtype=F32), np.array([10, 11, 12], dtype=np.int64)


def soup_empty():
    return np.zeros((0, 3, 3), dtype=F32), np.zeros((0, 3), dtype=F32), np.zeros((0,), dtype=np.int64)


HAND_MADE = dict(reversed_edge=soup_reversed_edge, corner_from_three_edges=soup_corner_from_three_edges, off_lattice=soup_off_lattice,
                 collapsed=soup_collapsed, empty=soup_empty)


def test_restatement_welds_an_edge_given_in_both_directions():
    tri, std, ids = soup_reversed_edge()
    assert not np.array_equal(tri[0, 0], tri[1, 1]) and not np.array_equal(tri[0, 1], tri[1, 0])
    o = W.weld(tri, std, ids, BM, VS, R)
    assert o["counts"].tolist() == [4, 2, 0, 0, 0]
    assert o["triangles"].tolist() == [[0, 1, 2], [1, 0, 3]]
    assert np.array_equal(o["vertices"], np.array([tri[0, 0], tri[0, 1], tri[0, 2], tri[1, 2]]))       # the lowest soup corner's copy, not an average
    assert o["vertex_std"].tolist() == [0.0, 1.0, 2.0, 5.0]
    assert o["triangle_flatten_id"].tolist() == [7, 8]
    assert np.allclose(np.abs(o["normals"]), [[0, 0, 1]] * 4, atol=1e-5) and (o["normals"][:, 2] < 0).sum() in (0, 4)
    assert W.weld_exact(tri)[0] == 6                                                                   # by position: nothing shared


def test_restatement_welds_a_lattice_corner_reached_from_three_edges():
    tri, std, ids = soup_corner_from_three_edges()
    o = W.weld(tri, std, ids, BM, VS, R)
    assert o["counts"].tolist() == [4, 3, 0, 0, 0]
    assert o["triangles"].tolist() == [[0, 1, 2], [0, 2, 3], [0, 3, 1]]
    key, keyed = W.corner_keys(tri.reshape(-1, 3), BM, VS, R)
    assert keyed.all() and (key[[0, 3, 6]] & 3).tolist() == [3, 3, 3] and len(set(key[[0, 3, 6]].tolist())) == 1
    assert (key[[1, 2, 5]] & 3).tolist() == [0, 1, 2]
    nrm = o["normals"]
    assert np.allclose(np.linalg.norm(nrm, axis=1), 1.0, atol=1e-6)
    assert np.allclose(nrm[0], np.ones(3) / np.sqrt(3), atol=1e-5) or np.allclose(nrm[0], -np.ones(3) / np.sqrt(3), atol=1e-5)


def test_restatement_leaves_an_off_lattice_corner_alone():
    tri, std, ids = soup_off_lattice()
    o = W.weld(tri, std, ids, BM, VS, R)
    assert o["counts"].tolist() == [4, 2, 0, 2, 0]
    assert o["triangles"].tolist() == [[0, 1, 2], [3, 2, 1]]
    assert np.array_equal(o["vertices"][0], o["vertices"][3])
    # not finite, or outside the 20 bits of the key: unkeyed as well
    bad = np.array([[[np.nan, 0, 0], [np.inf, 0, 0], lattice(2.0 ** 20 + 64, 1, 1)]], dtype=F32)
    assert W.weld(bad, std[:1], ids[:1], BM, VS, R)["counts"].tolist() == [3, 1, 0, 3, 0]
    assert W.weld(np.array([[lattice(-1, 1, 1), lattice(0, 1, 1), lattice(2.0 ** 20 - 64, 1, 1)]]), std[:1], ids[:1], BM, VS, R)["counts"][3] == 1


def test_restatement_drops_a_collapsed_triangle():
    tri, std, ids = soup_collapsed()
    o = W.weld(tri, std, ids, BM, VS, R)
    assert o["counts"].tolist() == [4, 2, 1, 0, 0]
    assert o["triangles"].tolist() == [[0, 1, 2], [1, 3, 2]]
    assert o["triangle_flatten_id"].tolist() == [10, 12]


def test_restatement_of_nothing():
    o = W.weld(*soup_empty(), BM, VS, R)
    assert o["counts"].tolist() == [0, 0, 0, 0, 0]
    assert o["vertices"].shape == (0, 3) and o["normals"].shape == (0, 3) and o["triangles"].shape == (0, 3) and o["triangles"].dtype == np.int32


def test_restatement_does_not_depend_on_which_copy_comes_first():
    tri, std, ids = W.sheet_soup(63)
    a = W.weld(tri, std, ids, BM, VS, R)
    p = np.random.default_rng(1).permutation(63)
    b = W.weld(tri[p], std[p], ids[p], BM, VS, R)
    assert a["counts"].tolist() == b["counts"].tolist()
    key = W.corner_keys(tri.reshape(-1, 3), BM, VS, R)[0]
    counts = np.unique(key, return_counts=True)[1]
    assert counts.min() == 1 and counts.max() == 6


# ---- the oracle's sphere ---------------------------------------------------------------------------------------------------------------
def test_restatement_closes_the_oracle_sphere_where_exact_positions_do_not(oracle_net):
    from oracle import difusion_oracle as O
    b = W.SPHERE_BOUND
    om = O.OracleMap(oracle_net, (-b, -b, -b), (b, b, b), W.SPHERE_VOXEL)
    xyz, nrm = W.sphere_cloud()
    om.integrate_keyframe(xyz, nrm)
    tri, tid, tstd = om.extract_mesh(W.SPHERE_RES, int(4e6), 2000.0, fast=True)
    assert tri.shape[0] > 5000
    o = W.weld(tri, tstd, tid, om.bound_min, om.voxel_size, W.SPHERE_RES)
    V, kept, dropped, unkeyed, status = o["counts"].tolist()
    assert unkeyed == 0 and status == 0 and kept + dropped == tri.shape[0] and dropped < 0.01 * kept
    t = W.assert_closed_surface(V, o["triangles"])
    assert t["n_used_vertices"] == V
    big = t["comps"][0]
    assert big["V"] > 0.9 * V
    # unit normals everywhere (every vertex has a triangle)
    nrm_len = np.linalg.norm(o["normals"].astype(np.float64), axis=1)
    assert np.abs(nrm_len - 1.0).max() < 1e-6
    # what the key is for: the same soup welded by bit-identical position stays torn
    Ve, te = W.weld_exact(tri)
    assert W.topology(Ve, te)["n_boundary"] > 1000
