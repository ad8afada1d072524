"""CPU: the numpy restatement of the surface sampler (tests/sample_ref.py) against properties that come from no code under test — the strata's
count bound, the area, exact barycentrics, points inside their triangles, the hash against published splitmix64 values — and the binding and the
PLY reader, which need no GPU."""
import ctypes

import numpy as np
import pytest
import torch

from tests import sample_ref as R
from tests import simplify_ref as S

F32 = np.float32
F64 = np.float64


@pytest.fixture(scope="module")
def sphere():
    v, tris = S.uv_sphere(0.5)
    assert tris.shape[0] == 1984
    return v, tris, R.build(v, tris)


# ---- the reference against derived properties --------------------------------------------------------------------------------------------
def test_weights_and_area(sphere):
    v, tris, b = sphere
    K, e = tris.shape[0], b["exponent"]
    assert b["counts"] == [K, 0, 0, 0, e, 0]
    assert 2 ** 31 <= int(b["w"].max()) < 2 ** 32 and int(b["prefix"][-1]) == b["total"] == sum(int(x) for x in b["w"]) < 2 ** 63
    # the float64 area of the float32 vertices, from the cross products alone; every floor loses less than one unit of 2^(e - 32)
    p = v[tris].astype(F64)
    a64 = float((0.5 * np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1)).sum())
    assert 0 <= a64 - R.area(b) < K * 2.0 ** (e - 33)
    assert abs(a64 - np.pi) < 0.02 * np.pi                                       # a sphere of radius 0.5, inscribed


@pytest.mark.parametrize("N", [1, 7, 1000, 100_000])
def test_samples_per_triangle_follow_the_weights(sphere, N):
    """Stratum j is one N-th of [0, T): the strata a triangle's interval of P meets are those it holds entirely (at most N w / T) and at most
    two that it shares, so its count differs from N w / T by less than 2 — whatever the hash does."""
    v, tris, b = sphere
    s = R.sample(v, tris, N, seed=5, b=b)
    count = np.bincount(s["triangle"], minlength=tris.shape[0])
    expect = N * b["w"].astype(F64) / float(b["total"])
    assert count.sum() == N and np.abs(count - expect).max() < 2
    assert (np.diff(s["triangle"]) >= 0).all()                                    # ascending triangle order
    lo, width = R.strata(b["total"], N)
    assert int(lo[0]) == 0 and int(lo[-1] + width[-1]) == b["total"] and int(width.max()) - int(width.min()) <= 1


def test_barycentrics_and_points(sphere):
    v, tris, b = sphere
    s = R.sample(v, tris, 100_000, seed=1, b=b)
    bary, pt = s["barycentric"], s["point"]
    assert bary.dtype == F32 and (bary >= 0).all() and ((bary[:, 0] + bary[:, 1]) + bary[:, 2] == F32(1)).all()
    assert (bary.astype(F64).sum(axis=1) == 1.0).all()                            # multiples of 2^-24: exact in any order
    assert 0.2 < float((bary[:, 0] < 1.0 / 3.0).mean()) < 0.8
    # inside the box of the triangle's vertices, widened by one ulp (of the largest |coordinate|) per term of the sum
    p = v[tris[s["triangle"]]].astype(F64)
    ulp = np.spacing(np.abs(v[tris[s["triangle"]]]).max(axis=(1, 2))).astype(F64)[:, None]
    assert (pt.astype(F64) >= p.min(axis=1) - 3 * ulp).all() and (pt.astype(F64) <= p.max(axis=1) + 3 * ulp).all()
    # and near the sphere: between the inscribed mesh's flattest chord and the radius
    r = np.linalg.norm(pt.astype(F64), axis=1)
    assert r.max() <= 0.5 + 1e-6 and r.min() > 0.5 * np.cos(np.pi / 32) ** 2 - 1e-6


def test_classes_of_a_planted_mesh():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [np.nan, 0, 0], [np.inf, 0, 0], [2.0 ** 60, 0, 0], [2, 0, 0], [2.0 ** -20, 0, 0], [0, 2.0 ** -20, 0]], F32)
    tris = np.array([[0, 1, 2], [0, 1, 9], [0, 1, 3], [0, 4, 2], [5, 1, 2], [0, 1, 6], [1, 1, 2], [0, 7, 8], [-1, 1, 2], [0, 1, 2]], np.int32)
    b = R.build(v, tris)
    assert b["counts"] == [2, 3, 3, 2, 1, R.BAD_INDEX]                            # n = 1 for the unit triangle: 1 = 0.5 * 2^1
    assert b["w"].tolist() == [2 ** 31, 0, 0, 0, 0, 0, 0, 0, 0, 2 ** 31] and b["total"] == 2 ** 32
    s = R.sample(v, tris, 1001, seed=3, b=b)
    assert sorted(set(s["triangle"].tolist())) == [0, 9] and abs(int((s["triangle"] == 0).sum()) - 500.5) < 2
    empty = R.sample(v, tris[1:7], 4)
    assert empty["build"]["total"] == 0 and empty["counts"] == [0, R.BAD_INDEX] and (empty["triangle"] == -1).all() and np.isnan(empty["point"]).all()
    assert R.sample(v, tris[:0], 3)["counts"] == [0, 0] and R.sample(v, tris, 0)["counts"] == [0, R.BAD_INDEX]


# ---- hashing -----------------------------------------------------------------------------------------------------------------------------
def _mix_int(z):
    m = 2 ** 64 - 1
    z = (z + 0x9E3779B97F4A7C15) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return z ^ (z >> 31)


def test_mix_is_splitmix64():
    # the first two outputs of splitmix64 seeded with 0 (the published test vector): mix(0) and mix(golden)
    assert int(R.mix(0)) == 0xE220A8397B1DCDAF and int(R.mix(0x9E3779B97F4A7C15)) == 0x6E789E6AA1B965F4
    z = np.array([0, 1, 2 ** 63, 2 ** 64 - 1, 0x0123456789ABCDEF], dtype=np.uint64)
    assert [int(x) for x in R.mix(z)] == [_mix_int(int(x)) for x in z]


def test_seeds(sphere):
    v, tris, b = sphere
    a0, a1, again = (R.sample(v, tris, 500, seed=s, b=b) for s in (7, 8, 7))
    assert a0["point"].tobytes() == again["point"].tobytes() and a0["triangle"].tobytes() == again["triangle"].tobytes()
    assert a0["point"].tobytes() != a1["point"].tobytes() and a0["barycentric"].tobytes() != a1["barycentric"].tobytes()
    assert (a0["barycentric"] != a1["barycentric"]).any(axis=1).mean() > 0.99
    assert R.sample(v, tris, 500, seed=-1, b=b)["point"].tobytes() == R.sample(v, tris, 500, seed=2 ** 64 - 1, b=b)["point"].tobytes()


# ---- the binding -------------------------------------------------------------------------------------------------------------------------
def test_sampler_entry_points_are_bound_and_exported():
    from di_fusion_amd import _build, _lib
    h = ctypes.CDLL(str(_build.build()))
    for name in ("dif_mesh_sampler_workspace_bytes", "dif_mesh_sampler_build", "dif_mesh_sample"):
        assert name in _lib.SIGNATURES and hasattr(h, name), name
    assert _lib.SAMPLER_COUNT == 8 and _lib.SAMPLE_COUNT == 2


# ---- PLY ---------------------------------------------------------------------------------------------------------------------------------
def _mesh(colours):
    from di_fusion_amd.system import mesh as M
    v, tris = S.uv_sphere(0.5, 6, 7)
    rng = np.random.default_rng(3)
    n = rng.normal(size=v.shape).astype(F32)
    std = rng.random(v.shape[0]).astype(F32)
    std[0] = np.array([0x7FC00123], dtype=np.uint32).view(F32)[0]                 # a NaN payload travels bit for bit
    t = torch.from_numpy
    return M.IndexedMesh(t(v), t(n), t(std), t(tris), t(np.arange(tris.shape[0], dtype=np.int64)), {},
                         t(rng.integers(0, 256, size=v.shape, dtype=np.uint8)) if colours else None, t(std.copy()) if colours else None)


@pytest.mark.parametrize("colours", [False, True])
def test_read_ply_reads_back_what_write_ply_wrote(tmp_path, colours):
    from di_fusion_amd.system import mesh as M
    m = _mesh(colours)
    m.write_ply(tmp_path / "m.ply")
    r = M.read_ply(tmp_path / "m.ply", "cpu")
    for k in ("vertices", "normals", "vertex_std", "triangles"):
        a, b = getattr(r, k), getattr(m, k)
        assert a.dtype == b.dtype and a.shape == b.shape and a.numpy().tobytes() == b.numpy().tobytes(), k
    assert r.triangle_flatten_id.dtype == torch.int64 and (r.triangle_flatten_id == -1).all() and r.triangle_flatten_id.shape == (m.triangles.shape[0],)
    if colours:
        assert r.colors.dtype == torch.uint8 and torch.equal(r.colors, m.colors) and (r.color_weight == 1).all()
    else:
        assert r.colors is None and r.color_weight is None
    r.write_ply(tmp_path / "again.ply")
    assert (tmp_path / "again.ply").read_bytes() == (tmp_path / "m.ply").read_bytes()


def _ply(header_lines, body):
    return ("\n".join(["ply"] + header_lines + ["end_header"]) + "\n").encode("ascii") + body


def test_read_ply_other_layouts_and_refusals(tmp_path):
    from di_fusion_amd.system import mesh as M
    p = tmp_path / "x.ply"
    # properties in another order and of other types, uint indices, no normals / quality / colours, an element after the faces
    vert = np.zeros((3,), dtype=[("red", "u1"), ("z", "<f8"), ("x", "<f4"), ("k", "<i4"), ("y", "<f4")])
    vert["x"], vert["y"], vert["z"] = [0, 1, 0], [0, 0, 1], [2.5, 2.5, 2.5]
    face = np.zeros((1,), dtype=[("n", "u1"), ("v", "<u4", (3,))])
    face["n"], face["v"] = 3, [[0, 1, 2]]
    head = ["format binary_little_endian 1.0", "comment x", "element vertex 3", "property uchar red", "property double z", "property float x", "property int k",
            "property float y", "element face 1", "property list uchar uint vertex_indices"]
    p.write_bytes(_ply(head + ["element edge 0", "property int a"], vert.tobytes() + face.tobytes()))
    r = M.read_ply(p, "cpu")
    assert r.vertices.tolist() == [[0, 0, 2.5], [1, 0, 2.5], [0, 1, 2.5]] and r.triangles.tolist() == [[0, 1, 2]] and r.triangles.dtype == torch.int32
    assert r.colors is None and (r.normals == 0).all() and (r.vertex_std == 0).all() and r.normals.shape == (3, 3)
    good = _ply(head, vert.tobytes() + face.tobytes())

    def refused(data, word):
        p.write_bytes(data)
        with pytest.raises(ValueError, match=word):
            M.read_ply(p, "cpu")

    refused(good.replace(b"binary_little_endian", b"ascii"), "ascii")
    refused(good.replace(b"binary_little_endian", b"binary_big_endian"), "binary_big_endian")
    refused(good[:-1], "truncated")
    refused(good[:-len(face.tobytes()) - 5], "truncated")
    refused(b"plx" + good[3:], "not a PLY")
    refused(good.replace(b"property float y\n", b""), "x, y and z")
    refused(good.replace(b"property int k", b"property list uchar int k"), "scalars")
    refused(good.replace(b"list uchar uint vertex_indices", b"list uint uint vertex_indices"), "list uint uint")
    refused(good.replace(b"element face 1", b"element edge 1"), "edge")
    quad = np.zeros((1,), dtype=[("n", "u1"), ("v", "<u4", (4,))])
    quad["n"] = 4
    refused(_ply(head, vert.tobytes() + quad.tobytes()), "face 0 has 4")
    big = face.copy()
    big["v"] = [[0, 1, 2 ** 31]]
    refused(_ply(head, vert.tobytes() + big.tobytes()), "int32")
