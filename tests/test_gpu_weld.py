"""GPU: `dif_mesh_weld` against its numpy restatement (tests/weld_ref.py) — indices, positions, std, ids and counts bit for bit (integer logic
and copies), normals to 2^-22 — on hand-made soups, scan boundaries, a full table, one giant class and a shuffled soup; then through
`DenseIndexedMap.indexed_mesh()` on the sphere cloud, where the output must be the closed surface tests/test_weld_cpu.py shows on the oracle."""
import numpy as np
import pytest
import torch

from di_fusion_amd import synthetic as syn
from di_fusion_amd.system import mesh as M
from di_fusion_amd.system.map import DenseIndexedMap
from tests import weld_ref as W
from tests.test_weld_cpu import BM, HAND_MADE, R, VS, lattice, read_ply

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F32 = np.float32
# the normal sums are exact integers on both sides; what can differ is the device's double sqrt / divide in the last bit, then one float32 rounding of
# a value <= 1 (2^-24): four times that
NORMAL_TOL = 2.0 ** -22


def gpu_weld(tri, std, ids, bound_min=BM, voxel_size=VS, r=R, n_xyz=None):
    return M.weld(torch.from_numpy(tri).to(DEV), torch.from_numpy(std).to(DEV), torch.from_numpy(ids).to(DEV), bound_min, voxel_size, r, n_xyz)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_same(got: M.IndexedMesh, want: dict, what=""):
    """returns the largest normal difference"""
    g = got.cpu()
    assert [got.counts[k] for k in M.COUNT_NAMES] == want["counts"].tolist(), what
    assert g.triangles.dtype == torch.int32 and g.triangle_flatten_id.dtype == torch.int64
    assert np.array_equal(g.triangles.numpy(), want["triangles"]), what
    assert np.array_equal(g.triangle_flatten_id.numpy(), want["triangle_flatten_id"]), what
    assert np.array_equal(bits(g.vertices.numpy()), bits(want["vertices"])), what
    assert np.array_equal(bits(g.vertex_std.numpy()), bits(want["vertex_std"])), what
    assert g.normals.shape == want["normals"].shape
    d = np.abs(g.normals.numpy().astype(np.float64) - want["normals"].astype(np.float64))
    worst = float(d.max()) if d.size else 0.0
    print(f"{what}: counts {want['counts'].tolist()}, max normal difference {worst:.3e}, bit-identical normals: "
          f"{np.array_equal(bits(g.normals.numpy()), bits(want['normals']))}")
    assert worst <= NORMAL_TOL, (what, worst)
    return worst


@pytest.mark.parametrize("name", sorted(HAND_MADE))
def test_hand_made_soups(name):
    tri, std, ids = HAND_MADE[name]()
    assert_same(gpu_weld(tri, std, ids), W.weld(tri, std, ids, BM, VS, R), name)


@pytest.mark.parametrize("T", [1, 63, 64, 65, 4096, 4097])
def test_sheet_across_the_scan_boundaries(T):
    """3 T corners / T triangles on either side of one wave, one workgroup chunk and the single-workgroup scan's limit (4,096 elements)."""
    tri, std, ids = W.sheet_soup(T)
    want = W.weld(tri, std, ids, BM, VS, R)
    assert want["counts"][0] < 3 * T or T == 1
    assert_same(gpu_weld(tri, std, ids), want, f"sheet T={T}")


def test_all_corners_distinct_fills_the_table():
    """No two corners share a lattice edge: 3 T classes, the most the table ever holds."""
    T = 1500
    k = np.arange(3 * T)
    p = np.stack([k % 17 + 0.5, (k // 17) % 19, k // (17 * 19)], axis=1).astype(np.float64)       # one point per x edge
    p += np.random.default_rng(2).uniform(-0.2, 0.2, size=(3 * T, 1)) * np.array([1.0, 0, 0])
    tri = (np.asarray(BM, dtype=np.float64) + p * (VS / R)).astype(F32).reshape(T, 3, 3)
    std = np.random.default_rng(3).random((T, 3)).astype(F32)
    ids = np.arange(T, dtype=np.int64)
    want = W.weld(tri, std, ids, BM, VS, R)
    assert want["counts"].tolist() == [3 * T, T, 0, 0, 0]
    assert_same(gpu_weld(tri, std, ids), want, "distinct")


def test_all_corners_one_point():
    """One class under the most contention there can be; every triangle collapses, the one vertex has no normal."""
    T = 4097
    tri = np.broadcast_to(lattice(3.5, 4, 5), (T, 3, 3)).copy()
    std = np.arange(3 * T, dtype=F32).reshape(T, 3)
    ids = np.arange(T, dtype=np.int64)
    want = W.weld(tri, std, ids, BM, VS, R)
    assert want["counts"].tolist() == [1, 0, T, 0, 0] and want["normals"].tolist() == [[0.0, 0.0, 0.0]]
    assert_same(gpu_weld(tri, std, ids), want, "one point")


def test_shuffled_soup_follows_its_own_order():
    tri, std, ids = W.sheet_soup(4097)
    p = np.random.default_rng(5).permutation(4097)
    tri, std, ids = tri[p].copy(), std[p].copy(), ids[p].copy()
    assert_same(gpu_weld(tri, std, ids), W.weld(tri, std, ids, BM, VS, R), "shuffled")


def test_arguments_are_checked():
    tri, std, ids = W.sheet_soup(4)
    with pytest.raises(RuntimeError, match="DIF_EINVAL"):
        gpu_weld(tri, std, ids, n_xyz=[16, (1 << 18), 16])                 # 2^18 * 4 + 1 >= 2^20
    gpu_weld(tri, std, ids, n_xyz=[16, (1 << 18) - 1, 16])
    with pytest.raises(RuntimeError):
        M.weld(torch.from_numpy(tri), torch.from_numpy(std), torch.from_numpy(ids), BM, VS, R)      # host tensors


# ---- through the map -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sphere_map(gpu_model):
    b = W.SPHERE_BOUND
    cfg = syn.MapConfig((-b, -b, -b), (b, b, b), W.SPHERE_VOXEL)
    m = DenseIndexedMap(gpu_model, cfg.namespace(), 29, DEV, initial_capacity=1024)
    xyz, nrm = W.sphere_cloud()
    xyz, nrm = torch.from_numpy(xyz).to(DEV), torch.from_numpy(nrm).to(DEV)
    assert m.indexed_mesh() is None
    m.integrate_keyframe(xyz, nrm)
    m.extract_mesh_arrays(W.SPHERE_RES, int(4e6), fast=True, max_std=2000.0, to_host=False)
    return m, xyz, nrm


def restate_cache(m, r):
    tri, tid, tstd = (t.cpu().numpy() for t in m.mesh_cache_tensors())
    return W.weld(tri, tstd, tid, m.bound_min.cpu().numpy(), F32(m.voxel_size), r), tri.shape[0]


def test_map_indexed_mesh(sphere_map, tmp_path):
    m, xyz, nrm = sphere_map
    a = m.indexed_mesh()
    want, T = restate_cache(m, W.SPHERE_RES)
    assert T > 5000
    assert_same(a, want, "sphere map")
    b = m.indexed_mesh().cpu()
    ac = a.cpu()
    for name in ("vertices", "normals", "vertex_std", "triangles", "triangle_flatten_id"):
        assert np.array_equal(getattr(ac, name).numpy().view(np.uint8), getattr(b, name).numpy().view(np.uint8)), name
    assert a.counts == b.counts and a.counts["unkeyed"] == 0 and a.counts["status"] == 0
    V = a.counts["vertices"]
    t = W.assert_closed_surface(V, ac.triangles.numpy())
    print("sphere map topology:", {k: v for k, v in t.items() if k != "boundary_comp_sizes"})
    assert np.abs(np.linalg.norm(ac.normals.numpy().astype(np.float64), axis=1) - 1.0).max() < 1e-6
    # PLY
    a.write_ply(tmp_path / "sphere.ply")
    vert, face = read_ply(tmp_path / "sphere.ply")
    got = np.stack([vert[k] for k in vert.dtype.names], axis=1)
    ref = np.concatenate([ac.vertices.numpy(), ac.normals.numpy(), ac.vertex_std.numpy()[:, None]], axis=1)
    assert np.array_equal(bits(got), bits(ref)) and np.array_equal(face["v"], ac.triangles.numpy()) and (face["n"] == 3).all()


def test_map_welds_again_after_another_frame_and_counts_another_lattice(sphere_map):
    m, xyz, nrm = sphere_map
    m.integrate_keyframe(xyz[:60000].contiguous(), nrm[:60000].contiguous())
    m.extract_mesh_arrays(W.SPHERE_RES, int(4e6), fast=True, max_std=2000.0, to_host=False)
    a = m.indexed_mesh()
    want, T = restate_cache(m, W.SPHERE_RES)
    assert_same(a, want, "sphere map, second extract")
    assert a.counts["unkeyed"] == 0
    assert a.counts["vertices"] < T and a.counts["triangles"] > 0.99 * T              # (a soup has 3 T)
    # the same cache (resolution 4) welded as if it were resolution 3: corners off that lattice are reported, not welded to something else
    c = m.indexed_mesh(voxel_resolution=3)
    want3, _ = restate_cache(m, 3)
    assert_same(c, want3, "sphere map, wrong resolution")
    assert c.counts["unkeyed"] > 0.5 * 3 * T
    assert c.counts["vertices"] >= c.counts["unkeyed"]
