"""GPU: `dif_mesh_sampler_build` / `dif_mesh_sample` against their numpy restatement (tests/sample_ref.py), byte for byte — every output array,
every count, T — across the wave, block and multi-block edges of the 64-bit scan, on a planted mesh with every class of triangle, on an analytic
sphere, on meshes without area; repeats, seeds, one sampler for several draws; `interpolate` on the samples; `IndexedMesh.compare` against
sample_ref + closest_ref; through `DenseIndexedMap.indexed_mesh()` on the two-sphere scene; refusals."""
import ctypes

import numpy as np
import pytest
import torch

from di_fusion_amd import _lib, synthetic as syn
from di_fusion_amd.system import mesh as M
from di_fusion_amd.system.map import DenseIndexedMap
from tests import closest_ref as C
from tests import closest_slack as K
from tests import components_ref as CR
from tests import sample_ref as R
from tests import simplify_ref as S
from tests import weld_ref as W

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F32 = np.float32
OUT_NAMES = ("point", "triangle", "barycentric")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def out_bytes(s: M.MeshSamples):
    g = s.cpu()
    return [getattr(g, k).numpy().tobytes() for k in OUT_NAMES]


def assert_build(smp: M.MeshSampler, b: dict, what):
    assert [smp.counts[k] for k in R.BUILD_NAMES] == b["counts"], (what, smp.counts, b["counts"])
    assert smp.total == b["total"] and smp.area == R.area(b), (what, smp.total, b["total"])


def assert_same(got: M.MeshSamples, want: dict, what):
    assert [got.counts[k] for k in R.SAMPLE_NAMES] == want["counts"], (what, got.counts, want["counts"])
    g = got.cpu()
    for k in OUT_NAMES:
        a, b = getattr(g, k).numpy(), want[k]
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == np.ascontiguousarray(b).tobytes(), (what, k)


def mesh_of(v, tris):
    V, Kt = v.shape[0], tris.shape[0]
    return M.IndexedMesh(dev(v), dev(np.zeros((V, 3), F32)), dev(np.zeros((V,), F32)), dev(tris), dev(np.full((Kt,), -1, np.int64)), {})


# ---- sizes -----------------------------------------------------------------------------------------------------------------------------
def soup_of(Kt):
    if Kt == 0:
        return S.tetrahedron()[0], np.zeros((0, 3), np.int32)
    V = max(8, min(Kt, 5000))
    return S.soup(V, Kt, min(V // 2, 600), seed=Kt)


# 300,001: the scan's workgroups walk more than one chunk of 256 (past 1024 x 256 triangles)
@pytest.mark.parametrize("Kt", [0, 1, 63, 64, 65, 255, 256, 257, 4097, 70_001, 300_001])
def test_sizes(Kt):
    v, tris = soup_of(Kt)
    b = R.build(v, tris)
    smp = M.sampler(dev(v), dev(tris))
    assert_build(smp, b, f"K = {Kt}")
    assert Kt < 63 or (b["counts"][0] > 0 and b["total"] >= 2 ** 31)
    for N in (0, 1, 2, 255, 257, 200_000):                                      # N < K and N > K; one sampler for all of them
        assert_same(smp.sample(N, seed=N + 1), R.sample(v, tris, N, seed=N + 1, b=b), f"K = {Kt}, N = {N}")
    print(f"K = {Kt}: {smp.counts}, T = {smp.total}")


# ---- a planted mesh --------------------------------------------------------------------------------------------------------------------
def planted():
    big = [[0, 0, 0], [4, 0, 0], [0, 4, 0]]                                      # n = 16
    v = np.array(big + [[np.nan, 0, 0], [np.inf, 1, 0], [2.0 ** 60, 0, 1], [1, 1, 1], [3, 3, 3], [2, 2, 2],
                        [0, 0, 5], [2.0 ** -18, 0, 5], [0, 2.0 ** -18, 5],        # n = 2^-36 = 16 * 2^-40: weightless
                        [0, 0, 6], [0.5, 0, 6], [0, 0.25, 6]], F32)               # a small one with a weight
    tris = np.array([[0, 1, 2], [0, 1, 15], [0, 1, 3], [0, 4, 2], [5, 1, 2], [6, 7, 8], [1, 1, 2], [9, 10, 11], [12, 13, 14], [2, 0, 1]], np.int32)
    return v, tris


def test_planted_mesh():
    v, tris = planted()
    b = R.build(v, tris)
    assert b["counts"] == [3, 3, 3, 1, 5, R.BAD_INDEX]                            # 16 = 0.5 * 2^5
    assert b["w"].tolist() == [2 ** 31, 0, 0, 0, 0, 0, 0, 0, 2 ** 24, 2 ** 31]    # the largest first, and last
    smp = M.sampler(dev(v), dev(tris))
    assert_build(smp, b, "planted")
    assert smp.counts["status"] == _lib.MESH_STATUS_BAD_INDEX and smp.area == 16.0 + 2.0 ** -4
    for N, seed in ((1, 0), (1000, 1), (4097, 2)):
        want = R.sample(v, tris, N, seed, b=b)
        got = smp.sample(N, seed)
        assert_same(got, want, f"planted, N = {N}")
        assert set(got.cpu().triangle.tolist()) <= {0, 8, 9}
    t = smp.sample(4097, 2).cpu().triangle.numpy()
    assert abs(int((t == 8).sum()) - 4097 * 2.0 ** 24 / b["total"]) < 2 and abs(int((t == 0).sum()) - 4097 * 2.0 ** 31 / b["total"]) < 2


# ---- the sphere ------------------------------------------------------------------------------------------------------------------------
CENTRE = (1.0, 1.0, 1.0)


@pytest.fixture(scope="module")
def sphere():
    v, tris = S.uv_sphere(0.5, centre=CENTRE)
    return v, tris, R.build(v, tris)


def test_sphere(sphere):
    v, tris, b = sphere
    smp = M.sampler(dev(v), dev(tris))
    assert_build(smp, b, "sphere")
    want = R.sample(v, tris, 100_000, 4, b=b)
    got = smp.sample(100_000, 4)
    assert_same(got, want, "sphere")
    count = np.bincount(got.cpu().triangle.numpy(), minlength=tris.shape[0])
    assert np.abs(count - 100_000 * b["w"].astype(np.float64) / b["total"]).max() < 2
    # two runs are bit-identical; seed s and s + 1 differ; through the mesh as through the flat operator
    again = M.sampler(dev(v), dev(tris)).sample(100_000, 4)
    assert out_bytes(again) == out_bytes(got) and again.counts == got.counts
    other = smp.sample(100_000, 5)
    assert_same(other, R.sample(v, tris, 100_000, 5, b=b), "sphere, seed 5")
    assert out_bytes(other)[0] != out_bytes(got)[0]
    assert out_bytes(mesh_of(v, tris).sample(100_000, 4)) == out_bytes(got)
    for seed in (-1, 2 ** 64 + 3, 2 ** 63):                                       # any integer, modulo 2^64
        assert_same(smp.sample(300, seed), R.sample(v, tris, 300, seed, b=b), f"seed {seed}")


def test_meshes_without_area():
    v = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0]], F32)
    for tris, what in ((np.array([[0, 1, 2], [1, 1, 3], [0, 3, 2]], np.int32), "all degenerate"), (np.zeros((0, 3), np.int32), "K = 0")):
        smp = M.sampler(dev(v), dev(tris))
        assert_build(smp, R.build(v, tris), what)
        assert smp.total == 0 and smp.area == 0.0 and smp.counts["weightless"] == tris.shape[0] and smp.counts["exponent"] == 0
        for N in (0, 5, 300):
            got = smp.sample(N, 9)
            assert_same(got, R.sample(v, tris, N, 9), f"{what}, N = {N}")
            g = got.cpu()
            assert got.counts == dict(samples=0, status=0) and (g.triangle == -1).all() and torch.isnan(g.point).all() and torch.isnan(g.barycentric).all()
    smp = M.sampler(dev(np.zeros((0, 3), F32)), dev(np.array([[0, 1, 2]], np.int32)))  # V = 0: every index is bad, nothing is dereferenced
    assert smp.counts["bad_index"] == 1 and smp.counts["status"] == _lib.MESH_STATUS_BAD_INDEX and smp.total == 0
    assert smp.sample(3).counts == dict(samples=0, status=_lib.MESH_STATUS_BAD_INDEX)


# ---- interpolate -----------------------------------------------------------------------------------------------------------------------
def test_interpolate_on_samples(sphere):
    v, tris, b = sphere
    nrm = ((v - np.asarray(CENTRE, F32)) * F32(2)).astype(F32)
    m = M.IndexedMesh(dev(v), dev(nrm), dev(v[:, 0].copy()), dev(tris), dev(np.zeros((tris.shape[0],), np.int64)), {})
    s = m.sample(5000, 2)
    want = R.sample(v, tris, 5000, 2, b=b)
    got_n, got_s = m.interpolate(s, m.normals).cpu().numpy(), m.interpolate(s, m.vertex_std).cpu().numpy()
    assert got_n.tobytes() == R.interpolate(tris, want["triangle"], want["barycentric"], nrm).tobytes()
    assert got_s.tobytes() == R.interpolate(tris, want["triangle"], want["barycentric"], v[:, 0]).tobytes()
    # the vertices interpolated are the points themselves
    assert m.interpolate(s, m.vertices).cpu().numpy().tobytes() == want["point"].tobytes()
    assert np.abs(np.linalg.norm(got_n, axis=1) - 1).max() < 0.01                 # an xyz + normal cloud of the sphere


# ---- compare ---------------------------------------------------------------------------------------------------------------------------
def ref_direction(av, at, bv, bt, n, seed, r, taus):
    """One direction of `compare` from sample_ref + closest_ref, with compare's cell rule."""
    pts = R.sample(av, at, n, seed)["point"]
    cell = max(C.default_cell(bv, bt), float(F32(float(F32(r)) / 59)))
    want = C.closest(bv, bt, pts, r, cell)
    d2 = want["d2"]
    d = np.sqrt(d2[np.isfinite(d2)].astype(np.float64))
    stats = dict(mean=d.mean(), rms=np.sqrt((d * d).mean()), median=np.sort(d)[(d.size - 1) // 2], max=d.max()) if d.size else {}
    return dict(stats, found=want["counts"][0], far=want["counts"][1] + want["counts"][2], within=[int((d <= t).sum()) for t in taus])


def check_compare(a, b, av, at, bv, bt, r, what, n=2000, seed=6, taus=(0.005, 0.01, 0.02)):
    got = a.compare(b, r, n_samples=n, seed=seed, thresholds=taus)
    want = dict(accuracy=ref_direction(av, at, bv, bt, n, seed, r, taus), completeness=ref_direction(bv, bt, av, at, n, seed + 1, r, taus))
    for side in ("accuracy", "completeness"):
        g, w = got[side], want[side]
        print(f"{what}, {side}: " + ", ".join(f"{k} {g[k]}" for k in ("mean", "rms", "median", "max", "found", "far", "within")))
        assert (g["found"], g["far"], g["within"]) == (w["found"], w["far"], w["within"]), (what, side, g, w)
        assert g["found"] + g["far"] == n
        for k in ("mean", "rms", "median", "max"):
            assert abs(g[k] - w[k]) <= 1e-9 * abs(w[k]), (what, side, k, g[k], w[k])
    assert abs(got["chamfer"] - 0.5 * (want["accuracy"]["mean"] + want["completeness"]["mean"])) <= 1e-9 * got["chamfer"]
    P, Rc = [x / n for x in want["accuracy"]["within"]], [x / n for x in want["completeness"]["within"]]
    assert got["precision"] == P and got["recall"] == Rc and got["thresholds"] == tuple(taus)
    assert got["fscore"] == [2 * p * q / (p + q) if p + q > 0 else 0.0 for p, q in zip(P, Rc)]
    return got


def test_compare(sphere):
    v, tris, _ = sphere
    a = mesh_of(v, tris)
    small = a.simplify(0.2)
    s = small.cpu()
    sv, st = s.vertices.numpy(), s.triangles.numpy()
    assert 0 < st.shape[0] < tris.shape[0] // 4
    got = check_compare(a, small, v, tris, sv, st, 0.05, "sphere against simplify(0.2)")
    assert got["accuracy"]["mean"] > 1e-3          # what the vertices alone cannot see
    shifted = (v + np.array([0.01, 0, 0], F32)).astype(F32)
    got = check_compare(a, mesh_of(shifted, tris), v, tris, shifted, tris, 0.05, "sphere against itself shifted by 0.01")
    assert got["accuracy"]["max"] <= 0.01 + 1e-6 and got["recall"][2] == 1.0 and got["precision"][0] < 1.0
    # against itself: a sample is not a vertex, so its distance is the float32 error of sampling and of the closest operator, not zero: per axis
    # the point's own three roundings (3 u m, u = 2^-24, m = the largest |coordinate|) and the two margins the closest operator grants its own
    # float32 arithmetic (the registration's 2^-20 m and the query's slack 2^-21 m: closest_slack)
    m = float(np.abs(v).max())
    bound = np.sqrt(3.0) * (float(K.R.WIDEN) + 2.0 ** -21 + 3 * 2.0 ** -24) * m
    got = check_compare(a, a, v, tris, v, tris, 0.05, "sphere against itself")
    assert got["accuracy"]["max"] <= bound and got["completeness"]["max"] <= bound and got["fscore"] == [1.0, 1.0, 1.0]
    assert got["accuracy"]["found"] == 2000


# ---- through the map -------------------------------------------------------------------------------------------------------------------
def test_through_the_map(gpu_model):
    b = W.SPHERE_BOUND
    cfg = syn.MapConfig((-b, -b, -b), (b, b, b), W.SPHERE_VOXEL)
    m = DenseIndexedMap(gpu_model, cfg.namespace(), 29, DEV, initial_capacity=1024)
    xyz, nrm = CR.two_sphere_cloud()
    m.integrate_keyframe(dev(xyz), dev(nrm))
    m.extract_mesh_arrays(W.SPHERE_RES, int(4e6), fast=True, max_std=2000.0, to_host=False)
    mesh = m.indexed_mesh(min_component_triangles=500)
    got = mesh.sample(10_000, seed=3)
    c = mesh.cpu()
    v, tris = c.vertices.numpy(), c.triangles.numpy()
    assert_same(got, R.sample(v, tris, 10_000, 3), "through the map")
    smp = mesh.sampler()
    assert_build(smp, R.build(v, tris), "through the map")
    print(f"two spheres: {tris.shape[0]} triangles, area {smp.area:.6f}, {smp.counts}")
    nr = mesh.interpolate(got, mesh.normals)
    assert tuple(nr.shape) == (10_000, 3) and bool(torch.isfinite(nr).all())
    full = mesh.compare(mesh.simplify(4.0 * W.SPHERE_VOXEL / W.SPHERE_RES), 0.2, n_samples=2000)
    assert full["accuracy"]["found"] == 2000 and 0 < full["chamfer"] < 0.05


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_every_refusal():
    v, tris = S.tetrahedron()
    tv, tt = dev(v), dev(tris)
    with pytest.raises(RuntimeError):
        M.sampler(torch.from_numpy(v), tt)                                        # a host tensor
    with pytest.raises(RuntimeError):
        M.sampler(tv.double(), tt)
    with pytest.raises(RuntimeError):
        M.sampler(tv, tt.long())
    with pytest.raises(RuntimeError):
        M.sampler(tv[:, :2].contiguous(), tt)
    with pytest.raises(RuntimeError):
        M.sampler(tv, tt.reshape(-1))
    smp = M.sampler(tv, tt)
    for n in (-1, 2 ** 31):
        with pytest.raises(ValueError):
            smp.sample(n)
    a = mesh_of(v, tris)
    with pytest.raises(ValueError):
        a.compare(a, 0.01, n_samples=10, thresholds=(0.005, 0.02))
    # the C entry points
    lib = _lib.load()
    assert lib.dif_mesh_sampler_workspace_bytes(4, (2 ** 31 + 2) // 3) == -1 and lib.dif_mesh_sampler_workspace_bytes(2 ** 31, 4) == -1
    assert lib.dif_mesh_sampler_workspace_bytes(-1, 4) == -1 and lib.dif_mesh_sampler_workspace_bytes(0, 0) > 0
    P, ws = _lib.ptr, smp.workspace
    counts = torch.zeros((10,), dtype=torch.int32, device=DEV)
    total = torch.zeros((1,), dtype=torch.int64, device=DEV)
    out = [torch.empty((3, 3), dtype=torch.float32, device=DEV), torch.empty((3,), dtype=torch.int32, device=DEV), torch.empty((3, 3), dtype=torch.float32, device=DEV)]

    def build(wsp=None, nbytes=None, v_=tv, t_=tt, c_=counts, tot=total):
        return lib.dif_mesh_sampler_build(P(v_), P(t_), 4, 4, P(ws) if wsp is None else wsp, ws.numel() if nbytes is None else nbytes, P(c_), P(tot), _lib.stream_ptr())

    def draw(wsp=None, nbytes=None, v_=tv, t_=tt, c_=counts, n=3, o=out):
        return lib.dif_mesh_sample(P(v_), P(t_), 4, 4, P(ws) if wsp is None else wsp, ws.numel() if nbytes is None else nbytes, n, 0, P(o[0]), P(o[1]), P(o[2]), P(c_),
                                   _lib.stream_ptr())

    assert build() == 0 and draw() == 0 and draw(n=0, o=[None, None, None]) == 0
    for rc in (build(wsp=ctypes.c_void_p(0)), build(wsp=ctypes.c_void_p(ws.data_ptr() + 8)), build(nbytes=ws.numel() - 1), build(v_=None), build(t_=None),
               build(c_=None), build(tot=None), draw(wsp=ctypes.c_void_p(0)), draw(nbytes=ws.numel() - 1), draw(v_=None), draw(t_=None), draw(c_=None),
               draw(n=-1), draw(n=2 ** 31), draw(o=[None, out[1], out[2]]), draw(o=[out[0], None, out[2]]), draw(o=[out[0], out[1], None])):
        assert rc == -1
    torch.cuda.synchronize()
