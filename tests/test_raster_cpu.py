"""CPU: the numpy restatement of the mesh renderer (tests/raster_ref.py) held to what a renderer must produce — single ownership of every pixel
on shared edges and vertices, the analytic sphere, a fronto-parallel plane, the round trip through the project's pixel convention, ties,
attributes and back-face culling.  tests/test_gpu_raster.py then holds the kernels to the restatement bit for bit."""
import re

import numpy as np
import pytest

from tests import raster_ref as R
from tests.conftest import ROOT

F32, F64 = np.float32, np.float64
H, W = 48, 64
INTR = (60.0, 60.0, 31.5, 23.5)
DIST, RADIUS = 1.5, 0.45


def look_at_origin(eye):
    """camera-to-world 4x4 of a camera at `eye` whose +z axis points at the origin (x right, y down)"""
    eye = np.asarray(eye, dtype=F64)
    z = -eye / np.linalg.norm(eye)
    x = np.cross(np.array([0.0, 1.0, 0.0]), z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    T = np.eye(4)
    T[:3, 0], T[:3, 1], T[:3, 2], T[:3, 3] = x, y, z, eye
    return T


POSE_AXIS = look_at_origin((0.0, 0.0, -DIST))
POSE_TURNED = look_at_origin((0.7, -0.5, -1.2))           # |eye| = 1.4849...


@pytest.fixture(scope="module")
def sphere():
    return R.icosphere(4, RADIUS)


@pytest.fixture(scope="module")
def sphere_views(sphere):
    return {name: R.render(*sphere, R.world_to_cam(pose), INTR, H, W) for name, pose in (("axis", POSE_AXIS), ("turned", POSE_TURNED))}


def snap_delta(vertices, tris, pose):
    """delta = z_max sqrt(2) / (512 min(fx, fy)): the farthest the 1/256-pixel snap moves a vertex sideways, z_max = the farthest vertex of a
    triangle that faces the camera (float64, from the mesh)"""
    v = np.asarray(vertices, dtype=F64)
    eye = pose[:3, 3]
    p0, p1, p2 = (v[tris[:, k]] for k in range(3))
    front = np.einsum("ij,ij->i", np.cross(p1 - p0, p2 - p0), p0 - eye) < 0
    zc = (v - eye) @ pose[:3, 2]
    return zc[np.unique(tris[front])].max() * np.sqrt(2.0) / (512.0 * min(INTR[0], INTR[1]))


def sphere_entry(pose, radius):
    """camera depth (z) at which the ray of every pixel enters the sphere of `radius` about the origin (NaN: it misses), and the incidence cosine"""
    fx, fy, cx, cy = INTR
    v, u = np.meshgrid(np.arange(H, dtype=F64), np.arange(W, dtype=F64), indexing="ij")
    d = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], axis=-1) @ pose[:3, :3].T          # world direction per unit of camera z
    o = pose[:3, 3]
    a, b, c = (d * d).sum(-1), 2.0 * (d @ o), o @ o - radius * radius
    disc = b * b - 4.0 * a * c
    with np.errstate(invalid="ignore"):
        z = np.where(disc >= 0.0, (-b - np.sqrt(disc)) / (2.0 * a), np.nan)
    p = o + z[..., None] * d
    cos = -np.einsum("ijk,ijk->ij", d / np.sqrt(a)[..., None], p / radius)
    return z, cos


def test_constants_match_the_header_and_the_binding():
    from di_fusion_amd import _lib
    src = (ROOT / "include" / "difusion.h").read_text()
    assert int(re.search(r"DIF_RASTER_THREAD_PIXELS\s*=\s*(\d+)", src).group(1)) == _lib.RASTER_THREAD_PIXELS == R.THREAD_PIXELS <= 256
    for name, val in re.findall(r"DIF_RASTER_([A-Z_]+)\s*=\s*(\d+)", src):
        assert getattr(_lib, f"RASTER_{name}") == int(val), name
    from di_fusion_amd.system import mesh as M
    assert M.RENDER_COUNT_NAMES == R.COUNT_NAMES and len(R.COUNT_NAMES) == _lib.RASTER_COUNT
    assert ctypes_size(_lib.DifRasterArgs) == 12 * 4 + 5 * 4 + 3 * 4


def ctypes_size(t):
    import ctypes
    return ctypes.sizeof(t)


def test_world_to_cam_matches_the_operator():
    from di_fusion_amd.system import mesh as M
    from di_fusion_amd.system.tracker import Pose
    want = R.world_to_cam(POSE_TURNED)
    assert want.dtype == F32 and want.shape == (12,)
    for pose in (POSE_TURNED, Pose(POSE_TURNED[:3, :3], POSE_TURNED[:3, 3])):
        assert np.array_equal(M.world_to_cam_rows(pose), want)
    r = want.reshape(3, 4).astype(F64)
    assert np.abs(r[:, :3] @ POSE_TURNED[:3, 3] + r[:, 3]).max() < 1e-6               # the eye is the camera's origin


@pytest.mark.parametrize("view", ["axis", "turned"])
def test_closed_sphere_covers_every_pixel_zero_or_two_times(sphere_views, view):
    r = sphere_views[view]
    assert set(np.unique(r["coverage"]).tolist()) == {0, 2}
    c = r["counts"]
    assert c["clipped"] == 0 and c["culled"] == 0 and c["status"] == 0 and c["drawn"] + c["degenerate"] + c["offscreen"] == 5120
    assert c["pixels_hit"] == int((r["coverage"] == 2).sum()) == int((r["triangle"] >= 0).sum()) > 900
    assert np.array_equal(np.isnan(r["depth"]), r["triangle"] < 0) and np.array_equal(np.isnan(r["std"]), r["triangle"] < 0)
    assert not r["normal"][r["triangle"] < 0].any()


@pytest.mark.parametrize("pose", [POSE_AXIS, POSE_TURNED], ids=["axis", "turned"])
def test_shared_edge_and_fan_give_each_pixel_one_owner(pose):
    w2c = R.world_to_cam(pose)
    v, t = R.shared_edge_pair(w2c, INTR)
    X, Y, _, valid = R.project(v, w2c, INTR, 0.05)
    assert valid.all() and X.tolist() == [8 * 256, 24 * 256, 24 * 256, 8 * 256] and Y.tolist() == [8 * 256, 24 * 256, 8 * 256, 24 * 256]
    n, s = R.flat_attributes(4)
    r = R.render(v, n, s, t, w2c, INTR, H, W)
    cov = r["coverage"]
    assert cov.max() == 1
    assert (cov[9:24, 9:24] == 1).all()                                       # the open square's centres, the diagonal among them
    diag = r["triangle"][np.arange(8, 25), np.arange(8, 25)]
    assert len(set(diag[1:-1].tolist())) == 1 and diag[1] >= 0                 # one triangle owns the whole shared edge
    assert cov.sum() in (15 * 15 + 16 + 16, 15 * 15 + 16 + 15, 15 * 15 + 15 + 16)        # top and left rim in, bottom and right rim out (corners: by the rule)
    assert cov[24, 9:24].sum() == 0 and cov[9:24, 24].sum() == 0              # bottom and right edges
    assert (cov[8, 9:24] == 1).all() and (cov[9:24, 8] == 1).all()            # top and left edges
    v, t = R.vertex_fan(w2c, INTR)
    X, Y, _, _ = R.project(v, w2c, INTR, 0.05)
    assert (X[0], Y[0]) == (20 * 256, 15 * 256)
    n, s = R.flat_attributes(v.shape[0])
    r = R.render(v, n, s, t, w2c, INTR, H, W)
    assert r["coverage"].max() == 1 and r["coverage"][15, 20] == 1
    jj, ii = np.mgrid[0:H, 0:W]
    inside = (ii - 20) ** 2 + (jj - 15) ** 2 < (9.3 * np.cos(np.pi / 7) - 0.01) ** 2       # the fan's inscribed circle
    assert (r["coverage"][inside] == 1).all() and inside.sum() > 200


@pytest.mark.parametrize("view,pose", [("axis", POSE_AXIS), ("turned", POSE_TURNED)])
def test_against_the_analytic_sphere(sphere, sphere_views, view, pose):
    v, _, _, tris = sphere
    r = sphere_views[view]
    p = v.astype(F64)
    nrm = np.cross(p[tris[:, 1]] - p[tris[:, 0]], p[tris[:, 2]] - p[tris[:, 0]])
    r_in = np.abs(np.einsum("ij,ij->i", nrm / np.linalg.norm(nrm, axis=1, keepdims=True), p[tris[:, 0]])).min()
    assert 0.99 * RADIUS < r_in < RADIUS
    z_out, cos = sphere_entry(pose, RADIUS)
    z_in, _ = sphere_entry(pose, r_in)
    covered = r["triangle"] >= 0
    holes, stray = int((~np.isnan(z_in) & ~covered).sum()), int((np.isnan(z_out) & covered).sum())
    delta = snap_delta(v, tris, pose)
    sel = covered & (cos >= 0.5)
    lo, hi = (z_out - r["depth"])[sel].max(), (r["depth"] - z_in)[sel].max()
    print(f"{view}: r_in {r_in:.6f}, holes {holes}, stray {stray}, delta {delta:.3e}, depth below entry(R) by {lo:.3e}, above entry(r_in) by {hi:.3e}, {int(sel.sum())} pixels")
    assert holes == 0 and stray == 0
    assert sel.sum() > 500 and lo <= 2.0 * delta and hi <= 2.0 * delta


def test_fronto_parallel_plane():
    """three products, two sums, one divide and one cast: every covered depth within relative 2^-22 of the plane's"""
    w2c = R.world_to_cam(np.eye(4))
    q = [(-3.3, -2.2), (70.1, -2.9), (69.4, 51.2), (-2.7, 50.6), (33.3, 21.7)]
    v = np.stack([R.plane_point(w2c, INTR, a, b, 2.0) for a, b in q]).astype(F32)
    assert (v[:, 2] == 2.0).all()
    t = np.array([[0, 1, 4], [1, 2, 4], [2, 3, 4], [3, 0, 4]], dtype=np.int32)
    n, s = R.flat_attributes(5)
    r = R.render(v, n, s, t, w2c, INTR, H, W)
    assert (r["coverage"] == 1).all() and r["counts"]["pixels_hit"] == H * W and r["counts"]["large"] == 4
    err = np.abs(r["depth"].astype(F64) / 2.0 - 1.0).max()
    print(f"plane: relative depth error {err:.3e} (bound {2.0 ** -22:.3e})")
    assert err <= 2.0 ** -22


def unproject_f32(depth):
    """k_unproject: x = (u - cx) / fx * d in float32"""
    fx, fy, cx, cy = (F32(a) for a in INTR)
    v, u = np.meshgrid(np.arange(H, dtype=F32), np.arange(W, dtype=F32), indexing="ij")
    return np.stack([(u - cx) / fx * depth, (v - cy) / fy * depth, depth], axis=-1)


@pytest.mark.parametrize("view,pose", [("axis", POSE_AXIS), ("turned", POSE_TURNED)])
def test_round_trip_through_the_pixel_convention(sphere, sphere_views, view, pose):
    """depth -> points as k_unproject makes them -> world: each lies on the plane of the triangle the pixel names, within 2 delta"""
    v, _, _, tris = sphere
    r = sphere_views[view]
    pts = unproject_f32(r["depth"])
    assert pts.dtype == F32
    hit = r["triangle"] >= 0
    world = pts[hit].astype(F64) @ pose[:3, :3].T + pose[:3, 3]
    p = v.astype(F64)
    t = tris[r["triangle"][hit]]
    nrm = np.cross(p[t[:, 1]] - p[t[:, 0]], p[t[:, 2]] - p[t[:, 0]])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    dist = np.abs(np.einsum("ij,ij->i", world - p[t[:, 0]], nrm))
    delta = snap_delta(v, tris, pose)
    print(f"{view}: round trip, largest distance to the named triangle's plane {dist.max():.3e} m (delta {delta:.3e})")
    assert dist.max() <= 2.0 * delta
    assert np.isnan(pts[~hit]).all()


def test_ties_go_to_the_lower_index_and_the_nearer_triangle_wins():
    w2c = R.world_to_cam(np.eye(4))
    far = np.stack([R.plane_point(w2c, INTR, a, b, 2.0) for a, b in ((5.2, 4.1), (40.3, 6.6), (20.9, 38.8))])
    near = np.stack([R.plane_point(w2c, INTR, a, b, 1.0) for a, b in ((10.5, 8.5), (30.2, 10.1), (20.4, 25.3))])
    v = np.concatenate([far, far, near]).astype(F32)
    n, s = R.flat_attributes(9)
    t = np.array([[3, 4, 5], [0, 1, 2], [0, 1, 2], [6, 7, 8]], dtype=np.int32)
    r = R.render(v, n, s, t, w2c, INTR, H, W)
    assert set(np.unique(r["triangle"]).tolist()) == {-1, 0, 3}                 # 1 and 2 are copies of 0: never seen
    assert r["coverage"].max() == 4 and (r["triangle"][r["coverage"] == 4] == 3).all()
    assert (r["triangle"][r["coverage"] == 3] == 0).all() and (r["coverage"] == 3).sum() > 100
    assert np.allclose(r["depth"][r["triangle"] == 3], 1.0, rtol=1e-6, atol=0) and np.allclose(r["depth"][r["triangle"] == 0], 2.0, rtol=1e-6, atol=0)


def test_constant_attributes_come_back_and_culling_takes_the_triangle_that_faces_away():
    w2c = R.world_to_cam(POSE_TURNED)
    q = [(5.2, 4.1), (40.3, 6.6), (20.9, 38.8), (45.5, 30.5), (60.25, 12.75), (50.5, 44.0)]
    z = [1.1, 1.7, 1.4, 0.9, 1.3, 1.2]
    v = np.stack([R.plane_point(w2c, INTR, a, b, d) for (a, b), d in zip(q, z)]).astype(F32)
    nv = np.array([0.36, -0.48, 0.8], dtype=F32)
    n = np.tile(nv, (6, 1))
    s = np.full(6, 0.0123, dtype=F32)
    t = np.array([[0, 1, 2], [3, 5, 4]], dtype=np.int32)
    p = v.astype(F64)
    eye = POSE_TURNED[:3, 3]
    away = [float(np.cross(p[b] - p[a], p[c] - p[a]) @ (p[a] - eye)) > 0 for a, b, c in t.tolist()]
    assert away == [True, False]                                               # (screen x right, y down: a clockwise triangle on screen faces away)
    r = R.render(v, n, s, t, w2c, INTR, H, W)
    hit = r["triangle"] >= 0
    assert set(np.unique(r["triangle"]).tolist()) == {-1, 0, 1} and r["counts"]["drawn"] == 2
    unit = nv.astype(F64) / np.linalg.norm(nv.astype(F64))
    assert (np.abs(r["normal"][hit].astype(F64) - unit) <= np.spacing(np.abs(unit).astype(F32))).all()      # 1 ulp of each component's own binade
    assert np.abs(r["std"][hit] - s[0]).max() <= np.spacing(s[0])
    c = R.render(v, n, s, t, w2c, INTR, H, W, cull_backfaces=True)
    assert c["counts"]["culled"] == 1 and c["counts"]["drawn"] == 1 and set(np.unique(c["triangle"]).tolist()) == {-1, 1}
    keep = r["triangle"] == 1
    assert np.array_equal(c["triangle"] == 1, keep) and np.array_equal(c["depth"][keep].view(np.uint32), r["depth"][keep].view(np.uint32))
    flipped = R.render(v, n, s, t[:, [0, 2, 1]], w2c, INTR, H, W, cull_backfaces=True)
    assert set(np.unique(flipped["triangle"]).tolist()) == {-1, 0}


def test_culling_leaves_the_front_of_the_closed_sphere(sphere, sphere_views):
    r = sphere_views["turned"]
    c = R.render(*sphere, R.world_to_cam(POSE_TURNED), INTR, H, W, cull_backfaces=True)
    assert set(np.unique(c["coverage"]).tolist()) == {0, 1} and c["counts"]["culled"] > 2000
    for name in ("depth", "normal", "std", "triangle"):
        assert c[name].tobytes() == r[name].tobytes(), name


def test_drops_are_counted():
    w2c = R.world_to_cam(np.eye(4))
    good = np.stack([R.plane_point(w2c, INTR, a, b, 1.0) for a, b in ((10.5, 8.5), (30.2, 10.1), (20.4, 25.3))])
    v = np.concatenate([good, [[0.0, 0.0, -1.0], [0.0, 0.0, 0.05], [np.nan, 0.0, 1.0], [0.0, np.inf, 1.0], [1e6, 0.0, 1.0], [-5.0, -5.0, 1.0]]]).astype(F32)
    t = np.array([[0, 1, 2], [0, 1, 3], [0, 1, 4], [0, 1, 5], [0, 1, 6], [0, 1, 7], [0, 0, 1], [0, 1, 9], [0, -1, 1], [8, 8, 0]], dtype=np.int32)
    n, s = R.flat_attributes(9)
    r = R.render(v, n, s, t, w2c, INTR, H, W, z_near=0.05)
    one = R.render(v, n, s, t[:1], w2c, INTR, H, W, z_near=0.05)
    c = r["counts"]
    assert (c["drawn"], c["clipped"], c["degenerate"], c["culled"], c["offscreen"], c["status"]) == (1, 5, 2, 0, 0, R.BAD_INDEX)
    for name in ("depth", "normal", "std", "triangle"):
        assert r[name].tobytes() == one[name].tobytes(), name
    off = R.render(v, n, s, np.array([[8, 8, 8], [0, 8, 1]], dtype=np.int32), w2c, INTR, H, W)
    assert off["counts"]["degenerate"] == 1 and off["counts"]["drawn"] == 1
