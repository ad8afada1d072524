"""GPU: `dif_mesh_render` against its numpy restatement (tests/raster_ref.py), BIT FOR BIT — the four images compared as bytes (NaN included)
and every count — on small overlapping triangles around the wave and workgroup boundaries, the cooperative path for large triangles, the image
borders, every kind of dropped triangle, bad indices, shared edges and vertex fans, ties and culling, empty inputs; then through
`DenseIndexedMap.render_view` on the two-sphere scene of tests/test_gpu_components.py."""
import ctypes

import numpy as np
import pytest
import torch

from di_fusion_amd import _lib, synthetic as syn
from di_fusion_amd.system import mesh as M
from di_fusion_amd.system.map import DenseIndexedMap
from di_fusion_amd.system.tracker import Pose
from tests import components_ref as C
from tests import raster_ref as R
from tests import weld_ref as W

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F32, F64 = np.float32, np.float64
IMAGES = {"64x48": (48, 64, (60.0, 57.5, 31.37, 23.81)), "37x29": (29, 37, (41.25, 43.5, 17.6, 14.3))}       # H, W, (fx, fy, cx, cy)
IMAGE_NAMES = ("depth", "normal", "std", "triangle")
T = _lib.RASTER_THREAD_PIXELS


def turned_pose():
    a, b = 0.31, -0.17
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    P = np.eye(4)
    P[:3, :3], P[:3, 3] = Rx @ Ry, (0.23, -0.41, 0.37)
    return P


POSES = {"identity": np.eye(4), "turned": turned_pose()}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def check(mesh, pose, image, what, z_near=0.05, cull=False):
    """the flat operator on the GPU == the restatement: images as bytes, every count; returns (got on the host, want)"""
    H, Wd, intr = IMAGES[image] if isinstance(image, str) else image
    v, n, s, t = (np.ascontiguousarray(a) for a in mesh)
    want = R.render(v, n, s, t, R.world_to_cam(pose), intr, H, Wd, z_near=z_near, cull_backfaces=cull, thread_pixels=T)
    got = M.render(dev(v), dev(n), dev(s), dev(t), pose, intr, H, Wd, z_near=z_near, cull_backfaces=cull)
    assert got.counts == want["counts"], (what, got.counts, want["counts"])
    g = got.cpu()
    assert g.depth.dtype == g.normal.dtype == g.std.dtype == torch.float32 and g.triangle.dtype == torch.int32
    assert g.depth.shape == (H, Wd) and g.normal.shape == (H, Wd, 3) and g.std.shape == (H, Wd) and g.triangle.shape == (H, Wd)
    for name in IMAGE_NAMES:
        a, b = getattr(g, name).numpy(), want[name]
        if a.tobytes() != b.tobytes():
            bad = np.argwhere(a.view(np.uint32) != b.view(np.uint32))
            raise AssertionError(f"{what}: {name} differs at {len(bad)} places, first {bad[0].tolist()}: {a[tuple(bad[0])]!r} != {b[tuple(bad[0])]!r}")
    return g, want


def same_images(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in IMAGE_NAMES)


def concat(*meshes):
    """several (v, n, s, t) as one mesh"""
    off, out = 0, [[], [], [], []]
    for v, n, s, t in meshes:
        for k, a in enumerate((v, n, s, np.where(t >= 0, t + off, t).astype(np.int32))):
            out[k].append(a)
        off += v.shape[0]
    return tuple(np.concatenate(a) for a in out)


def screen_mesh(pose, image, uv, z, tris, seed=0):
    """vertices given by pixel position and depth"""
    intr = IMAGES[image][2]
    v = R.plane_points(R.world_to_cam(pose), intr, np.asarray(uv, dtype=F64), np.asarray(z, dtype=F64)).astype(F32)
    n, s = R.flat_attributes(v.shape[0], seed)
    return v, n, s, np.asarray(tris, dtype=np.int32).reshape(-1, 3)


# ---- small triangles -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 63, 64, 65, 257, 4097])
@pytest.mark.parametrize("image,pose", [("64x48", "turned"), ("37x29", "identity")])
def test_random_small_triangles(K, image, pose):
    H, Wd, intr = IMAGES[image]
    mesh = R.small_triangles(K, R.world_to_cam(POSES[pose]), intr, H, Wd, seed=K)
    g, want = check(mesh, POSES[pose], image, f"{K} small triangles, {image}, {pose}")
    c = want["counts"]
    assert c["drawn"] + c["degenerate"] + c["offscreen"] == K and c["clipped"] == 0 and c["large"] == 0 and c["status"] == 0
    if K >= 63:
        assert want["coverage"].max() >= 3 and c["pixels_hit"] >= 60                                  # they overlap
    if K >= 257:
        assert c["offscreen"] > 0 and c["pixels_hit"] > 200                                           # and some hang over the rim
    print(f"K {K} {image}: {c}, deepest stack {int(want['coverage'].max())}")


# ---- the cooperative path ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("image,pose", [("64x48", "turned"), ("37x29", "identity")])
def test_one_triangle_over_the_whole_image_with_small_ones_on_both_sides(image, pose):
    H, Wd, intr = IMAGES[image]
    P = POSES[pose]
    big = screen_mesh(P, image, [(-40.0, -30.0), (3.0 * Wd, -25.0), (-35.0, 3.0 * H)], [1.4, 1.9, 1.6], [[0, 1, 2]])
    w2c = R.world_to_cam(P)
    front = R.small_triangles(150, w2c, intr, H, Wd, seed=1, depth=(0.5, 1.0))
    behind = R.small_triangles(150, w2c, intr, H, Wd, seed=2, depth=(2.5, 3.0))
    g, want = check(concat(front, big, behind), P, image, f"large triangle, {image}")
    assert want["counts"]["large"] == 1 and want["counts"]["pixels_hit"] == H * Wd
    tri = want["triangle"]
    assert (tri == 150).sum() > H * Wd // 2 and (tri < 150).sum() > 50 and (tri > 150).sum() == 0
    # the large triangle alone, listed first, last and twice
    check(concat(big, front), P, image, "large triangle first")
    g2, w2 = check(concat(big, big), P, image, "large triangle twice")
    assert w2["counts"]["large"] == 2 and (w2["triangle"] == 0).all()


def boxes(n):
    return [(w, n // w) for w in range(1, n + 1) if n % w == 0]


@pytest.mark.parametrize("image,pose", [("64x48", "identity"), ("37x29", "turned")])
def test_boxes_of_exactly_the_thread_limit_and_one_more(image, pose):
    """Pixel boxes of w x h = RASTER_THREAD_PIXELS (the thread walks them) and RASTER_THREAD_PIXELS + 1 (the workgroup does), every shape that
    fits the image; both paths run the same pixel function, and both must give the restatement's pixels."""
    H, Wd, intr = IMAGES[image]
    meshes, n_large = [], 0
    rng = np.random.default_rng(5)
    for n in (T, T + 1):
        for w, h in boxes(n):
            if w + 3 > Wd or h + 3 > H:
                continue
            u0, v0 = int(rng.integers(0, Wd - w - 2)), int(rng.integers(0, H - h - 2))
            # pixel centres u0 + 1 .. u0 + w and v0 + 1 .. v0 + h lie inside the bounding box
            uv = [(u0 + 0.5, v0 + 0.5), (u0 + w + 0.2, v0 + 0.7), (u0 + 0.3 * w, v0 + h + 0.3)]
            meshes.append(screen_mesh(POSES[pose], image, uv, rng.uniform(0.8, 2.5, size=3), [[0, 1, 2]], seed=n + w))
            n_large += n == T + 1
    assert len(meshes) >= 6 and 0 < n_large < len(meshes)
    g, want = check(concat(*meshes), POSES[pose], image, f"boxes of {T} and {T + 1} pixels")
    assert want["counts"]["large"] == n_large and want["counts"]["drawn"] == len(meshes)
    assert len(np.unique(want["triangle"])) > len(meshes) // 2                     # (a sliver may hold no pixel centre, or hide behind another)


# ---- borders and drops -------------------------------------------------------------------------------------------------------------------
def base_mesh(pose, image):
    return screen_mesh(pose, image, [(6.5, 5.25), (25.2, 7.1), (14.4, 21.3), (20.5, 12.5), (34.0, 9.75), (27.75, 26.5)], [1.0, 1.3, 1.1, 0.9, 1.4, 1.2],
                       [[0, 1, 2], [3, 5, 4]])


@pytest.mark.parametrize("image,pose", [("64x48", "turned"), ("37x29", "identity")])
def test_image_borders(image, pose):
    H, Wd, intr = IMAGES[image]
    P = POSES[pose]
    over = [[(-3.2, 10.1), (2.7, 8.3), (1.1, 14.9)], [(Wd - 2.5, 5.5), (Wd + 4.1, 7.2), (Wd - 1.2, 12.8)],
            [(10.3, -2.9), (16.8, -1.1), (12.2, 3.4)], [(8.1, H - 3.3), (15.6, H - 1.4), (11.9, H + 3.8)],
            [(-2.4, -1.7), (3.9, -2.2), (-1.3, 4.6)], [(Wd - 2.2, H - 2.6), (Wd + 3.0, H - 1.0), (Wd - 1.5, H + 2.1)]]
    outside = [[(-9.2, 10.1), (-3.3, 8.3), (-4.9, 14.9)], [(Wd + 0.5, 5.5), (Wd + 7.1, 7.2), (Wd + 1.8, 12.8)],
               [(10.3, -7.9), (16.8, -6.1), (12.2, -1.6)], [(8.1, H + 0.3), (15.6, H + 2.4), (11.9, H + 6.8)]]
    uv = np.array(over + outside, dtype=F64).reshape(-1, 2)
    m = screen_mesh(P, image, uv, np.full(len(uv), 1.25), np.arange(len(uv)).reshape(-1, 3), seed=3)
    g, want = check(m, P, image, f"borders, {image}")
    assert want["counts"]["drawn"] == 6 and want["counts"]["offscreen"] == 4 and set(np.unique(want["triangle"]).tolist()) == {-1, 0, 1, 2, 3, 4, 5}
    # a vertex beyond the 2^22 guard (16,384 pixels): the triangle goes, the others stay
    far = screen_mesh(P, image, [(5.5, 5.5), (12.5, 20.5), (17000.0, 9.0), (5.5, 5.5), (12.5, 20.5), (-17000.0, 9.0), (5.5, 5.5), (12.5, 20.5), (16300.0, 9.0)],
                      np.full(9, 1.5), [[0, 1, 2], [3, 4, 5], [6, 7, 8]], seed=4)
    g2, want2 = check(concat(m, far), P, image, f"guard, {image}")
    assert want2["counts"]["clipped"] == 2 and want2["counts"]["large"] == 1 and want2["counts"]["drawn"] == 7


@pytest.mark.parametrize("image,pose", [("64x48", "identity"), ("37x29", "turned")])
def test_dropped_triangles_are_counted_and_leave_the_rest_alone(image, pose):
    P = POSES[pose]
    H, Wd, intr = IMAGES[image]
    base = base_mesh(P, image)
    _, alone = check(base, P, image, "base")
    assert alone["counts"]["drawn"] == 2 and alone["counts"]["pixels_hit"] > 100
    z_near = 0.25                                                                # (a float32: pc.z == z_near can be hit exactly under the identity)
    a, b = (8.5, 6.5), (22.5, 9.5)
    uv = [a, b, (15.0, 18.0), a, b, (15.0, 18.0), a, b, (15.0, 18.0), (10.0, 10.0), (12.0, 12.0), (14.0, 14.0), a, b, (15.0, 18.0)]
    # behind the camera; at z_near itself (exactly so under the identity, a hair behind it otherwise); one vertex short of z_near (the triangle
    # straddles the plane: no clipping, it goes); three snapped points on one line; a repeated index; NaN, +inf and -inf coordinates
    z = [1.0, 1.0, -0.7, 1.0, 1.0, z_near if pose == "identity" else z_near - 1e-3, 0.9, 1.1, 0.1, 1.0, 1.2, 1.4, 1.0, 1.0, 1.0]
    drops = list(screen_mesh(P, image, uv, z, [[0, 1, 2], [3, 4, 5], [6, 7, 8], [9, 10, 11], [0, 0, 1], [12, 0, 1], [0, 13, 1], [14, 1, 0]], seed=6))
    if pose == "identity":
        assert drops[0][5, 2] == F32(z_near)
    drops[0][12:15] = np.array([[np.nan, 0.1, 1.0], [0.1, np.inf, 1.0], [0.1, 0.2, -np.inf]], dtype=F32)
    g, want = check(concat(base, tuple(drops)), P, image, f"drops, {image}", z_near=z_near)
    c = want["counts"]
    assert (c["drawn"], c["clipped"], c["degenerate"], c["offscreen"], c["culled"], c["status"]) == (2, 6, 2, 0, 0, 0), c
    assert same_images(want, alone)


def test_bad_indices_are_reported_and_never_followed():
    """The index V: the word past the end of every (V,) array lies inside the same allocation, so a missing check shows as a wrong answer,
    never as a fault."""
    P, image = POSES["turned"], "64x48"
    H, Wd, intr = IMAGES[image]
    v, n, s, t = R.small_triangles(40, R.world_to_cam(P), intr, H, Wd, seed=9)
    V = v.shape[0]
    _, rest = check((v, n, s, t), P, image, "without the bad ones")
    ok = np.array([[0, 1, 2]], dtype=np.int32)
    tb = np.concatenate([t, [[7, V, 8]], [[0, 1, -1]], [[V + 5, 2, 3]]]).astype(np.int32)            # (V + 5 still lies in the allocations)
    g, want = check((v, n, s, tb), P, image, "index V, -1 and V + 5")
    assert want["counts"]["status"] == _lib.MESH_STATUS_BAD_INDEX == R.BAD_INDEX and g.triangle.max() < 40
    assert same_images(want, rest) and {k: c for k, c in want["counts"].items() if k != "status"} == {k: c for k, c in rest["counts"].items() if k != "status"}
    check((v[:0], n[:0], s[:0], ok), P, image, "no vertices at all")


@pytest.mark.parametrize("image,pose", [("64x48", "turned"), ("37x29", "identity")])
def test_shared_edge_and_fan(image, pose):
    H, Wd, intr = IMAGES[image]
    w2c = R.world_to_cam(POSES[pose])
    for name, (v, t) in (("shared edge", R.shared_edge_pair(w2c, intr)), ("fan", R.vertex_fan(w2c, intr))):
        n, s = R.flat_attributes(v.shape[0], 2)
        g, want = check((v, n, s, t), POSES[pose], image, f"{name}, {image}")
        assert want["coverage"].max() == 1 and want["counts"]["pixels_hit"] == int(want["coverage"].sum()) > 200
        X, Y, _, _ = R.project(v, w2c, intr, 0.05)
        assert (X[0] % 256, Y[0] % 256) == (0, 0)                                # vertex 0 sits on a pixel centre in both scenes
        assert want["triangle"][Y[0] // 256, X[0] // 256] >= 0


@pytest.mark.parametrize("cull", [False, True])
def test_ties_and_culling(cull):
    P, image = POSES["turned"], "64x48"
    base = base_mesh(P, image)                                                   # triangle 0 faces away from the camera, triangle 1 faces it
    v, n, s, t = base
    n2, s2 = R.flat_attributes(v.shape[0], 11)                                   # the copies carry other attributes: the owner shows
    twice = concat(base, (v, n2, s2, t), (v, n2, s2, t[:, [0, 2, 1]]))
    g, want = check(twice, P, image, f"duplicates, cull {cull}", cull=cull)
    seen = set(np.unique(want["triangle"]).tolist())
    _, alone = check(base, P, image, "base", cull=cull)
    if cull:                                                                     # of the three copies of triangle 0 only the turned one (4) faces the camera
        assert seen == {-1, 1, 4} and want["counts"]["culled"] == 3 and want["counts"]["drawn"] == 3
        assert np.array_equal(want["triangle"] == 1, alone["triangle"] == 1) and alone["counts"]["culled"] == 1
    else:                                                                        # a turned copy is the same oriented triangle: equal depths, the lower index
        assert seen == {-1, 0, 1} and want["counts"]["culled"] == 0 and want["counts"]["drawn"] == 6
        assert same_images(want, alone)
    # a nearer triangle listed later still wins
    near = screen_mesh(P, image, [(6.5, 5.25), (14.4, 21.3), (25.2, 7.1)], [0.8, 0.8, 0.8], [[0, 1, 2]], seed=12)
    g, want = check(concat(base, near), P, image, "nearer and later", cull=cull)
    assert (want["triangle"] == 2).sum() > 50 and (want["triangle"] == 0).sum() == 0


def test_empty_inputs_a_single_pixel_and_a_repeat():
    P = POSES["identity"]
    v, n, s, t = base_mesh(P, "64x48")
    g, want = check((v, n, s, t[:0]), P, "64x48", "no triangles")
    assert want["counts"] == dict.fromkeys(R.COUNT_NAMES, 0) and np.isnan(g.depth.numpy()).all() and (g.triangle.numpy() == -1).all()
    check((v[:0], n[:0], s[:0], t[:0]), P, "37x29", "nothing at all")
    one = (1, 1, (50.0, 50.0, 0.0, 0.0))
    w2c = R.world_to_cam(P)
    pv = R.plane_points(w2c, one[2], np.array([(-0.5, -0.5), (1.0, -0.25), (-0.25, 1.0)]), np.array([1.0, 1.5, 2.0])).astype(F32)
    pn, ps = R.flat_attributes(3)
    g, want = check((pv, pn, ps, np.array([[0, 1, 2]], dtype=np.int32)), P, one, "1 x 1")
    assert want["counts"]["pixels_hit"] == 1 and g.triangle.tolist() == [[0]]
    H, Wd, intr = IMAGES["64x48"]
    mesh = R.small_triangles(4097, R.world_to_cam(POSES["turned"]), intr, H, Wd, seed=21)
    d = [dev(a) for a in mesh]
    a = M.render(*d, POSES["turned"], intr, H, Wd).cpu()
    b = M.render(*d, POSES["turned"], intr, H, Wd).cpu()
    assert a.counts == b.counts and all(getattr(a, k).numpy().tobytes() == getattr(b, k).numpy().tobytes() for k in IMAGE_NAMES)


def test_arguments_are_checked():
    P = POSES["identity"]
    H, Wd, intr = IMAGES["64x48"]
    v, n, s, t = base_mesh(P, "64x48")
    d = [dev(a) for a in (v, n, s, t)]
    with pytest.raises(RuntimeError):
        M.render(torch.from_numpy(v), d[1], d[2], d[3], P, intr, H, Wd)                       # host tensor
    with pytest.raises(RuntimeError):
        M.render(d[0], d[1], d[2], torch.from_numpy(t), P, intr, H, Wd)
    with pytest.raises(RuntimeError):
        M.render(d[0].double(), d[1], d[2], d[3], P, intr, H, Wd)
    with pytest.raises(RuntimeError):
        M.render(d[0], d[1], d[2], d[3].long(), P, intr, H, Wd)
    with pytest.raises(RuntimeError):
        M.render(d[0], d[1][:-1], d[2], d[3], P, intr, H, Wd)
    with pytest.raises(RuntimeError, match="DIF_EINVAL"):
        M.render(*d, P, intr, 0, Wd)
    with pytest.raises(RuntimeError, match="DIF_EINVAL"):
        M.render(*d, P, (0.0, 60.0, 1.0, 1.0), H, Wd)
    with pytest.raises(RuntimeError, match="DIF_EINVAL"):
        M.render(*d, P, (60.0, float("nan"), 1.0, 1.0), H, Wd)
    # the entry point itself: H = 0, and a workspace one byte short
    lib = _lib.load()
    assert lib.dif_mesh_render_workspace_bytes(6, 2, 0, Wd) == -1 and lib.dif_mesh_render_workspace_bytes(6, 2, 1 << 16, 1 << 15) == -1
    need = int(lib.dif_mesh_render_workspace_bytes(6, 2, H, Wd))
    ws = torch.empty((need,), dtype=torch.uint8, device=DEV)
    out = [torch.empty(shape, dtype=dt, device=DEV) for shape, dt in (((H, Wd), torch.float32), ((H, Wd, 3), torch.float32), ((H, Wd), torch.float32),
                                                                     ((H, Wd), torch.int32), ((_lib.RASTER_COUNT,), torch.int32))]

    def call(height, ws_bytes):
        args = M.raster_args(P, intr, height, Wd)
        return lib.dif_mesh_render(*(_lib.ptr(x) for x in d), 6, 2, ctypes.byref(args), _lib.ptr(ws), ws_bytes, *(_lib.ptr(x) for x in out), _lib.stream_ptr())

    assert call(0, need) == -1 and call(H, need - 1) == -1 and call(H, need) == 0
    torch.cuda.synchronize()
    assert out[4].cpu().tolist()[_lib.RASTER_DRAWN] == 2


# ---- through the map -------------------------------------------------------------------------------------------------------------------
VIEW = (48, 64, (60.0, 60.0, 32.0, 24.0))                  # the principal point is the centre of pixel (32, 24)


@pytest.fixture(scope="module")
def two_sphere_map(gpu_model):
    b = W.SPHERE_BOUND
    cfg = syn.MapConfig((-b, -b, -b), (b, b, b), W.SPHERE_VOXEL)
    m = DenseIndexedMap(gpu_model, cfg.namespace(), 29, DEV, initial_capacity=1024)
    assert m.render_view(np.eye(4), VIEW[2], VIEW[0], VIEW[1]) is None             # a fresh map has nothing to show
    xyz, nrm = C.two_sphere_cloud()
    m.integrate_keyframe(dev(xyz), dev(nrm))
    m.extract_mesh_arrays(W.SPHERE_RES, int(4e6), fast=True, max_std=2000.0, to_host=False)
    return m


def render_bytes(r: M.MeshRender):
    g = r.cpu()
    return [getattr(g, k).numpy().tobytes() for k in IMAGE_NAMES]


def test_through_the_map(two_sphere_map):
    m = two_sphere_map
    H, Wd, intr = VIEW
    centre = np.array([0.013, -0.021, 0.007])                                    # weld_ref.sphere_cloud
    pose = np.eye(4)
    pose[:3, 3] = centre + np.array([0.0, 0.0, -2.0])
    mesh = m.indexed_mesh()
    got = m.render_view(pose, intr, H, Wd)
    host = mesh.cpu()
    want = R.render(host.vertices.numpy(), host.normals.numpy(), host.vertex_std.numpy(), host.triangles.numpy(), R.world_to_cam(pose), intr, H, Wd,
                    thread_pixels=T)
    g = got.cpu()
    assert got.counts == want["counts"], (got.counts, want["counts"])
    for name in IMAGE_NAMES:
        assert getattr(g, name).numpy().tobytes() == want[name].tobytes(), name
    print(f"two-sphere map at {Wd}x{H}: {got.counts}, {mesh.counts['triangles']} triangles")
    # the same through every door
    assert render_bytes(m.render_view(pose, intr, H, Wd, mesh=mesh)) == render_bytes(mesh.render(pose, intr, H, Wd)) == render_bytes(got)
    assert render_bytes(m.render_view(Pose(pose[:3, :3], pose[:3, 3]), intr, H, Wd)) == render_bytes(got)
    from types import SimpleNamespace
    assert render_bytes(m.render_view(pose, SimpleNamespace(fx=intr[0], fy=intr[1], cx=intr[2], cy=intr[3]), H, Wd)) == render_bytes(got)
    # without the fragments: only triangles of the two closed spheres are named
    kept = m.indexed_mesh(min_component_triangles=500)
    topo = kept.topology()
    assert topo.count == 2 and topo.n_boundary.tolist() == [0, 0] and topo.euler.tolist() == [2, 2]
    r500 = m.render_view(pose, intr, H, Wd, min_component_triangles=500)
    assert render_bytes(r500) == render_bytes(kept.render(pose, intr, H, Wd))
    tri = r500.triangle.cpu().numpy()
    named = np.unique(tri[tri >= 0])
    comp = topo.triangle_component.cpu().numpy()
    assert named.max() < kept.counts["triangles"] and set(comp[named].tolist()) == {0, 1}           # both spheres are in view
    # sanity, not a precision pin: the depth at the principal point is the front of the large sphere, within a voxel
    d = float(g.depth[24, 32])
    print(f"depth at the principal point {d:.6f}, analytic {2 - 0.45:.6f}, difference {d - (2 - 0.45):+.6f} m (voxel {W.SPHERE_VOXEL})")
    assert abs(d - (2.0 - 0.45)) < W.SPHERE_VOXEL
    culled = m.render_view(pose, intr, H, Wd, cull_backfaces=True, mesh=mesh)
    print(f"with culling: {culled.counts}")
