"""GPU: `dif_mesh_locator_build` / `dif_mesh_closest` against their numpy restatement (tests/closest_ref.py: the all-pairs minimum, no grid),
byte for byte — every output array, every count — on an analytic sphere at three cell sizes, on the mesh's own vertices, on planted points and
triangles at every edge of the contract, on a translated soup with queries planted on cell borders, beside a scene-sized triangle on the large
list; sizes, capacity, stride, repeats, refusals; and through `DenseIndexedMap.indexed_mesh()` on the two-sphere scene."""
import ctypes

import numpy as np
import pytest
import torch

from di_fusion_amd import _lib, synthetic as syn
from di_fusion_amd.system import mesh as M
from di_fusion_amd.system.map import DenseIndexedMap
from tests import closest_ref as R
from tests import closest_slack as K
from tests import components_ref as C
from tests import simplify_ref as S
from tests import weld_ref as W
from tests.test_closest_cpu import TRI_V, planted_points

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F32 = np.float32
OUT_NAMES = ("d2", "triangle", "point", "barycentric")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def out_bytes(c: M.MeshClosest):
    g = c.cpu()
    assert g.d2.dtype == torch.float32 and g.triangle.dtype == torch.int32 and g.point.dtype == torch.float32 and g.barycentric.dtype == torch.float32
    return [getattr(g, k).numpy().tobytes() for k in OUT_NAMES]


def assert_same(got: M.MeshClosest, want: dict, what):
    assert [got.counts[k] for k in R.QUERY_NAMES] == want["counts"], (what, got.counts, want["counts"])
    g = got.cpu()
    for k in OUT_NAMES:
        a, b = getattr(g, k).numpy(), want[k]
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == np.ascontiguousarray(b).tobytes(), (what, k)


def assert_build(loc: M.MeshLocator, v, tris, what, max_cells=R.MAX_CELLS):
    want = R.registration(v, tris, loc.counts["cell"], max_cells)
    assert [loc.counts[k] for k in R.BUILD_NAMES] == want, (what, loc.counts, want)


def check(v, tris, q, max_distance, cell, what, want=None, **kw):
    loc = M.locator(dev(v), dev(tris), cell, **kw)
    if int(np.asarray(tris).shape[0]) <= 4000:
        assert_build(loc, v, tris, what, kw.get("max_cells") or R.MAX_CELLS)
    got = loc.closest(dev(q), max_distance)
    want = R.closest(v, tris, q, max_distance, loc.counts["cell"]) if want is None else want
    assert_same(got, want, what)
    return loc, got, want


# ---- the sphere ------------------------------------------------------------------------------------------------------------------------
CENTRE = (1.0, 1.0, 1.0)                     # inside one cell of edge 4; no coordinate is a zero


@pytest.fixture(scope="module")
def sphere():
    v, tris = S.uv_sphere(0.5, centre=CENTRE)
    rng = np.random.default_rng(11)
    d = rng.normal(size=(2000, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    r = np.repeat([0.3, 0.5, 0.7, 0.9], 500)                                   # inside, on, outside, beyond max_distance
    q = (np.asarray(CENTRE) + d * r[:, None]).astype(F32)
    want = R.closest(v, tris, q, 0.25, 0.1)
    assert want["counts"] == [1500, 500, 0, 0]
    return v, tris, q, want


@pytest.mark.parametrize("cell,kind", [(None, "default"), (0.01, "large"), (4.0, "one cell")])
def test_sphere_at_three_cell_sizes(sphere, cell, kind):
    v, tris, q, want = sphere
    loc, got, _ = check(v, tris, q, 0.25, cell, f"sphere, {kind}", want)
    c = loc.counts
    print(f"sphere, {kind}: {c}")
    if kind == "default":
        assert c["cell"] == R.default_cell(v, tris) and c["large"] == 0
        again = M.locator(dev(v), dev(tris)).closest(dev(q), 0.25)               # two runs are bit-identical
        assert out_bytes(again) == out_bytes(got) and again.counts == got.counts
    elif kind == "large":
        assert c["large"] > c["indexed"]
    else:
        assert c["cells"] == 1 and c["pairs"] == c["indexed"] == tris.shape[0]
    assert torch.equal(got.distance, torch.sqrt(got.d2))


def test_own_vertices_are_at_distance_zero(sphere):
    v, tris = sphere[:2]
    _, got, _ = check(v, tris, v, 0.05, None, "own vertices")
    g = got.cpu()
    assert (g.d2.numpy() == 0).all() and g.point.numpy().tobytes() == v.tobytes() and got.counts["found"] == v.shape[0]


def test_all_pairs_path_gives_the_same(sphere):
    v, tris, q, want = sphere
    loc, _, _ = check(v, tris, q, 0.25, None, "every triangle large", want, max_cells=-1)
    assert loc.counts["indexed"] == 0 and loc.counts["large"] == tris.shape[0] and loc.counts["pairs"] == 0


# ---- planted points and triangles ------------------------------------------------------------------------------------------------------
def test_planted_set():
    rows = planted_points()
    nan, inf = np.nan, np.inf
    v = np.concatenate([TRI_V, [[nan, 0, 0], [2, 0, 0], [3, 0, 0], [1e30, 0, 0]]]).astype(F32)
    # the triangle of the CPU test, its copy, and: a NaN vertex, out-of-range indices, exactly collinear, a repeated index, beyond the key range
    tris = np.array([[0, 1, 2], [0, 1, 2], [0, 1, 4], [0, 1, 8], [-1, 0, 1], [0, 5, 6], [1, 1, 2], [0, 1, 7]], np.int32)
    up = np.nextafter(F32(2), F32(3))
    q = np.array([r[0] for r in rows] + [[0.5, 0, 1],                           # above the edge ab of triangle 0 and of its copy
                 [0.25, 0.25, 2], [0.25, 0.25, up],                            # exactly at max_distance (inside), one ulp beyond (far)
                 [nan, 0, 0], [0, inf, 0], [0, 0, -inf], [1e9, 0, 0], [0, 0, -1e9]], dtype=F32)
    loc, got, want = check(v, tris, q, 2.0, 0.5, "planted")
    c = loc.counts
    assert (c["indexed"] + c["large"], c["degenerate"], c["skipped"], c["bad_index"], c["status"]) == (2, 2, 2, 2, _lib.MESH_STATUS_BAD_INDEX)
    g = got.cpu()
    n = len(rows)
    assert g.triangle.numpy()[:n].tolist() == [0 if r[4] <= 4.0 else -1 for r in rows]
    assert np.array_equal(g.point.numpy()[:n], np.array([r[2] for r in rows], dtype=F32))
    assert np.array_equal(g.barycentric.numpy()[:n], np.array([r[3] for r in rows], dtype=F32))
    assert np.array_equal(g.d2.numpy()[:n], np.array([r[4] for r in rows], dtype=F32))
    assert g.triangle.numpy()[n:].tolist() == [0, 0, -1, -1, -1, -1, -1, -1]
    assert got.counts == dict(found=n + 2, far=1, bad_point=5, status=0)
    # equidistant from two triangles over their shared edge, and on it: the lower index, whichever of the two comes first
    tie = np.array([[0.5, 0, 1], [0.25, 0, 0]], dtype=F32)
    for t2 in ([[0, 1, 2], [0, 1, 3]], [[0, 1, 3], [0, 1, 2]], [[1, 2, 0], [0, 1, 2], [0, 1, 3]]):
        _, got, _ = check(TRI_V, np.array(t2, np.int32), tie, 10.0, 0.5, f"tie {t2}")
        assert got.cpu().triangle.tolist() == [0, 0] and got.cpu().d2.tolist() == [1.0, 0.0]


# ---- the slack: a translated soup, queries on cell borders -------------------------------------------------------------------------------
SHIFT = np.array([1000.0, -3000.5, 0.0])


FACTORS = (1.0, 0.37, 2.9)


def translated_soup():
    """3,000 small triangles in a unit cube moved to where a float32 ulp is 6e-5 / 2.4e-4 — a good part of the slack — and 4,097 queries: a third
    on the COMPUTED edges fl(j c) of the cells of each of the three cell sizes the soup is searched with (a third of them each; on the edge and
    one and two ulps to either side, on one, two or three axes), a third halfway between the centroid of a triangle and that of its NEAREST
    neighbour (two candidates at nearly the same distance, often in different cells), the rest uniform, some beyond max_distance.
    tests/closest_slack.py has the cases that are built to break a search without margins."""
    rng = np.random.default_rng(23)
    K, N, cell = 3000, 4097, 0.05
    centre = rng.uniform(0, 1, size=(K, 1, 3))
    v = (SHIFT + centre + rng.normal(size=(K, 3, 3)) * 0.012).astype(F32).reshape(-1, 3)
    tris = np.arange(3 * K, dtype=np.int32).reshape(K, 3)
    q = (SHIFT + rng.uniform(-0.1, 1.1, size=(N, 3))).astype(F32)
    n1 = N // 3
    on = rng.random((n1, 3)) < 0.6
    ulps = rng.integers(-2, 3, size=(n1, 3))
    for g, factor in enumerate(FACTORS):
        rows = slice(g * n1 // 3, (g + 1) * n1 // 3)
        c = F32(cell * factor)
        edge = np.floor(q[rows] * (F32(1) / c)) * c                             # float32: the edge as the kernel computes it
        assert edge.dtype == F32
        q[rows] = np.where(on[rows], edge, q[rows])
    for s in (-2, -1, 1, 2):
        step = q[:n1].copy()
        for _ in range(abs(s)):
            step = np.nextafter(step, F32(np.inf if s > 0 else -np.inf))
        q[:n1] = np.where(on & (ulps == s), step, q[:n1])
    cen = centre[:, 0]
    d = ((cen[:, None, :] - cen[None, :, :]) ** 2).sum(axis=2)
    np.fill_diagonal(d, np.inf)
    i = rng.integers(0, K, size=n1)
    q[n1:2 * n1] = ((cen[i] + cen[np.argmin(d[i], axis=1)]) / 2 + SHIFT).astype(F32)
    return v, tris, q, cell


@pytest.fixture(scope="module")
def soup():
    v, tris, q, cell = translated_soup()
    want = R.closest(v, tris, q, 0.12, cell)
    assert want["counts"][0] > 3000 and want["counts"][1] > 20 and want["counts"][2] == 0
    return v, tris, q, cell, want


@pytest.mark.parametrize("factor", FACTORS)
def test_translated_soup(soup, factor):
    v, tris, q, cell, want = soup
    loc, got, _ = check(v, tris, q, 0.12, cell * factor, f"soup, cell {cell * factor}", want)
    print(f"soup, cell {cell * factor:.4f}: {loc.counts}; {got.counts}")
    assert loc.counts["indexed"] > 0 and loc.counts["pairs"] > loc.counts["indexed"]


@pytest.mark.parametrize("factor", FACTORS)
def test_planted_slack_cases(factor):
    """The cases that a search without its margins answers wrongly (proved on the CPU: tests/test_closest_cpu.py), built for this cell."""
    cell = 0.05 * factor
    v, tris, q = K.planted_cases(cell)
    loc, got, want = check(v, tris, q, 2.4 * cell, cell, f"planted slack cases, cell {cell}")
    assert got.counts["found"] == q.shape[0] >= 40 and loc.counts["cell"] == float(F32(cell))


def test_soup_with_stride_six_and_small_capacity(soup):
    v, tris, q, cell, want = soup
    q6 = np.concatenate([q, np.full_like(q, np.nan)], axis=1)
    loc = M.locator(dev(v), dev(tris), cell, pair_capacity=1)                     # the wrapper retries with the exact number
    assert_build(loc, v, tris, "capacity 1")
    assert loc.args.pair_capacity == loc.counts["pairs"] and loc.counts["status"] == 0
    assert_same(loc.closest(dev(q6), 0.12), want, "stride 6 on the retried locator")
    assert_same(loc.closest(dev(q6)[:, :3].contiguous(), 0.12), want, "packed")
    # the flat C call alone reports the overflow and the pairs needed
    lib = _lib.load()
    args = M.locator_args(cell, 1)
    ws = torch.empty((int(lib.dif_mesh_locator_workspace_bytes(v.shape[0], tris.shape[0], 1)),), dtype=torch.uint8, device=DEV)
    counts = torch.empty((_lib.LOCATOR_COUNT,), dtype=torch.int32, device=DEV)
    tv, tt = dev(v), dev(tris)
    assert lib.dif_mesh_locator_build(_lib.ptr(tv), _lib.ptr(tt), v.shape[0], tris.shape[0], ctypes.byref(args), _lib.ptr(ws), ws.numel(), _lib.ptr(counts),
                                      _lib.stream_ptr()) == 0
    c = counts.cpu().tolist()
    assert c[_lib.LOCATOR_STATUS] == _lib.MESH_STATUS_PAIR_OVERFLOW and c[_lib.LOCATOR_PAIRS] == loc.counts["pairs"] and c[_lib.LOCATOR_CELLS] == 0
    with pytest.raises(RuntimeError, match="not built"):
        M.MeshLocator(ws, args, tris.shape[0], {}).closest(dev(q[:5]), 0.12)


# ---- the large list beside the grid ----------------------------------------------------------------------------------------------------
def test_one_scene_sized_triangle_among_small_ones():
    rng = np.random.default_rng(31)
    K = 2000
    centre = rng.uniform(-1, 1, size=(K, 1, 3))
    small = (centre + rng.normal(size=(K, 3, 3)) * 0.02).astype(F32).reshape(-1, 3)
    v = np.concatenate([small, np.array([[-3, -3, 0.1], [3, -3, 0.1], [0, 4, -0.2]], F32)])
    tris = np.concatenate([np.arange(3 * K, dtype=np.int32).reshape(K, 3), [[3 * K, 3 * K + 1, 3 * K + 2]]]).astype(np.int32)
    q = rng.uniform(-1.2, 1.2, size=(1500, 3)).astype(F32)
    loc, got, want = check(v, tris, q, 0.5, 0.08, "large list")
    assert loc.counts["large"] == 1 and loc.counts["indexed"] == K
    share = float((want["triangle"] == K).mean())
    print(f"large list: {share:.3f} of the queries are closest to the large triangle; {loc.counts}")
    assert 0.05 < share < 0.95 and want["counts"][1] == 0


# ---- sizes -----------------------------------------------------------------------------------------------------------------------------
def test_empty_and_single():
    v, tris = S.tetrahedron()
    q = np.array([[0.2, 0.2, 0.2], [5, 5, 5]], F32)
    for n in (0, 1, 2):
        check(v, tris, q[:n], 1.0, None, f"N = {n}")
    _, got, _ = check(v, np.zeros((0, 3), np.int32), q, 1.0, None, "K = 0")
    assert got.counts == dict(found=0, far=2, bad_point=0, status=0)
    _, got, _ = check(np.zeros((0, 3), F32), np.zeros((0, 3), np.int32), q, 1.0, None, "V = K = 0")
    assert got.counts["far"] == 2
    loc, got, _ = check(np.zeros((0, 3), F32), tris, q, 1.0, 0.5, "V = 0")
    assert loc.counts["bad_index"] == 4 and loc.counts["status"] == _lib.MESH_STATUS_BAD_INDEX and got.counts["far"] == 2


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_every_refusal():
    v, tris = S.tetrahedron()
    tv, tt, q = dev(v), dev(tris), dev(np.zeros((3, 3), F32))
    for cell in (0.0, -1.0, float("nan"), float("inf"), 1e-50):
        with pytest.raises(ValueError):
            M.locator(tv, tt, cell)
    with pytest.raises(ValueError):
        M.locator(tv, tt, 0.5, pair_capacity=0)
    with pytest.raises(RuntimeError):
        M.locator(torch.from_numpy(v), tt)                                        # a host tensor
    with pytest.raises(RuntimeError):
        M.locator(tv.double(), tt)
    with pytest.raises(RuntimeError):
        M.locator(tv, tt.long())
    with pytest.raises(RuntimeError):
        M.locator(tv[:, :2].contiguous(), tt)
    with pytest.raises(RuntimeError):
        M.locator(tv, tt, 0.5, pair_capacity=2 ** 28)
    loc = M.locator(tv, tt, 0.5)
    for r in (0.0, -1.0, float("nan"), float("inf"), 0.5 * 60.001):
        with pytest.raises(ValueError):
            loc.closest(q, r)
    assert loc.closest(q, 0.5 * 60).counts["found"] == 3                        # the ring limit itself is served
    with pytest.raises(RuntimeError):
        loc.closest(q.cpu(), 1.0)
    with pytest.raises(RuntimeError):
        loc.closest(q.double(), 1.0)
    with pytest.raises(RuntimeError):
        loc.closest(q[:, :2].contiguous(), 1.0)
    with pytest.raises(RuntimeError):
        loc.closest(q.reshape(-1), 1.0)
    # the C entry points
    lib = _lib.load()
    assert lib.dif_mesh_locator_workspace_bytes(4, (2 ** 31 + 2) // 3, 8) == -1 and lib.dif_mesh_locator_workspace_bytes(2 ** 31, 4, 8) == -1
    assert lib.dif_mesh_locator_workspace_bytes(4, 4, 2 ** 31) == -1 and lib.dif_mesh_locator_workspace_bytes(4, 4, 0) == -1
    assert lib.dif_mesh_locator_workspace_bytes(-1, 4, 8) == -1 and lib.dif_mesh_locator_workspace_bytes(0, 0, 1) > 0
    counts = torch.zeros((8,), dtype=torch.int32, device=DEV)
    out = [torch.empty((3,), dtype=torch.float32, device=DEV), torch.empty((3,), dtype=torch.int32, device=DEV),
           torch.empty((3, 3), dtype=torch.float32, device=DEV), torch.empty((3, 3), dtype=torch.float32, device=DEV)]
    P, ws, a = _lib.ptr, loc.workspace, loc.args

    def build(args=a, wsp=None, nbytes=None, v_=tv, t_=tt, c_=counts):
        return lib.dif_mesh_locator_build(P(v_), P(t_), 4, 4, ctypes.byref(args) if args is not None else None, P(ws) if wsp is None else wsp,
                                          ws.numel() if nbytes is None else nbytes, P(c_), _lib.stream_ptr())

    def query(args=a, wsp=None, nbytes=None, r=1.0, stride=3, pts=q, o=out, c_=counts, n=3):
        return lib.dif_mesh_closest(ctypes.byref(args) if args is not None else None, 4, P(ws) if wsp is None else wsp, ws.numel() if nbytes is None else nbytes,
                                    P(pts), n, stride, r, P(o[0]), P(o[1]), P(o[2]), P(o[3]), P(c_), _lib.stream_ptr())

    bad_cell, many = _lib.DifLocatorArgs(0.0, 0, a.pair_capacity), _lib.DifLocatorArgs(0.5, 2 ** 20 + 1, a.pair_capacity)
    assert build() == 0 and query() == 0
    for rc in (build(args=None), build(args=bad_cell), build(args=many), build(wsp=ctypes.c_void_p(0)), build(wsp=ctypes.c_void_p(ws.data_ptr() + 8)),
               build(nbytes=ws.numel() - 1), build(v_=None), build(t_=None), build(c_=None),
               query(args=None), query(args=bad_cell), query(wsp=ctypes.c_void_p(0)), query(nbytes=ws.numel() - 1), query(r=0.0), query(r=float("inf")),
               query(r=31.0), query(stride=2), query(pts=None), query(c_=None), query(n=-1), query(o=[None, out[1], out[2], out[3]]),
               query(o=[out[0], None, out[2], out[3]]), query(o=[out[0], out[1], None, out[3]]), query(o=[out[0], out[1], out[2], None])):
        assert rc == -1
    torch.cuda.synchronize()


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


def stats_of(d2):
    d = np.sqrt(d2[np.isfinite(d2)]).astype(np.float64)
    return dict(mean=d.mean(), rms=np.sqrt((d * d).mean()), max=d.max(), median=np.sort(d)[(d.size - 1) // 2])      # (torch's median: the lower middle)


def test_through_the_map(two_sphere_map):
    full = two_sphere_map.indexed_mesh(min_component_triangles=500)           # the two spheres without the fragments beside them: those collapse as a whole
    step = F32(W.SPHERE_VOXEL) / F32(W.SPHERE_RES)
    c = 4.0 * float(step)
    small = full.simplify(c, tuple(float(F32(-W.SPHERE_BOUND) - step / F32(2)) for _ in range(3)))      # the grid `indexed_mesh(simplify_cell=c)` uses
    assert 0 < small.counts["vertices"] < full.counts["vertices"] // 8
    f, s = full.cpu(), small.cpu()
    fv, ft, sv, st = f.vertices.numpy(), f.triangles.numpy(), s.vertices.numpy(), s.triangles.numpy()
    r = 2.0 * c
    for name, a, b, av, bv, bt in (("simplified -> full", small, full, sv, fv, ft), ("full -> simplified", full, small, fv, sv, st)):
        want = R.closest(bv, bt, av, r, R.default_cell(bv, bt))
        assert want["counts"][1:] == [0, 0, 0], (name, want["counts"])              # the reference alone: nothing is farther than two cells
        got = a.distance_to(b, r)
        assert got["d2"].cpu().numpy().tobytes() == want["d2"].tobytes() and got["far"] == 0 and got["found"] == av.shape[0], name
        ws = stats_of(want["d2"])
        print(f"{name}: {av.shape[0]} vertices against {bt.shape[0]} triangles, cell {c}: " + ", ".join(f"{k} {got[k]:.6f}" for k in ws))
        for k in ws:                                                              # (the device's float32 sqrt may be an ulp off the correctly rounded one)
            assert abs(got[k] - ws[k]) <= 2.0 ** -22 * ws[k] + 1e-12, (name, k, got[k], ws[k])
        if a is small:
            assert got["max"] <= np.sqrt(3.0) * c                                  # a cluster mean lies within sqrt(3) cell of each member
    # a max_distance far beyond 60 default cells: distance_to picks a cell that serves it, and no answer depends on the cell
    assert small.distance_to(full, 100.0)["d2"].cpu().numpy().tobytes() == small.distance_to(full, r)["d2"].cpu().numpy().tobytes()
    with pytest.raises(ValueError):
        small.distance_to(full, 100.0, cell=0.1)
    # the unfiltered mesh, the public route: its fragments collapse as a whole, so some of its vertices have nothing of the simplified surface
    # within two cells — how many is the restatement's to say
    whole = two_sphere_map.indexed_mesh()
    lean = whole.simplify(c, small.counts["origin"])
    w, l = whole.cpu(), lean.cpu()
    for name, a, b, av, bv, bt in (("simplified -> whole", lean, whole, l.vertices.numpy(), w.vertices.numpy(), w.triangles.numpy()),
                                   ("whole -> simplified", whole, lean, w.vertices.numpy(), l.vertices.numpy(), l.triangles.numpy())):
        want = R.closest(bv, bt, av, r, R.default_cell(bv, bt))
        got = a.distance_to(b, r)
        print(f"{name}: {av.shape[0]} vertices against {bt.shape[0]} triangles: found {got['found']}, far {got['far']}")
        assert got["d2"].cpu().numpy().tobytes() == want["d2"].tobytes() and [got["found"], got["far"]] == want["counts"][:2], name
    # std carried from the full mesh to the simplified one's vertices
    cl = full.closest(small.vertices, r)
    want = R.closest(fv, ft, sv, r, R.default_cell(fv, ft))
    assert_same(cl, want, "closest through the mesh")
    std = full.interpolate(cl, full.vertex_std).cpu().numpy()
    b, x = want["barycentric"], f.vertex_std.numpy()[ft[want["triangle"]]]
    assert std.tobytes() == ((b[:, 0] * x[:, 0] + b[:, 1] * x[:, 1]) + b[:, 2] * x[:, 2]).astype(F32).tobytes()
    nrm = full.interpolate(cl, full.normals)
    assert tuple(nrm.shape) == (sv.shape[0], 3) and bool(torch.isfinite(nrm).all())
