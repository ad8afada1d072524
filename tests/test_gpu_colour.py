"""GPU: `dif_mesh_colour_view` and `dif_mesh_colour_resolve` against their numpy restatement (tests/colour_ref.py), BIT FOR BIT — the
accumulators as uint64, every count, the resolved colours as bytes and the weights as bits; no tolerance anywhere, because everything that is
summed is an integer — on small overlapping triangles around the wave boundaries with every gate alone and together, the cooperative path of
the rasteriser, shared edges and fans, a closed surface, the image borders, bad pixels, bad indices, accumulation over views, empty and
refused calls, the rasteriser on the same workspace; then through `DenseIndexedMap.coloured_mesh` on the two-sphere scene of
tests/test_gpu_components.py."""
import ctypes

import numpy as np
import pytest
import torch

from di_fusion_amd import _lib, synthetic as syn
from di_fusion_amd.system import mesh as M
from di_fusion_amd.system.map import DenseIndexedMap
from tests import colour_ref as C
from tests import components_ref as CR
from tests import raster_ref as R
from tests import weld_ref as W

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F32, F64 = np.float32, np.float64
IMAGES = {"64x48": (48, 64, (60.0, 57.5, 31.37, 23.81)), "37x29": (29, 37, (41.25, 43.5, 17.6, 14.3)),        # H, W, (fx, fy, cx, cy)
          "centred": (48, 64, (60.0, 60.0, 32.0, 24.0))}
GATES = {"off": dict(depth_tol=0.02, min_cos=0.0, edge_gate=False), "edge": dict(depth_tol=0.02, min_cos=0.0, edge_gate=True),
         "grazing": dict(depth_tol=0.02, min_cos=0.3, edge_gate=False), "all": dict(depth_tol=0.02, min_cos=0.3, edge_gate=True)}


def turned_pose():
    a, b = 0.31, -0.17
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    P = np.eye(4)
    P[:3, :3], P[:3, 3] = Rx @ Ry, (0.23, -0.41, 0.37)
    return P


def pose_at(x, y, z, turn=0.0):
    P = np.eye(4)
    P[:3, :3] = np.array([[np.cos(turn), 0, np.sin(turn)], [0, 1, 0], [-np.sin(turn), 0, np.cos(turn)]])
    P[:3, 3] = (x, y, z)
    return P


POSES = {"identity": np.eye(4), "turned": turned_pose(), "front": pose_at(0.0, 0.0, -2.0), "side": pose_at(-0.9, 0.1, -1.7, turn=0.45),
         "close": pose_at(0.0, 0.0, -0.75)}


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def check_resolve(accum_dev, accum_ref, what, min_weights=(0.0,)):
    for mw in min_weights:
        colors, weight, n = M.colour_resolve(accum_dev, mw)
        rgb8, w, coloured = C.resolve(accum_ref, C.weight_units(mw))
        assert colors.dtype == torch.uint8 and weight.dtype == torch.float32
        assert n == coloured, (what, mw, n, coloured)
        assert same_bits(colors.cpu().numpy(), rgb8), (what, mw, "rgb8")
        assert same_bits(weight.cpu().numpy(), w), (what, mw, "weight")


def check(mesh, pose, image, rgb, what, depth_in=None, accum=None, z_near=0.05, cull=False, gates="all", resolve=True):
    """the flat operators on the GPU == the restatement: accumulators, counts, resolved colours.  `mesh` = (vertices, normals, triangles),
    `accum` = (device tensor, numpy) to add to, or None for zeroed ones.  Returns (device accumulator, the restatement's dict)."""
    H, Wd, intr = IMAGES[image] if isinstance(image, str) else image
    g = GATES[gates] if isinstance(gates, str) else gates
    v, n, t = (np.ascontiguousarray(a) for a in mesh)
    before = None if accum is None else accum[1]
    want = C.colour_view(v, n, t, R.world_to_cam(pose), intr, rgb, depth_in=depth_in, depth_tol=g["depth_tol"], min_cos2=C.min_cos2(g["min_cos"]),
                         edge_gate=g["edge_gate"], z_near=z_near, cull_backfaces=cull, accum=before)
    acc = M.colour_accumulator(v.shape[0], DEV) if accum is None else accum[0]
    counts = M.colour_view(dev(v), dev(n), dev(t), acc, dev(rgb), pose, intr, depth=dev(depth_in), z_near=z_near, cull_backfaces=cull, gates=M.colour_args(**g))
    assert counts == want["counts"], (what, counts, want["counts"])
    assert sum(counts[k] for k in C.COUNT_NAMES[:6]) == H * Wd
    got = acc.cpu().numpy()
    if not same_bits(got, want["accum"]):
        bad = np.argwhere(got != want["accum"])
        raise AssertionError(f"{what}: the accumulators differ at {len(bad)} places, first {bad[0].tolist()}: {got[tuple(bad[0])]} != {want['accum'][tuple(bad[0])]}")
    if resolve:
        check_resolve(acc, want["accum"], what)
    return acc, want


def concat(*meshes):
    """several (v, n, t) as one mesh"""
    off, out = 0, [[], [], []]
    for v, n, t in meshes:
        for k, a in enumerate((v, n, np.where(t >= 0, t + off, t).astype(np.int32))):
            out[k].append(a)
        off += v.shape[0]
    return tuple(np.concatenate(a) for a in out)


def screen_mesh(pose, image, uv, z, tris, seed=0):
    """vertices given by pixel position and depth, random unit normals"""
    intr = IMAGES[image][2]
    v = R.plane_points(R.world_to_cam(pose), intr, np.asarray(uv, dtype=F64), np.asarray(z, dtype=F64)).astype(F32)
    return v, R.flat_attributes(v.shape[0], seed)[0], np.asarray(tris, dtype=np.int32).reshape(-1, 3)


def small(K, pose, image, seed, depth=(0.6, 3.0)):
    H, Wd, intr = IMAGES[image]
    v, n, _, t = R.small_triangles(K, R.world_to_cam(POSES[pose]), intr, H, Wd, seed=seed, depth=depth)
    return v, n, t


def planted_depth(depth, tol, seed):
    """the rendered depth with NaN, +inf and +-2 tol planted at hit pixels (and a value where nothing was hit)"""
    rng = np.random.default_rng(seed)
    d = depth.copy()
    jj, ii = np.nonzero(np.isfinite(depth))
    pick = rng.permutation(len(jj))[:40]
    for k, p in enumerate(pick):
        d[jj[p], ii[p]] = (np.nan, np.inf, depth[jj[p], ii[p]] + F32(2 * tol), depth[jj[p], ii[p]] - F32(2 * tol))[k % 4]
    empty = np.argwhere(np.isnan(depth))
    if len(empty):
        d[tuple(empty[0])] = 1.0
    return d, len(pick)


# ---- small triangles -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("image,pose", [("64x48", "turned"), ("37x29", "identity")])
def test_small_triangles_under_every_gate(image, pose):
    H, Wd, intr = IMAGES[image]
    mesh = small(2000, pose, image, seed=2000)
    rgb = C.random_rgb(H, Wd, 1)
    P = POSES[pose]
    _, free = check(mesh, P, image, rgb, f"{image} gates off", gates="off")
    hit = free["render"]["counts"]["pixels_hit"]
    assert free["counts"]["used"] == hit > 500 and free["render"]["coverage"].max() >= 3
    d, planted = planted_depth(free["render"]["depth"], 0.02, 3)
    _, gated = check(mesh, P, image, rgb, f"{image} depth gate", depth_in=d, gates="off")
    assert gated["counts"]["depth"] == planted and gated["counts"]["used"] == hit - planted
    _, e = check(mesh, P, image, rgb, f"{image} edge gate", gates="edge")
    _, g = check(mesh, P, image, rgb, f"{image} grazing gate", gates="grazing")
    _, a = check(mesh, P, image, rgb, f"{image} every gate", depth_in=d, gates="all")
    assert e["counts"]["edge"] > hit // 2 and 0 < g["counts"]["grazing"] < hit and g["counts"]["used"] > 100
    assert a["counts"]["depth"] == planted and a["counts"]["edge"] > 0
    print(f"{image}: off {free['counts']}, depth {gated['counts']}, edge {e['counts']}, grazing {g['counts']}, all {a['counts']}")


# ---- the cooperative path ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("image,pose", [("64x48", "turned"), ("37x29", "identity")])
def test_a_large_triangle_feeds_the_splat(image, pose):
    H, Wd, intr = IMAGES[image]
    P = POSES[pose]
    big = screen_mesh(P, image, [(-40.0, -30.0), (3.0 * Wd, -25.0), (-35.0, 3.0 * H)], [1.4, 1.9, 1.6], [[0, 1, 2]])
    mesh = concat(small(150, pose, image, 1, depth=(0.5, 1.0)), big, small(150, pose, image, 2, depth=(2.5, 3.0)))
    rgb = C.random_rgb(H, Wd, 4)
    _, want = check(mesh, P, image, rgb, f"large triangle, {image}", gates="off")
    assert want["render"]["counts"]["large"] == 1 and want["counts"]["used"] == H * Wd
    S = want["accum"][:, 3]
    assert (S[450:453] > 0).all() and not S[453:].any()                          # the large one received; nothing behind it did
    _, want = check(mesh, P, image, rgb, f"large triangle, every gate, {image}", depth_in=want["render"]["depth"], gates="all")
    assert want["counts"]["used"] > 0 and want["counts"]["edge"] > 0


# ---- shared edges ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("image,pose", [("64x48", "turned"), ("37x29", "identity")])
def test_a_pixel_on_a_shared_edge_is_splat_once(image, pose):
    H, Wd, intr = IMAGES[image]
    w2c = R.world_to_cam(POSES[pose])
    rgb = C.random_rgb(H, Wd, 5)
    for name, (v, t) in (("shared edge", R.shared_edge_pair(w2c, intr)), ("fan", R.vertex_fan(w2c, intr))):
        n = np.tile(-w2c.reshape(3, 4)[2, :3], (v.shape[0], 1)).astype(F32)      # along the optical axis: no pixel is grazing
        acc, want = check((v, n, t), POSES[pose], image, rgb, f"{name}, {image}", gates="grazing")
        assert want["render"]["coverage"].max() == 1 and want["counts"]["used"] == int(want["render"]["coverage"].sum()) > 200
        # once, to its owner: the weights of a pixel go to the triangle its pixel names and sum to cos^2 (three roundings)
        used = want["classes"] == C.USED
        total = want["weights"][used].sum(axis=1).astype(np.int64)
        assert (np.abs(total - want["cos2"][used] * 65536.0) <= 1.5 + 1e-9).all()
        assert int(acc.cpu().numpy()[:, 3].sum()) == int(total.sum())


# ---- a closed surface --------------------------------------------------------------------------------------------------------------------
def test_hidden_vertices_of_a_closed_surface_receive_nothing():
    v, n, _, t = R.icosphere(3)
    H, Wd, intr = IMAGES["centred"]
    rgb = C.random_rgb(H, Wd, 6)
    for gates in ("off", "all"):
        acc, want = check((v, n, t), POSES["front"], "centred", rgb, f"icosphere, gates {gates}", gates=gates)
        got = acc.cpu().numpy()
        back = v[:, 2] > 0.1                                                     # the camera sits on the negative z axis
        front = got[v[:, 2] < -0.3, 3] > 0
        assert back.sum() > v.shape[0] // 3 and not got[back].any() and (front.all() if gates == "off" else front.sum() > len(front) // 2)
        assert want["counts"]["used"] > 200
    assert want["counts"]["edge"] > 20                                           # (towards the limb the depth falls by more than 2 cm a pixel)
    # a small sphere in front of a large one: the edge gate takes the pixels on both sides of the step
    v, n, t, _ = C.two_spheres(2)
    _, on = check((v, n, t), POSES["front"], "centred", rgb, "two spheres, edge gate", gates=dict(depth_tol=0.05, min_cos=0.0, edge_gate=True))
    _, off = check((v, n, t), POSES["front"], "centred", rgb, "two spheres, no gate", gates=dict(depth_tol=0.05, min_cos=0.0, edge_gate=False))
    assert on["counts"]["edge"] > 40 and on["counts"]["used"] + on["counts"]["edge"] == off["counts"]["used"]


# ---- borders -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("image,pose", [("64x48", "turned"), ("37x29", "identity")])
def test_image_borders(image, pose):
    H, Wd, intr = IMAGES[image]
    P = POSES[pose]
    over = [[(-3.2, 10.1), (2.7, 8.3), (1.1, 14.9)], [(Wd - 2.5, 5.5), (Wd + 4.1, 7.2), (Wd - 1.2, 12.8)],
            [(10.3, -2.9), (16.8, -1.1), (12.2, 3.4)], [(8.1, H - 3.3), (15.6, H - 1.4), (11.9, H + 3.8)],
            [(-2.4, -1.7), (3.9, -2.2), (-1.3, 4.6)], [(Wd - 2.2, H - 2.6), (Wd + 3.0, H - 1.0), (Wd - 1.5, H + 2.1)]]
    uv = np.array(over, dtype=F64).reshape(-1, 2)
    edge_on = dict(depth_tol=0.02, min_cos=0.0, edge_gate=True)
    straddling = screen_mesh(P, image, uv, np.full(len(uv), 1.25), np.arange(len(uv)).reshape(-1, 3), seed=3)
    rgb = C.random_rgb(H, Wd, 7)
    _, want = check(straddling, P, image, rgb, f"borders, {image}", gates="off")
    assert want["render"]["counts"]["drawn"] == 6 and all(want["classes"][j, i] == C.USED for j, i in ((0, 0), (H - 1, Wd - 1)))
    check(straddling, P, image, rgb, f"borders, edge gate, {image}", gates=edge_on)
    # behind them one triangle over the whole image, at one depth: a border pixel has no neighbour outside the image, so nothing in the
    # background is an edge pixel but the ring around the six triangles in front of it
    back = screen_mesh(P, image, [(-40.0, -30.0), (3.0 * Wd, -25.0), (-35.0, 3.0 * H)], [2.0, 2.0, 2.0], [[0, 1, 2]])
    _, alone = check(back, P, image, rgb, f"a plane to the borders, {image}", gates=edge_on)
    assert alone["counts"]["used"] == H * Wd and alone["counts"]["edge"] == 0
    _, both = check(concat(straddling, back), P, image, rgb, f"borders over a plane, {image}", gates=edge_on)
    cls = both["classes"]
    assert both["counts"]["no_hit"] == 0 and both["counts"]["edge"] > 20 and cls[0, Wd // 2 + 10] == C.USED and cls[H // 2 + 8, Wd - 1] == C.USED


# ---- bad pixels, bad indices -------------------------------------------------------------------------------------------------------------
def test_bad_pixels_are_counted_and_send_nothing():
    image, P = "centred", POSES["front"]
    H, Wd, intr = IMAGES[image]
    v, n, _, t = R.icosphere(2)
    rgb = C.random_rgb(H, Wd, 8)
    _, clean = check((v, n, t), P, image, rgb, "clean", gates="off")
    d = clean["render"]["depth"].copy()
    bad = rgb.copy()
    bad[20:24, 30:34, 0] = np.nan
    bad[24, 30:34, 1] = np.inf
    bad[25, 30:34, 2] = -np.inf
    bad[0, 0] = np.nan                                                           # nothing is hit there: NO_HIT comes first
    d[26, 30:34] = np.nan
    d[27, 30:34] = -np.inf
    d[20, 30] = np.nan                                                           # the colour is bad there too: BAD_COLOUR comes first
    acc, want = check((v, n, t), P, image, bad, "bad pixels", depth_in=d, gates="off")
    assert want["counts"]["bad_colour"] == 24 and want["counts"]["depth"] == 8 and want["counts"]["used"] == clean["counts"]["used"] - 32
    assert want["counts"]["no_hit"] == clean["counts"]["no_hit"]
    # what the bad pixels would have sent is missing, nothing else: the same as a run over an image in which they hit nothing
    got = acc.cpu().numpy()
    assert (got <= clean["accum"]).all() and int(clean["accum"][:, 3].sum()) - int(got[:, 3].sum()) == int(clean["weights"][20:28, 30:34].sum())


def test_bad_indices_are_reported_and_never_followed():
    """The index V: the words past the end of a (V,3) array lie inside the same allocation, so a missing check shows as a wrong answer,
    never as a fault."""
    P, image = POSES["turned"], "64x48"
    H, Wd, intr = IMAGES[image]
    v, n, t = small(40, "turned", image, seed=9)
    V = v.shape[0]
    rgb = C.random_rgb(H, Wd, 9)
    _, rest = check((v, n, t), P, image, rgb, "without the bad ones", gates="grazing")
    tb = np.concatenate([t, [[7, V, 8]], [[0, 1, -1]], [[V + 5, 2, 3]]]).astype(np.int32)
    acc, want = check((v, n, tb), P, image, rgb, "index V, -1 and V + 5", gates="grazing")
    assert want["counts"]["status"] == _lib.MESH_STATUS_BAD_INDEX and rest["counts"]["status"] == 0
    assert {k: c for k, c in want["counts"].items() if k != "status"} == {k: c for k, c in rest["counts"].items() if k != "status"}
    assert same_bits(acc.cpu().numpy(), rest["accum"]) and rest["counts"]["used"] > 30
    _, none = check((v[:0], n[:0], np.array([[0, 1, 2]], dtype=np.int32)), P, image, rgb, "no vertices at all")
    assert none["counts"]["no_hit"] == H * Wd and none["counts"]["status"] == _lib.MESH_STATUS_BAD_INDEX


# ---- accumulation ------------------------------------------------------------------------------------------------------------------------
def test_views_add_up():
    image = "centred"
    H, Wd, intr = IMAGES[image]
    v, n, t, _ = C.two_spheres(2)
    a, b = C.random_rgb(H, Wd, 10), C.random_rgb(H, Wd, 11)
    acc, first = check((v, n, t), POSES["front"], image, a, "first view")
    alone = acc.cpu().numpy().copy()
    acc, both = check((v, n, t), POSES["side"], image, b, "second view on top", accum=(acc, first["accum"]))
    assert (both["accum"][:, 3] > first["accum"][:, 3]).any()
    # the other way round, and the same view twice
    acc2, second = check((v, n, t), POSES["side"], image, b, "second view alone")
    acc2, ba = check((v, n, t), POSES["front"], image, a, "first view on top", accum=(acc2, second["accum"]))
    assert same_bits(acc.cpu().numpy(), acc2.cpu().numpy()) and same_bits(both["accum"], ba["accum"])
    acc3, _ = check((v, n, t), POSES["front"], image, a, "first view again")
    acc3, twice = check((v, n, t), POSES["front"], image, a, "the same view twice", accum=(acc3, first["accum"]))
    assert same_bits(acc3.cpu().numpy(), 2 * alone) and alone[:, 3].any()
    # two runs of 2000 small triangles (deep stacks, every atomic contended) are bit-identical
    mesh = small(2000, "turned", "64x48", seed=21)
    rgb = C.random_rgb(48, 64, 12)
    d = [dev(x) for x in mesh]
    runs = []
    for _ in range(2):
        acc = M.colour_accumulator(mesh[0].shape[0], DEV)
        c = M.colour_view(*d, acc, dev(rgb), POSES["turned"], IMAGES["64x48"][2], gates=M.colour_args(0.02, 0.0, False))
        runs.append((c, acc.cpu().numpy()))
    assert runs[0][0] == runs[1][0] and same_bits(runs[0][1], runs[1][1]) and runs[0][1].any()


def test_the_colourer_of_a_mesh():
    image = "centred"
    H, Wd, intr = IMAGES[image]
    v, n, s, t = R.icosphere(2)
    mesh = M.IndexedMesh(dev(v), dev(n), dev(s), dev(t), torch.arange(t.shape[0], dtype=torch.int64, device=DEV), dict(vertices=v.shape[0], triangles=t.shape[0]))
    col = mesh.colourer()
    assert col.views == 0 and col.accum.dtype == torch.uint64 and tuple(col.accum.shape) == (v.shape[0], 4) and not col.accum.cpu().numpy().any()
    a, b = C.random_rgb(H, Wd, 13), C.random_rgb(H, Wd, 14)
    want = C.colour_view(v, n, t, R.world_to_cam(POSES["front"]), intr, a, depth_tol=0.03, min_cos2=C.min_cos2(0.2), edge_gate=True)
    c = col.add_view(dev(a), POSES["front"], intr, depth_tol=0.03, min_cos=0.2)
    assert c == want["counts"] and col.views == 1
    depth = want["render"]["depth"]
    want2 = C.colour_view(v, n, t, R.world_to_cam(POSES["front"]), intr, b, depth_in=depth, cull_backfaces=True, accum=want["accum"])
    c = col.add_view(dev(b), POSES["front"], intr, depth=dev(depth), cull_backfaces=True)
    assert c == want2["counts"] and col.views == 2 and same_bits(col.accum.cpu().numpy(), want2["accum"])
    out = col.resolve()
    rgb8, w, coloured = C.resolve(want2["accum"])
    assert out.vertices is mesh.vertices and out.triangles is mesh.triangles and out.normals is mesh.normals and mesh.colors is None
    assert out.counts == dict(mesh.counts, coloured=coloured) and 0 < coloured < v.shape[0]
    assert same_bits(out.colors.cpu().numpy(), rgb8) and same_bits(out.color_weight.cpu().numpy(), w)
    host = out.cpu()
    assert same_bits(host.colors.numpy(), rgb8) and host.counts == out.counts
    kept = out.select(torch.ones(t.shape[0], dtype=torch.bool, device=DEV))
    assert kept.colors is None and kept.color_weight is None and out.remove_small_components(1).colors is None


# ---- resolve -----------------------------------------------------------------------------------------------------------------------------
def test_resolve_thresholds():
    acc = np.array([[0, 0, 0, 0], [10, 20, 30, 1], [255 * 65536, 0, 65536 * 127, 65536], [3, 3, 3, 2], [5, 5, 5, 2], [255 << 40, 1 << 40, 77 << 39, 1 << 40]],
                   dtype=np.uint64)
    rng = np.random.default_rng(15)
    S = rng.integers(0, 1 << 30, size=700).astype(np.uint64)                     # more than one wave, a tail
    S[rng.random(700) < 0.2] = 0
    many = np.concatenate([(rng.random((700, 3)) * 255.0 * S[:, None].astype(F64)).astype(np.uint64), S[:, None]], axis=1)      # sum_c <= 255 S
    for a in (acc, many):
        d = dev(a)
        # at, just below and just above the weight of a vertex; 0 and 1 unit are the same threshold
        check_resolve(d, a, "resolve", min_weights=(0.0, 1.0 / 65536, 2.0 / 65536, 2.5 / 65536, 3.0 / 65536, 1.0, 1.0 + 1.0 / 65536, float(1 << 24), 1e9))
    colors, weight, n = M.colour_resolve(dev(acc))
    assert n == 5 and colors.cpu().tolist()[:5] == [[128, 128, 128], [10, 20, 30], [255, 0, 127], [2, 2, 2], [3, 3, 3]] and weight.cpu().tolist()[2] == 1.0
    colors, weight, n = M.colour_resolve(M.colour_accumulator(0, DEV))
    assert n == 0 and tuple(colors.shape) == (0, 3) and tuple(weight.shape) == (0,)
    with pytest.raises(RuntimeError):
        M.colour_resolve(dev(acc.astype(np.int64)))
    with pytest.raises(RuntimeError):
        M.colour_resolve(dev(acc), -1.0)
    lib = _lib.load()
    out = [torch.empty((6, 3), dtype=torch.uint8, device=DEV), torch.empty((6,), dtype=torch.float32, device=DEV), torch.zeros((1,), dtype=torch.int32, device=DEV)]
    d = dev(acc)
    P, s = _lib.ptr, _lib.stream_ptr()
    assert lib.dif_mesh_colour_resolve(P(d), -1, 0, P(out[0]), P(out[1]), P(out[2]), s) == -1
    assert lib.dif_mesh_colour_resolve(P(d), 1 << 31, 0, P(out[0]), P(out[1]), P(out[2]), s) == -1
    assert lib.dif_mesh_colour_resolve(P(d), 6, 0, P(out[0]), P(out[1]), None, s) == -1
    assert lib.dif_mesh_colour_resolve(None, 6, 0, P(out[0]), P(out[1]), P(out[2]), s) == -1
    assert lib.dif_mesh_colour_resolve(P(d), 6, 0, None, P(out[1]), P(out[2]), s) == -1
    assert lib.dif_mesh_colour_resolve(P(d), 6, 0, P(out[0]), None, P(out[2]), s) == -1
    assert lib.dif_mesh_colour_resolve(None, 0, 0, None, None, P(out[2]), s) == 0
    torch.cuda.synchronize()
    assert out[2].cpu().tolist() == [0]


# ---- empty and refused calls -------------------------------------------------------------------------------------------------------------
def test_empty_inputs_and_a_single_pixel():
    P = POSES["identity"]
    v, n, t = screen_mesh(P, "64x48", [(6.5, 5.25), (25.2, 7.1), (14.4, 21.3)], [1.0, 1.3, 1.1], [[0, 1, 2]])
    rgb = C.random_rgb(48, 64, 16)
    _, want = check((v, n, t[:0]), P, "64x48", rgb, "no triangles")
    assert want["counts"] == dict(dict.fromkeys(C.COUNT_NAMES, 0), no_hit=48 * 64)
    _, want = check((v[:0], n[:0], t[:0]), P, "37x29", C.random_rgb(29, 37, 17), "nothing at all")
    assert want["counts"]["no_hit"] == 29 * 37
    one = (1, 1, (50.0, 50.0, 0.0, 0.0))
    pv = R.plane_points(R.world_to_cam(P), one[2], np.array([(-0.5, -0.5), (1.0, -0.25), (-0.25, 1.0)]), np.array([1.0, 1.5, 2.0])).astype(F32)
    pn = np.tile(np.array([[0.0, 0.0, -1.0]], dtype=F32), (3, 1))
    acc, want = check((pv, pn, np.array([[0, 1, 2]], dtype=np.int32)), P, one, np.array([[[0.25, 0.5, 0.75]]], dtype=F32), "1 x 1", gates="all")
    assert want["counts"]["used"] == 1 and (acc.cpu().numpy()[:, 3] > 0).all()              # a single pixel has no neighbour: no edge


def test_arguments_are_checked():
    P = POSES["identity"]
    H, Wd, intr = IMAGES["64x48"]
    v, n, t = screen_mesh(P, "64x48", [(6.5, 5.25), (25.2, 7.1), (14.4, 21.3), (20.5, 12.5), (34.0, 9.75), (27.75, 26.5)], [1.0, 1.3, 1.1, 0.9, 1.4, 1.2],
                          [[0, 1, 2], [3, 5, 4]])
    d = dict(v=dev(v), n=dev(n), t=dev(t))
    rgb = dev(C.random_rgb(H, Wd, 18))
    acc = M.colour_accumulator(6, DEV)
    with pytest.raises(RuntimeError):
        M.colour_view(torch.from_numpy(v), d["n"], d["t"], acc, rgb, P, intr)                 # host tensor
    with pytest.raises(RuntimeError):
        M.colour_view(d["v"], d["n"], d["t"], acc, rgb.cpu(), P, intr)
    with pytest.raises(RuntimeError):
        M.colour_view(d["v"], d["n"], d["t"].long(), acc, rgb, P, intr)
    with pytest.raises(RuntimeError):
        M.colour_view(d["v"], d["n"], d["t"], acc[:5], rgb, P, intr)
    with pytest.raises(RuntimeError):
        M.colour_view(d["v"], d["n"], d["t"], torch.zeros((6, 4), dtype=torch.int64, device=DEV), rgb, P, intr)
    with pytest.raises(RuntimeError):
        M.colour_view(d["v"], d["n"], d["t"], acc, rgb[:, :, :2].contiguous(), P, intr)
    with pytest.raises(RuntimeError):
        M.colour_view(d["v"], d["n"], d["t"], acc, rgb, P, intr, depth=torch.zeros((H, Wd + 1), device=DEV))
    with pytest.raises(RuntimeError, match="DIF_EINVAL"):
        M.colour_view(d["v"], d["n"], d["t"], acc, rgb, P, (0.0, 60.0, 1.0, 1.0))
    with pytest.raises(RuntimeError, match="DIF_EINVAL"):
        M.colour_view(d["v"], d["n"], d["t"], acc, rgb, P, intr, gates=M.colour_args(depth_tol=-0.01))
    with pytest.raises(RuntimeError, match="DIF_EINVAL"):
        M.colour_view(d["v"], d["n"], d["t"], acc, torch.zeros((0, Wd, 3), device=DEV), P, intr)
    # the entry point itself
    lib = _lib.load()
    assert lib.dif_mesh_colour_workspace_bytes(6, 2, 0, Wd) == -1 and lib.dif_mesh_colour_workspace_bytes(6, 2, 1 << 16, 1 << 15) == -1
    need = int(lib.dif_mesh_colour_workspace_bytes(6, 2, H, Wd))
    assert need >= int(lib.dif_mesh_render_workspace_bytes(6, 2, H, Wd))
    ws = torch.empty((need + 16,), dtype=torch.uint8, device=DEV)
    counts = torch.full((_lib.COLOUR_COUNT,), -7, dtype=torch.int32, device=DEV)
    ok = dict(vertices=d["v"], normals=d["n"], triangles=d["t"], V=6, K=2, view=M.raster_args(P, intr, H, Wd), gates=M.colour_args(), rgb=rgb, depth=None,
              ws=_lib.ptr(ws), ws_bytes=need, accum=acc, counts=counts)

    def call(**kw):
        a = dict(ok, **kw)
        P_ = lambda x: x if isinstance(x, ctypes.c_void_p) else _lib.ptr(x)      # noqa: E731
        return lib.dif_mesh_colour_view(P_(a["vertices"]), P_(a["normals"]), P_(a["triangles"]), a["V"], a["K"],
                                        None if a["view"] is None else ctypes.byref(a["view"]), None if a["gates"] is None else ctypes.byref(a["gates"]),
                                        P_(a["rgb"]), P_(a["depth"]), a["ws"], a["ws_bytes"], P_(a["accum"]), P_(a["counts"]), _lib.stream_ptr())

    def view(**kw):
        a = M.raster_args(P, intr, H, Wd)
        for k, x in kw.items():
            setattr(a, k, x)
        return a

    def gates(**kw):
        a = M.colour_args()
        for k, x in kw.items():
            setattr(a, k, x)
        return a

    refused = [dict(view=None), dict(gates=None), dict(rgb=None), dict(accum=None), dict(counts=None), dict(vertices=None), dict(normals=None), dict(triangles=None),
               dict(ws=ctypes.c_void_p(0)), dict(ws=ctypes.c_void_p(ws.data_ptr() + 8)), dict(ws_bytes=need - 1), dict(V=-1), dict(V=1 << 31), dict(K=-1),
               dict(K=(2 ** 31 + 2) // 3), dict(view=view(height=0)), dict(view=view(width=-3)), dict(view=view(height=1 << 16, width=1 << 15)),
               dict(view=view(fx=0.0)), dict(view=view(fy=-1.0)), dict(view=view(fx=float("nan"))), dict(view=view(fy=float("inf"))),
               dict(view=view(z_near=-0.1)), dict(view=view(z_near=float("nan"))), dict(view=view(z_near=float("inf"))),
               dict(gates=gates(depth_tol=-1e-6)), dict(gates=gates(depth_tol=float("nan"))), dict(gates=gates(depth_tol=float("inf"))),
               dict(gates=gates(min_cos2=-1e-6)), dict(gates=gates(min_cos2=float("nan"))), dict(gates=gates(min_cos2=float("inf")))]
    for kw in refused:
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert counts.cpu().tolist() == [-7] * _lib.COLOUR_COUNT and not acc.cpu().numpy().any()             # refused before anything was launched
    assert call() == 0 and call(gates=gates(depth_tol=0.0, min_cos2=0.0)) == 0 and call(depth=torch.full((H, Wd), 1.0, device=DEV)) == 0
    torch.cuda.synchronize()
    c = counts.cpu().tolist()
    assert sum(c[:6]) == H * Wd and c[_lib.COLOUR_STATUS] == 0 and c[7] == 0 and acc.cpu().numpy().any()


# ---- the rasteriser on the same workspace --------------------------------------------------------------------------------------------------
def test_the_rasteriser_is_left_alone():
    image, pose = "64x48", "turned"
    H, Wd, intr = IMAGES[image]
    P = POSES[pose]
    big = screen_mesh(P, image, [(-40.0, -30.0), (3.0 * Wd, -25.0), (-35.0, 3.0 * H)], [1.4, 1.9, 1.6], [[0, 1, 2]])
    v, n, t = concat(small(300, pose, image, 31), big)
    s = R.flat_attributes(v.shape[0], 32)[1]
    want = R.render(v, n, s, t, R.world_to_cam(P), intr, H, Wd, thread_pixels=_lib.RASTER_THREAD_PIXELS)
    lib = _lib.load()
    V, K = v.shape[0], t.shape[0]
    need = int(lib.dif_mesh_colour_workspace_bytes(V, K, H, Wd))
    ws = torch.empty((need,), dtype=torch.uint8, device=DEV)
    d = [dev(x) for x in (v, n, s, t)]
    acc = M.colour_accumulator(V, DEV)
    c = M.colour_view(d[0], d[1], d[3], acc, dev(C.random_rgb(H, Wd, 33)), P, intr, workspace=ws)
    assert c["used"] > 0
    out = [torch.empty(shape, dtype=dt, device=DEV) for shape, dt in (((H, Wd), torch.float32), ((H, Wd, 3), torch.float32), ((H, Wd), torch.float32),
                                                                     ((H, Wd), torch.int32), ((_lib.RASTER_COUNT,), torch.int32))]
    args = M.raster_args(P, intr, H, Wd)
    assert lib.dif_mesh_render(*(_lib.ptr(x) for x in d), V, K, ctypes.byref(args), _lib.ptr(ws), need, *(_lib.ptr(x) for x in out), _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert dict(zip(M.RENDER_COUNT_NAMES, out[4].cpu().tolist())) == want["counts"] and want["counts"]["large"] == 1
    for k, name in enumerate(("depth", "normal", "std", "triangle")):
        assert same_bits(out[k].cpu().numpy(), want[name]), name
    # and the other way round: the colours after a render on that workspace
    acc2 = M.colour_accumulator(V, DEV)
    assert M.colour_view(d[0], d[1], d[3], acc2, dev(C.random_rgb(H, Wd, 33)), P, intr, workspace=ws) == c and same_bits(acc.cpu().numpy(), acc2.cpu().numpy())


# ---- through the map -------------------------------------------------------------------------------------------------------------------
VIEW = (48, 64, (60.0, 60.0, 32.0, 24.0))
CENTRE = np.array([0.013, -0.021, 0.007])                                        # weld_ref.sphere_cloud


@pytest.fixture(scope="module")
def two_sphere_map(gpu_model):
    b = W.SPHERE_BOUND
    cfg = syn.MapConfig((-b, -b, -b), (b, b, b), W.SPHERE_VOXEL)
    m = DenseIndexedMap(gpu_model, cfg.namespace(), 29, DEV, initial_capacity=1024)
    assert m.coloured_mesh([]) is None                                           # a fresh map has nothing to colour
    xyz, nrm = CR.two_sphere_cloud()
    m.integrate_keyframe(dev(xyz), dev(nrm))
    m.extract_mesh_arrays(W.SPHERE_RES, int(4e6), fast=True, max_std=2000.0, to_host=False)
    return m


def orbit(k):
    """The scene is one keyframe cloud, not a stream: three poses on a circle of 2 m about the large sphere, looking at it."""
    return pose_at(CENTRE[0] - 2.0 * np.sin(0.35 * k), CENTRE[1], CENTRE[2] - 2.0 * np.cos(0.35 * k), turn=0.35 * k)


def test_through_the_map(two_sphere_map, tmp_path):
    m = two_sphere_map
    H, Wd, intr = VIEW
    mesh = m.indexed_mesh(min_component_triangles=500)
    topo = mesh.topology()
    assert topo.count == 2 and topo.n_boundary.tolist() == [0, 0]
    large = int(torch.argmax(topo.n_triangles))
    palette = np.zeros((3, 3), dtype=F32)                                        # per component; the last row is the background nobody may receive
    palette[large], palette[1 - large], palette[2] = (0.8, 0.2, 0.1), (0.1, 0.3, 0.9), (1.0, 0.0, 1.0)
    comp = topo.triangle_component.cpu().numpy()
    views, seen = [], set()
    for k in (-1, 0, 1):
        tri = mesh.render(orbit(k), intr, H, Wd).triangle.cpu().numpy()
        label = np.where(tri >= 0, comp[np.maximum(tri, 0)], 2)
        seen |= set(np.unique(label).tolist())
        views.append((dev(palette[label]), None, orbit(k), intr))
    assert seen == {0, 1, 2}                                                     # both spheres and some background are in view
    out = m.coloured_mesh(views, min_component_triangles=500)
    assert out.counts["coloured"] > 0 and out.counts["triangles"] == mesh.counts["triangles"] and same_bits(out.triangles.cpu().numpy(), mesh.triangles.cpu().numpy())
    host = out.cpu()
    colors, weight, vc = host.colors.numpy(), host.color_weight.numpy(), topo.vertex_component.cpu().numpy()
    assert int((weight > 0).sum()) == out.counts["coloured"]
    for c in (large, 1 - large):
        mine = (vc == c) & (weight > 0)
        q = [int(np.rint(float(F64(x)) * 255.0)) for x in palette[c]]
        assert mine.sum() > (0 if c != large else 200) and (colors[mine] == q).all(), (c, q, np.unique(colors[mine], axis=0))
    assert (colors[weight == 0] == 128).all() and (weight == 0).sum() > 100      # the far side of the large sphere
    print(f"two-sphere map: {out.counts}, {int((weight > 0).sum())} of {len(weight)} vertices coloured")
    # the first view against the restatement, bit for bit, through the mesh's own colourer
    col = mesh.colourer()
    c = col.add_view(*views[1][:1], views[1][2], intr)
    hm = mesh.cpu()
    want = C.colour_view(hm.vertices.numpy(), hm.normals.numpy(), hm.triangles.numpy(), R.world_to_cam(orbit(0)), intr, views[1][0].cpu().numpy())
    assert c == want["counts"] and same_bits(col.accum.cpu().numpy(), want["accum"])
    # a threshold nobody reaches leaves every vertex grey
    grey = m.coloured_mesh(views, min_component_triangles=500, min_weight=1e6)
    assert grey.counts["coloured"] == 0 and (grey.colors.cpu().numpy() == 128).all() and same_bits(grey.color_weight.cpu().numpy(), weight)
    out.write_ply(tmp_path / "coloured.ply")
    vert, face = C.read_ply(tmp_path / "coloured.ply")
    assert vert.dtype.names[-3:] == ("red", "green", "blue") and np.array_equal(np.stack([vert[k] for k in ("red", "green", "blue")], axis=1), colors)
    assert np.array_equal(face["v"], host.triangles.numpy()) and same_bits(np.stack([vert[k] for k in "xyz"], axis=1), host.vertices.numpy())
