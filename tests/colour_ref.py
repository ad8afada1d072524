"""Numpy restatement of `dif_mesh_colour_view` and `dif_mesh_colour_resolve` (DESIGN.md "Colouring an indexed mesh"), written from the rule, not
from the kernel.  Projection, coverage and the z-buffer are tests/raster_ref.py's (its depth and triangle images ARE the z-buffer: depth bits
and winner); the per-pixel arithmetic follows the stated order in float64, the sums are np.uint64 — integers, so no order of additions can
show.  tests/test_colour_cpu.py holds this file to what the rule implies; tests/test_gpu_colour.py holds the kernels to this file, bit for bit.

The rule.  Every pixel falls into exactly one class, tested in this order.  NO_HIT: no triangle won the pixel.  BAD_COLOUR: one of its three
rgb values is not finite.  DEPTH: a depth frame is given and its value is not finite or |depth_in - d| > depth_tol in float32, d = the z-buffer
depth.  EDGE: the edge gate is on and a 4-neighbour inside the image is empty or has a depth dn with |dn - d| > depth_tol.  GRAZING: with the
barycentrics b_k = (E_k iz_k) / s of the rasteriser, n = (b0 n0 + b1 n1) + b2 n2 per component, the view ray dw = R^T (rx, ry, 1) with
rx = (i - cx) / fx, ry = (j - cy) / fy and each component (a rx + b ry) + c over column k of the world-to-camera rotation,
nd = (n.x dw.x + n.y dw.y) + n.z dw.z, nn and dd likewise, cos2 = (nd nd) / (nn dd): not (nn > 0), cos2 not finite, or cos2 < min_cos2.
USED: q_c = rint(clip(rgb_c, 0, 1) 255), w_k = rint((b_k cos2) 65536); w_k q_r, w_k q_g, w_k q_b, w_k are added to vertex k of the oriented
triangle.  Resolve: S = the summed weight; S >= max(min_weight, 1): (2 sum_c + S) // (2 S), else 128; weight = float32(S / 65536).
"""
import numpy as np

from tests import raster_ref as R

F32, F64, I64, U64 = np.float32, np.float64, np.int64, np.uint64
USED, NO_HIT, BAD_COLOUR, DEPTH, EDGE, GRAZING = range(6)
COUNT_NAMES = ("used", "no_hit", "bad_colour", "depth", "edge", "grazing", "status")
WEIGHT_ONE = 65536


def min_cos2(min_cos):
    """the float32 the library compares cos^2 with: squared in float64, rounded once"""
    return F32(F64(min_cos) * F64(min_cos))


def depth_steps(depth, tol):
    """(H,W) bool: the pixel has a 4-neighbour inside the image that is empty (NaN) or whose depth differs by more than tol (float32)"""
    d = np.asarray(depth, dtype=F32)
    empty = np.isnan(d)
    out = np.zeros(d.shape, dtype=bool)
    with np.errstate(invalid="ignore"):
        def far(dn, dc, en):
            diff = np.abs(dn - dc)
            assert diff.dtype == F32
            return en | (diff > F32(tol))
        out[:, 1:] |= far(d[:, :-1], d[:, 1:], empty[:, :-1])                    # the neighbour on the left
        out[:, :-1] |= far(d[:, 1:], d[:, :-1], empty[:, 1:])                    # on the right
        out[1:, :] |= far(d[:-1, :], d[1:, :], empty[:-1, :])                    # above
        out[:-1, :] |= far(d[1:, :], d[:-1, :], empty[1:, :])                    # below
    return out


def colour_view(vertices, normals, triangles, w2c, intrinsics, rgb, depth_in=None, depth_tol=0.02, min_cos2=min_cos2(0.3), edge_gate=True,
                z_near=0.05, cull_backfaces=False, accum=None):
    """Adds one view to `accum` ((V,4) uint64; a zeroed one if None; the argument itself is left alone).
    -> dict(accum (V,4) uint64, counts {name: int}, classes (H,W) int, weights (H,W,3) uint64: w_k of the USED pixels, vertex (H,W,3) int: the
    oriented triangle's vertices at the pixels that reached the grazing test (-1 elsewhere), cos2 (H,W) f64 (NaN elsewhere),
    render: what raster_ref.render gave for the view)"""
    rgb = np.asarray(rgb, dtype=F32)
    H, W = rgb.shape[:2]
    assert rgb.shape == (H, W, 3)
    v = np.asarray(vertices, dtype=F32).reshape(-1, 3)
    V = v.shape[0]
    nrm = np.asarray(normals, dtype=F32).reshape(-1, 3).astype(F64)
    tris = np.asarray(triangles).reshape(-1, 3).astype(I64)
    acc = np.zeros((V, 4), dtype=U64) if accum is None else np.array(accum, dtype=U64, copy=True)
    assert acc.shape == (V, 4)
    tol = F32(depth_tol)
    rend = R.render(v, nrm.astype(F32), np.zeros(V, dtype=F32), tris, w2c, intrinsics, H, W, z_near=z_near, cull_backfaces=cull_backfaces)
    tri_img, d = rend["triangle"], rend["depth"]
    cls = np.full((H, W), NO_HIT, dtype=np.int32)
    todo = tri_img >= 0
    bad = todo & ~np.isfinite(rgb).all(axis=2)
    cls[bad] = BAD_COLOUR
    todo &= ~bad
    if depth_in is not None:
        din = np.asarray(depth_in, dtype=F32)
        assert din.shape == (H, W)
        with np.errstate(invalid="ignore"):
            diff = np.abs(din - d)
            assert diff.dtype == F32
            off = todo & (~np.isfinite(din) | (diff > tol))
        cls[off] = DEPTH
        todo &= ~off
    if edge_gate:
        edge = todo & depth_steps(d, tol)
        cls[edge] = EDGE
        todo &= ~edge
    weights = np.zeros((H, W, 3), dtype=U64)
    vertex = np.full((H, W, 3), -1, dtype=I64)
    cos2_img = np.full((H, W), np.nan, dtype=F64)
    if todo.any():
        X, Y, iz, _ = R.project(v, w2c, intrinsics, z_near)
        jj, ii = np.nonzero(todo)
        t = tri_img[todo].astype(I64)
        a, b, c = tris[t, 0], tris[t, 1], tris[t, 2]
        area2 = (X[b] - X[a]) * (Y[c] - Y[a]) - (X[c] - X[a]) * (Y[b] - Y[a])
        assert (area2 != 0).all()
        swapped = area2 < 0
        o = np.stack([a, np.where(swapped, c, b), np.where(swapped, b, c)], axis=1)
        px, py = I64(256) * ii.astype(I64), I64(256) * jj.astype(I64)
        E = []
        for p, q in ((1, 2), (2, 0), (0, 1)):
            dx, dy = X[o[:, q]] - X[o[:, p]], Y[o[:, q]] - Y[o[:, p]]
            E.append(dx * (py - Y[o[:, p]]) - dy * (px - X[o[:, p]]))
        z = [iz[o[:, k]] for k in range(3)]
        s = (E[0].astype(F64) * z[0] + E[1].astype(F64) * z[1]) + E[2].astype(F64) * z[2]
        bk = [(E[k].astype(F64) * z[k]) / s for k in range(3)]
        r = np.asarray(w2c, dtype=F32).reshape(3, 4).astype(F64)
        fx, fy, cx, cy = (F64(F32(x)) for x in intrinsics)
        rx, ry = (ii.astype(F64) - cx) / fx, (jj.astype(F64) - cy) / fy
        with np.errstate(all="ignore"):
            n = [(bk[0] * nrm[o[:, 0], k] + bk[1] * nrm[o[:, 1], k]) + bk[2] * nrm[o[:, 2], k] for k in range(3)]
            dw = [(r[0, k] * rx + r[1, k] * ry) + r[2, k] for k in range(3)]
            nd = (n[0] * dw[0] + n[1] * dw[1]) + n[2] * dw[2]
            nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]
            dd = (dw[0] * dw[0] + dw[1] * dw[1]) + dw[2] * dw[2]
            cos2 = (nd * nd) / (nn * dd)
            grazing = ~(nn > 0.0) | ~np.isfinite(cos2) | (cos2 < F64(F32(min_cos2)))
        cls[jj, ii] = np.where(grazing, GRAZING, USED)
        vertex[jj, ii] = o
        cos2_img[jj, ii] = cos2
        u = ~grazing
        if u.any():
            q = np.rint(np.minimum(np.maximum(rgb[jj[u], ii[u]].astype(F64), 0.0), 1.0) * 255.0).astype(U64)          # (P, 3)
            for k in range(3):
                w = np.rint((bk[k][u] * cos2[u]) * F64(WEIGHT_ONE)).astype(U64)
                assert int(w.max()) * 255 < 2 ** 24
                weights[jj[u], ii[u], k] = w
                send = w > 0
                for ch in range(3):
                    np.add.at(acc[:, ch], o[u, k][send], w[send] * q[send, ch])
                np.add.at(acc[:, 3], o[u, k][send], w[send])
    counts = {name: int((cls == k).sum()) for k, name in enumerate(COUNT_NAMES[:6])}
    counts["status"] = rend["counts"]["status"]
    return dict(accum=acc, counts=counts, classes=cls, weights=weights, vertex=vertex, cos2=cos2_img, render=rend)


def resolve(accum, min_weight=0):
    """`min_weight` in accumulator units (weight * 65536), an integer.  -> rgb8 (V,3) uint8, weight (V,) f32, vertices coloured"""
    acc = np.asarray(accum, dtype=U64).reshape(-1, 4)
    V = acc.shape[0]
    rgb8 = np.full((V, 3), 128, dtype=np.uint8)
    least = max(int(min_weight), 1)
    n = 0
    for i in range(V):
        S = int(acc[i, 3])                                                       # Python integers: no width to overflow
        if S >= least:
            n += 1
            for ch in range(3):
                q = (2 * int(acc[i, ch]) + S) // (2 * S)
                assert 0 <= q <= 255
                rgb8[i, ch] = q
    weight = (acc[:, 3].astype(F64) / F64(WEIGHT_ONE)).astype(F32)
    return rgb8, weight, n


def weight_units(min_weight):
    """a weight in pixels -> the integer the entry point takes (the least S that passes)"""
    return int(np.ceil(F64(min_weight) * F64(WEIGHT_ONE)))


# ---- inputs and helpers shared by the CPU and the GPU tests ------------------------------------------------------------------------------
def random_rgb(height, width, seed=0):
    """(H,W,3) float32, mostly inside [0,1], some values below 0 and above 1 (the clamp)"""
    rng = np.random.default_rng(seed)
    return rng.uniform(-0.1, 1.1, size=(height, width, 3)).astype(F32)


def two_spheres(subdivisions=2):
    """A small sphere (r 0.12) 0.9 in front of a large one (r 0.45 at the origin) for a camera on the negative z axis: a depth step of more
    than 0.4 all around the small one's silhouette.  -> vertices, normals, triangles, first vertex of the small sphere"""
    v0, n0, _, t0 = R.icosphere(subdivisions, 0.45)
    v1, n1, _, t1 = R.icosphere(subdivisions, 0.12, centre=(0.05, 0.02, -0.9))
    return np.concatenate([v0, v1]), np.concatenate([n0, n1]), np.concatenate([t0, t1 + v0.shape[0]]).astype(np.int32), v0.shape[0]


def read_ply(path):
    """Reader for what `IndexedMesh.write_ply` writes, colours included: binary little-endian, float and uchar vertex properties,
    uchar/int face lists.  -> vertex records, face records"""
    data = open(path, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    counts, props, element = {}, [], None
    for ln in lines:
        w = ln.split()
        if w[:1] == ["element"]:
            element = w[1]
            counts[element] = int(w[2])
        elif w[:1] == ["property"] and element == "vertex":
            props.append((w[2], {"float": "<f4", "uchar": "u1"}[w[1]]))
        elif w[:1] == ["property"] and element == "face":
            assert w[1:] == ["list", "uchar", "int", "vertex_indices"]
    vert = np.frombuffer(data, dtype=props, count=counts["vertex"], offset=end)
    face = np.frombuffer(data, dtype=[("n", "u1"), ("v", "<i4", (3,))], count=counts["face"], offset=end + vert.nbytes)
    assert end + vert.nbytes + face.nbytes == len(data)
    return vert, face
