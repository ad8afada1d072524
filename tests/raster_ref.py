"""Numpy restatement of `dif_mesh_render` (DESIGN.md "Rendering an indexed mesh"), written from the rule, not from the kernel: float32 for the
projection, int64 for the edge functions, float64 for the depth, the barycentric weights, the normal and the std, every operation in the
stated order.  A Python loop over the triangles (test sizes), numpy over the pixels of a triangle's box.  tests/test_raster_cpu.py holds this
file to what a renderer must produce; tests/test_gpu_raster.py holds the kernels to this file, bit for bit.

The rule.  Camera point pc[k] = ((r[k][0] x + r[k][1] y) + r[k][2] z) + t[k] in float32.  A vertex is valid when pc is finite, pc.z > z_near
and both snapped coordinates X = rint((fx (pc.x / pc.z) + cx) 256), Y likewise, are below 2^22 in magnitude; iz = 1 / (double) pc.z.
A triangle, in this order: an index outside [0, V) -> dropped, status BAD_INDEX; an invalid vertex -> clipped; area2 = (X1 - X0)(Y2 - Y0) -
(X2 - X0)(Y1 - Y0) == 0 -> degenerate; cull_backfaces and area2 > 0 (cross(p1 - p0, p2 - p0) points away from the camera) -> culled;
area2 < 0 -> vertices 1 and 2 swap; no pixel centre (256 i, 256 j) in the bounding box clipped to the image -> offscreen; else drawn, and
large if the box holds more than `thread_pixels` pixels.  Edge p -> q (v1->v2, v2->v0, v0->v1): E = dx (py - Yp) - dy (px - Xp); the pixel is
covered when every E >= 0 if (dy < 0 or (dy == 0 and dx > 0)) else E >= 1.  s = (E0 iz0 + E1 iz1) + E2 iz2, depth = float32(area2 / s);
the pixel keeps the lowest (depth bits << 32 | triangle index).  b_k = (E_k iz_k) / s; std = float32((b0 s0 + b1 s1) + b2 s2); n likewise per
component, / sqrt((nx nx + ny ny) + nz nz), zero when that length is 0 or not finite.  Empty pixel: depth NaN, normal 0, std NaN, triangle -1.
"""
import numpy as np

F32, F64, I64 = np.float32, np.float64, np.int64
BAD_INDEX = 1
GUARD = 2.0 ** 22
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
COUNT_NAMES = ("pixels_hit", "drawn", "clipped", "degenerate", "culled", "offscreen", "large", "status")
THREAD_PIXELS = 64


def world_to_cam(pose):
    """camera-to-world 4x4 (or (R, t)) -> the 12 float32 of the row-major 3x4 world-to-camera transform: R^T and -R^T t in float64, rounded."""
    if isinstance(pose, tuple):
        R, t = np.asarray(pose[0], dtype=F64), np.asarray(pose[1], dtype=F64)
    else:
        pose = np.asarray(pose, dtype=F64)
        R, t = pose[:3, :3], pose[:3, 3]
    return np.concatenate([R.T, -(R.T @ t)[:, None]], axis=1).astype(F32).reshape(12)


def project(vertices, w2c, intrinsics, z_near):
    """-> X, Y (int64), iz (float64), valid (bool), per vertex"""
    v = np.asarray(vertices, dtype=F32).reshape(-1, 3)
    r = np.asarray(w2c, dtype=F32).reshape(3, 4)
    fx, fy, cx, cy = (F32(a) for a in intrinsics)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    with np.errstate(all="ignore"):
        pc = [((r[k, 0] * x + r[k, 1] * y) + r[k, 2] * z) + r[k, 3] for k in range(3)]
        assert all(p.dtype == F32 for p in pc)
        sx = np.rint((fx * (pc[0] / pc[2]) + cx) * F32(256.0))
        sy = np.rint((fy * (pc[1] / pc[2]) + cy) * F32(256.0))
        assert sx.dtype == F32 and sy.dtype == F32
        valid = np.isfinite(pc[0]) & np.isfinite(pc[1]) & np.isfinite(pc[2]) & (pc[2] > F32(z_near))
        valid &= (np.abs(sx) < F32(GUARD)) & (np.abs(sy) < F32(GUARD))          # (NaN fails)
        X = np.where(valid, sx, 0).astype(I64)
        Y = np.where(valid, sy, 0).astype(I64)
        iz = np.where(valid, 1.0 / pc[2].astype(F64), 0.0)
    return X, Y, iz, valid


def _edges(X, Y, o, px, py):
    """E0, E1, E2 (int64 arrays over the pixels) of the oriented triangle o = (v0, v1, v2), and the coverage"""
    E, cover = [], np.ones(np.shape(px), dtype=bool)
    for p, q in ((o[1], o[2]), (o[2], o[0]), (o[0], o[1])):
        dx, dy = int(X[q] - X[p]), int(Y[q] - Y[p])
        e = I64(dx) * (py - I64(Y[p])) - I64(dy) * (px - I64(X[p]))
        cover &= e >= (0 if (dy < 0 or (dy == 0 and dx > 0)) else 1)
        E.append(e)
    return E, cover


def render(vertices, normals, vertex_std, triangles, w2c, intrinsics, height, width, z_near=0.05, cull_backfaces=False, thread_pixels=THREAD_PIXELS):
    """-> dict(depth (H,W) f32, normal (H,W,3) f32, std (H,W) f32, triangle (H,W) i32, counts {name: int}, coverage (H,W) i32: how many
    triangles cover each pixel, hidden ones included — for the tests of the coverage rule, not an output of the library)"""
    H, W = int(height), int(width)
    tris = np.asarray(triangles).reshape(-1, 3).astype(I64)
    V = np.asarray(vertices).reshape(-1, 3).shape[0]
    nrm = np.asarray(normals, dtype=F32).reshape(-1, 3).astype(F64)
    std = np.asarray(vertex_std, dtype=F32).reshape(-1).astype(F64)
    X, Y, iz, valid = project(vertices, w2c, intrinsics, z_near)
    counts = dict.fromkeys(COUNT_NAMES, 0)
    zbuf = np.full((H, W), EMPTY, dtype=np.uint64)
    coverage = np.zeros((H, W), dtype=np.int32)
    oriented = np.zeros((tris.shape[0], 3), dtype=I64)
    for t, (a, b, c) in enumerate(tris.tolist()):
        if not (0 <= a < V and 0 <= b < V and 0 <= c < V):
            counts["status"] |= BAD_INDEX
            continue
        if not (valid[a] and valid[b] and valid[c]):
            counts["clipped"] += 1
            continue
        area2 = int(X[b] - X[a]) * int(Y[c] - Y[a]) - int(X[c] - X[a]) * int(Y[b] - Y[a])
        if area2 == 0:
            counts["degenerate"] += 1
            continue
        if cull_backfaces and area2 > 0:
            counts["culled"] += 1
            continue
        o = (a, b, c)
        if area2 < 0:
            o, area2 = (a, c, b), -area2
        oriented[t] = o
        xs, ys = [int(X[k]) for k in o], [int(Y[k]) for k in o]
        i0, i1 = max(-(-min(xs) // 256), 0), min(max(xs) // 256, W - 1)         # ceil, floor
        j0, j1 = max(-(-min(ys) // 256), 0), min(max(ys) // 256, H - 1)
        if i0 > i1 or j0 > j1:
            counts["offscreen"] += 1
            continue
        counts["drawn"] += 1
        if (i1 - i0 + 1) * (j1 - j0 + 1) > thread_pixels:
            counts["large"] += 1
        jj, ii = np.meshgrid(np.arange(j0, j1 + 1, dtype=I64), np.arange(i0, i1 + 1, dtype=I64), indexing="ij")
        E, cover = _edges(X, Y, o, I64(256) * ii, I64(256) * jj)
        if not cover.any():
            continue
        assert np.all(E[0] + E[1] + E[2] == area2)
        s = (E[0].astype(F64) * iz[o[0]] + E[1].astype(F64) * iz[o[1]]) + E[2].astype(F64) * iz[o[2]]
        d = (F64(area2) / s[cover]).astype(F32)
        word = (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(t)
        sub = zbuf[j0:j1 + 1, i0:i1 + 1]
        sub[cover] = np.minimum(sub[cover], word)
        coverage[j0:j1 + 1, i0:i1 + 1] += cover
    hit = zbuf != EMPTY
    counts["pixels_hit"] = int(hit.sum())
    depth = np.full((H, W), np.nan, dtype=F32)
    out_std = np.full((H, W), np.nan, dtype=F32)
    normal = np.zeros((H, W, 3), dtype=F32)
    triangle = np.full((H, W), -1, dtype=np.int32)
    if hit.any():
        jj, ii = np.nonzero(hit)
        w = zbuf[hit]
        t = (w & np.uint64(0xFFFFFFFF)).astype(I64)
        depth[hit] = (w >> np.uint64(32)).astype(np.uint32).view(F32)
        triangle[hit] = t.astype(np.int32)
        o = oriented[t]                                                         # (P, 3)
        px, py = I64(256) * ii.astype(I64), I64(256) * jj.astype(I64)
        E = []
        for p, q in ((1, 2), (2, 0), (0, 1)):
            dx, dy = X[o[:, q]] - X[o[:, p]], Y[o[:, q]] - Y[o[:, p]]
            E.append(dx * (py - Y[o[:, p]]) - dy * (px - X[o[:, p]]))
        z = [iz[o[:, k]] for k in range(3)]
        s = (E[0].astype(F64) * z[0] + E[1].astype(F64) * z[1]) + E[2].astype(F64) * z[2]
        b = [(E[k].astype(F64) * z[k]) / s for k in range(3)]
        with np.errstate(all="ignore"):
            out_std[hit] = ((b[0] * std[o[:, 0]] + b[1] * std[o[:, 1]]) + b[2] * std[o[:, 2]]).astype(F32)
            n = [(b[0] * nrm[o[:, 0], k] + b[1] * nrm[o[:, 1], k]) + b[2] * nrm[o[:, 2], k] for k in range(3)]
            length = np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
            ok = (length > 0.0) & np.isfinite(length)
            normal[hit] = np.stack([np.where(ok, n[k] / length, 0.0).astype(F32) for k in range(3)], axis=1)
    return dict(depth=depth, normal=normal, std=out_std, triangle=triangle, counts=counts, coverage=coverage)


# ---- inputs shared by the CPU and the GPU tests -----------------------------------------------------------------------------------------
def icosphere(subdivisions, radius=0.45, centre=(0.0, 0.0, 0.0)):
    """A closed sphere of 20 * 4^subdivisions triangles, wound so that cross(p1 - p0, p2 - p0) points outwards; normals = radial, std = a smooth
    function of the position.  -> vertices (V,3) f32, normals (V,3) f32, std (V,) f32, triangles (K,3) i32"""
    g = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    v = [np.asarray(p, dtype=F64) / np.linalg.norm(p) for p in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(subdivisions):
        mid, nf = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[k] = len(v) - 1
            return mid[k]

        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    n = np.asarray(v)
    tris = np.asarray(f, dtype=np.int32)
    p = np.asarray(centre, dtype=F64) + radius * n
    out = np.einsum("ij,ij->i", np.cross(p[tris[:, 1]] - p[tris[:, 0]], p[tris[:, 2]] - p[tris[:, 0]]), n[tris[:, 0]])
    assert (out > 0).all()
    std = 0.01 + 0.005 * (n[:, 0] + 0.5 * n[:, 1])
    return p.astype(F32), n.astype(F32), std.astype(F32), tris


def plane_point(w2c, intrinsics, u, v, z):
    """World point (float64) that the camera sees at pixel position (u, v) (fractions allowed) and camera depth z."""
    r = np.asarray(w2c, dtype=F64).reshape(3, 4)
    fx, fy, cx, cy = (float(a) for a in intrinsics)
    pc = np.array([(u - cx) / fx * z, (v - cy) / fy * z, z])
    return r[:, :3].T @ (pc - r[:, 3])


def plane_points(w2c, intrinsics, uv, z):
    """`plane_point` for arrays: uv (N,2), z (N,) -> (N,3) float64"""
    r = np.asarray(w2c, dtype=F64).reshape(3, 4)
    fx, fy, cx, cy = (float(a) for a in intrinsics)
    uv, z = np.asarray(uv, dtype=F64), np.asarray(z, dtype=F64)
    pc = np.stack([(uv[:, 0] - cx) / fx * z, (uv[:, 1] - cy) / fy * z, z], axis=1)
    return (pc - r[:, 3]) @ r[:, :3]


def small_triangles(K, w2c, intrinsics, height, width, seed=0, depth=(0.6, 3.0)):
    """K triangles of 1-4 pixels across, every vertex at a depth of its own near the triangle's, with random attributes.  Half of them crowd
    into a patch of 10 x 8 pixels (deep stacks of overlapping triangles at any K), the others scatter over the image and two pixels beyond its
    rim.  -> vertices (3K,3) f32, normals, std, triangles (K,3) i32"""
    rng = np.random.default_rng(seed)
    centre = rng.uniform((-2.0, -2.0), (width + 1.0, height + 1.0), size=(K, 2))
    corner = rng.uniform((0.0, 0.0), (max(width - 10.0, 1.0), max(height - 8.0, 1.0)))
    crowd = rng.random(K) < 0.5
    centre[crowd] = corner + rng.uniform((0.0, 0.0), (10.0, 8.0), size=(int(crowd.sum()), 2))
    ang = rng.uniform(0.0, 2.0 * np.pi, size=(K, 1)) + np.array([0.0, 2.1, 4.2]) + rng.uniform(-0.5, 0.5, size=(K, 3))
    radius = rng.uniform(0.6, 2.3, size=(K, 1)) * rng.uniform(0.7, 1.0, size=(K, 3))
    uv = centre[:, None, :] + radius[..., None] * np.stack([np.cos(ang), np.sin(ang)], axis=-1)
    z = rng.uniform(*depth, size=(K, 1)) * rng.uniform(0.97, 1.03, size=(K, 3))
    v = plane_points(w2c, intrinsics, uv.reshape(-1, 2), z.reshape(-1)).astype(F32)
    n, s = flat_attributes(3 * K, seed + 1)
    return v, n, s, np.arange(3 * K, dtype=np.int32).reshape(K, 3)


def shared_edge_pair(w2c, intrinsics, z=1.5):
    """Two triangles sharing the edge (8, 8) - (24, 24), which runs through pixel centres; the outer corners sit on pixel centres too, so
    further centres lie on the outer edges."""
    q = [(8, 8), (24, 24), (24, 8), (8, 24)]
    v = np.stack([plane_point(w2c, intrinsics, u, w, z) for u, w in q]).astype(F32)
    return v, np.array([[0, 1, 2], [1, 0, 3]], dtype=np.int32)


def vertex_fan(w2c, intrinsics, n=7, centre=(20, 15), radius=9.3, z=1.2):
    """n triangles around a vertex that projects exactly onto a pixel centre"""
    ang = 0.3 + 2.0 * np.pi * np.arange(n) / n
    q = [centre] + [(centre[0] + radius * np.cos(a), centre[1] + radius * np.sin(a)) for a in ang]
    v = np.stack([plane_point(w2c, intrinsics, u, w, z) for u, w in q]).astype(F32)
    return v, np.array([[0, 1 + k, 1 + (k + 1) % n] for k in range(n)], dtype=np.int32)


def flat_attributes(V, seed=0):
    """random unit normals and positive stds for V vertices"""
    rng = np.random.default_rng(seed)
    n = rng.standard_normal((V, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    return n.astype(F32), (0.01 + 0.02 * rng.random(V)).astype(F32)
