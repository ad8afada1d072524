"""numpy restatement of the mesh weld (`dif_mesh_weld`, di_fusion_amd/system/mesh.py): keys by lattice edge, classes, first-occurrence vertex
order, degenerate drop, fixed-point area-weighted normals.  Written from the operator's specification (DESIGN.md "Indexed mesh"), not from the
kernel: the GPU tests hold the kernel to it, the CPU tests hold it to the topology it is meant to produce.

All key arithmetic is float32, as on the device (the library is built without contraction, so numpy float32 reproduces it).
"""
import numpy as np

F32 = np.float32
LATTICE_TOL = F32(2.0 ** -10)        # of a cell
KEY_LIMIT = 1 << 20                  # lattice coordinates are packed in 20 bits each
NORMAL_SCALE = 2.0 ** 30             # fixed point of the normal sums (the groupby sum's convention)


def corner_keys(p, bound_min, voxel_size, r):
    """(N,3) float32 positions -> (key int64 (N,), keyed bool (N,)).  An unkeyed corner is its own vertex."""
    p = np.asarray(p, dtype=F32).reshape(-1, 3)
    n = p.shape[0]
    bm = np.asarray(bound_min, dtype=F32)
    with np.errstate(all="ignore"):
        L = ((p - bm) / F32(voxel_size)) * F32(r)
        q = np.rint(L)
        f = np.abs(L - q)
    assert L.dtype == F32 and f.dtype == F32
    finite = np.isfinite(L).all(axis=1)
    f = np.where(finite[:, None], f, F32(0))
    rows = np.arange(n)
    a = np.argmax(f, axis=1)                                  # ties: lowest axis
    others = f.copy()
    others[rows, a] = 0
    on_lattice = (others < LATTICE_TOL).all(axis=1)
    corner = f[rows, a] < LATTICE_TOL
    c = np.where(finite[:, None], q, F32(0))
    c[rows, a] = np.where(corner, c[rows, a], np.where(finite, np.floor(L[rows, a]), F32(0)))
    kind = np.where(corner, 3, a).astype(np.int64)
    in_range = ((c >= 0) & (c < KEY_LIMIT)).all(axis=1)
    keyed = finite & on_lattice & in_range
    ci = np.where(keyed[:, None], c, F32(0)).astype(np.int64)
    key = (ci[:, 0] << 42) | (ci[:, 1] << 22) | (ci[:, 2] << 2) | kind
    return key, keyed


def _normals(vertices, tris, voxel_size, r):
    V = vertices.shape[0]
    s = F32(r) / F32(voxel_size)
    p0, p1, p2 = (vertices[tris[:, k]] for k in range(3))
    e1, e2 = (p1 - p0) * s, (p2 - p0) * s
    cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    c = np.stack([cx, cy, cz], axis=1)
    assert c.dtype == F32
    with np.errstate(all="ignore"):                                          # (a NaN corner: garbage in, garbage out)
        fixed = np.rint(c.astype(np.float64) * NORMAL_SCALE).astype(np.int64)
    acc = np.zeros((V, 3), dtype=np.int64)
    for k in range(3):
        np.add.at(acc, tris[:, k], fixed)
    a = acc.astype(np.float64)
    length = np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2])
    with np.errstate(all="ignore"):
        nrm = np.where(length[:, None] > 0, a / length[:, None], 0.0)
    return nrm.astype(F32)


def weld(tri, std, ids, bound_min, voxel_size, r):
    """tri (T,3,3) f32, std (T,3) f32, ids (T,) i64 -> dict(vertices (V,3), normals (V,3), vertex_std (V,), triangles (K,3) i32,
    triangle_flatten_id (K,) i64, counts [V, kept, dropped, unkeyed, status])."""
    tri = np.ascontiguousarray(tri, dtype=F32).reshape(-1, 3, 3)
    T = tri.shape[0]
    p = tri.reshape(-1, 3)
    std = np.ascontiguousarray(std, dtype=F32).reshape(-1)
    ids = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
    n = 3 * T
    key, keyed = corner_keys(p, bound_min, voxel_size, r)
    label = np.where(keyed, key, -1 - np.arange(n, dtype=np.int64))          # an unkeyed corner: a class of its own
    _, first, inv = np.unique(label, return_index=True, return_inverse=True)
    inv = inv.reshape(-1)
    order = np.argsort(first, kind="stable")                                  # representatives (lowest soup index of a class) in soup order
    rank = np.empty_like(order)
    rank[order] = np.arange(order.size)
    reps = first[order]
    vid = rank[inv].astype(np.int32).reshape(T, 3)
    vertices = p[reps].copy()
    keep = (vid[:, 0] != vid[:, 1]) & (vid[:, 1] != vid[:, 2]) & (vid[:, 0] != vid[:, 2])
    tris = np.ascontiguousarray(vid[keep])
    return dict(vertices=vertices, normals=_normals(vertices, tris, voxel_size, r), vertex_std=std[reps].copy(), triangles=tris,
                triangle_flatten_id=ids[keep].copy(),
                counts=np.array([reps.size, int(keep.sum()), int(T - keep.sum()), int(n - keyed.sum()), 0], dtype=np.int32))


def weld_exact(tri):
    """The weld that does NOT close the mesh: classes of bit-identical positions.  Returns (V, triangles (K,3)) with degenerates dropped."""
    p = np.ascontiguousarray(tri, dtype=F32).reshape(-1, 3)
    bits = np.ascontiguousarray(p + F32(0)).view(np.uint32).reshape(-1, 3)    # (+0: -0.0 and 0.0 are one position)
    _, inv = np.unique(bits, axis=0, return_inverse=True)
    vid = inv.reshape(-1, 3)
    keep = (vid[:, 0] != vid[:, 1]) & (vid[:, 1] != vid[:, 2]) & (vid[:, 0] != vid[:, 2])
    return int(inv.max()) + 1 if inv.size else 0, vid[keep]


# ---- topology ------------------------------------------------------------------------------------------------------------------------
def topology(V, tris):
    """Edge and component census of an indexed mesh: dict(max_edge_use, n_boundary, comps=[dict(V, E, F, boundary, euler)] largest first,
    boundary_comp_sizes = vertex count of the component of every boundary edge)."""
    tris = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    e = np.concatenate([tris[:, [0, 1]], tris[:, [1, 2]], tris[:, [2, 0]]], axis=0)
    e = np.sort(e, axis=1)
    ue, cnt = np.unique(e, axis=0, return_counts=True)
    parent = np.arange(V)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in ue:
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    root = np.array([find(x) for x in range(V)], dtype=np.int64)
    used = np.zeros(V, dtype=bool)
    used[tris.reshape(-1)] = True
    comps = []
    for r_ in np.unique(root[used]):
        nv = int((root == r_).sum())
        em = root[ue[:, 0]] == r_
        ne = int(em.sum())
        nf = int((root[tris[:, 0]] == r_).sum())
        comps.append(dict(V=nv, E=ne, F=nf, boundary=int((cnt[em] == 1).sum()), euler=nv - ne + nf))
    comps.sort(key=lambda c: -c["V"])
    size_of = {int(r_): int((root == r_).sum()) for r_ in np.unique(root)}
    bsizes = [size_of[int(root[a])] for a, _ in ue[cnt == 1]]
    return dict(max_edge_use=int(cnt.max()) if cnt.size else 0, n_boundary=int((cnt == 1).sum()), comps=comps, boundary_comp_sizes=bsizes,
                n_used_vertices=int(used.sum()))


def assert_closed_surface(V, tris):
    """The three properties the weld is for: no edge with more than two triangles; every boundary edge in a component holding less than 2 % of
    the vertices; the largest component closed with V - E + F = 2."""
    t = topology(V, tris)
    assert t["max_edge_use"] <= 2, t["max_edge_use"]
    assert all(s < 0.02 * V for s in t["boundary_comp_sizes"]), (sorted(t["boundary_comp_sizes"])[-5:], V)
    big = t["comps"][0]
    assert big["boundary"] == 0 and big["euler"] == 2, big
    return t


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
SPHERE_BOUND, SPHERE_VOXEL, SPHERE_RES = 0.8, 0.1, 4


def sphere_cloud():
    """120,000 points on a sphere of radius 0.45 about (0.013, -0.021, 0.007), normals = surface normals (float32)."""
    rng = np.random.default_rng(0)
    nrm = rng.standard_normal((120000, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    xyz = np.array([0.013, -0.021, 0.007]) + 0.45 * nrm
    return xyz.astype(F32), nrm.astype(F32)


def sheet_soup(T, r=4, voxel_size=0.1, bound_min=(-0.8, -0.8, -0.8), width=9, seed=0):
    """T triangles over the squares of one lattice plane, five per square.  Their corners are the square's lattice corners and points ON the x
    and y lattice edges that leave them, so a vertex is shared by 1 to 6 soup corners (fewer at the rim of the sheet).  Where on its edge a
    vertex sits is a function of the edge; on top of that every coordinate of every copy moves by -1, 0 or +1 ulp (what an interpolation with
    reversed end points leaves behind).  Returns (tri (T,3,3) f32, std (T,3) f32, ids (T,) i64)."""
    rng = np.random.default_rng(seed)
    bm = np.asarray(bound_min, dtype=np.float64)
    cell = voxel_size / r
    n_sq = (T + 4) // 5
    s = np.arange(n_sq)
    i, j = (s % width).astype(np.float64), (s // width).astype(np.float64)
    z = np.full(n_sq, 5.0)

    def fx(i_, j_):
        return 0.25 + 0.5 * ((i_ * 7 + j_ * 3) % 11) / 11.0

    def fy(i_, j_):
        return 0.25 + 0.5 * ((i_ * 5 + j_ * 2) % 13) / 13.0

    c00 = np.stack([i, j, z], axis=1)
    ex = np.stack([i + fx(i, j), j, z], axis=1)
    ey = np.stack([i, j + fy(i, j), z], axis=1)
    ex1 = np.stack([i + fx(i, j + 1), j + 1, z], axis=1)              # the x edge of square (i, j + 1)
    ey1 = np.stack([i + 1, j + fy(i + 1, j), z], axis=1)              # the y edge of square (i + 1, j)
    c10, c01 = c00 + np.array([1.0, 0, 0]), c00 + np.array([0, 1.0, 0])
    tri = np.empty((5 * n_sq, 3, 3), dtype=np.float64)
    for k, t in enumerate([(c00, ex, ey), (ex, c10, ey1), (ey, ex1, c01), (ex, ey1, ex1), (c00, c10, c01)]):
        tri[k::5] = np.stack(t, axis=1)
    flat = (bm + tri * cell)[:T].astype(F32).reshape(-1)
    jitter = rng.integers(-1, 2, size=flat.shape)
    flat = np.where(jitter > 0, np.nextafter(flat, F32(np.inf)), np.where(jitter < 0, np.nextafter(flat, F32(-np.inf)), flat)).astype(F32)
    std = rng.random((T, 3)).astype(F32)
    ids = rng.integers(0, 4096, size=(T,)).astype(np.int64)
    return flat.reshape(T, 3, 3), std, ids
