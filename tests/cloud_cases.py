"""The point-cloud neighbourhood ops (csrc/kernels_cloud.hip.h: dif_knn, dif_remove_radius_outlier, dif_estimate_normals) stated without
the product and without oracle/: the neighbour list by exhaustive search on the float32 distance, the normal once in float64 (the statement)
and once in float32 in the kernel's order (the restatement), and the clouds both run on.  Everything here is NumPy;
tests/test_cloud_cpu.py pins it, tests/test_gpu_cloud_envelope.py holds the kernels to it.

WHAT IS STATED (reference: ext/pcproc/pcproc.cu:21-209 over cuda_kdtree.cu:1152-1240)
  knn               d2 = (dx*dx + dy*dy) + dz*dz in float32, in that order: the operation is DEFINED on the float32 distance.  Per point the k
                    smallest under the total order (d2, index), itself included, cut at d2 < float32(r) * float32(r) (strict); (-1, inf) beyond.
  accepted          the product indexes points by cells of size c = float32(r / rings) * 1.002f and takes a point only when
                    |floor(x * (1 / c))| < 2^20 - 64 on every axis (float32 throughout; NaN and Inf fail).  A point that is not accepted has
                    no neighbours and is nobody's neighbour: (-1, inf) rows, mask 0, NaN normal.  rings: 2 (kNN, normals) or 1 (outlier mask)
                    up to 131,072 points, 4 or 2 above.  So |x| <= 262,144 r is accepted by every op and |x| >= 2^20 * 1.002 r by none.
  outlier mask      the nb_points-th entry of the list is inside the radius
  normals           entries 1 .. k-1 of the list while inside the radius (the first entry outside closes it); fewer than 5 -> NaN; mean, the
                    covariance sums, the unit eigenvector of the smallest eigenvalue, flipped when dot(n, p - cam) > 0.
                    float64: numpy.linalg.eigh on the float64 covariance of the float32 coordinates.
                    float32: pcproc.cu's closed form operation for operation, sums in list order, the phase shift and its cosine in double.
"""
from __future__ import annotations

import functools
import math

import numpy as np

F32, F64 = np.float32, np.float64
CLOUD_OFF = 1 << 20
LIMIT = CLOUD_OFF - 64                 # |cell| < LIMIT on every axis
RINGS_SWITCH = 131072                  # n <= this: the sparse ring count
RINGS = dict(knn=(2, 4), normals=(2, 4), outlier=(1, 2))
GOLDEN = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1


# ---- the grid, restated (only to say which points are accepted, to place points on cell faces, and to construct collisions) --------------
def rings_of(op, n):
    return RINGS[op][0 if n <= RINGS_SWITCH else 1]


def cell_size(radius, rings):
    """-> (c, 1 / c) as the host computes them in float32"""
    c = F32(F32(radius) / F32(rings)) * F32(1.002)
    return c, F32(1.0) / c


def cells_of(pc, radius, rings):
    """-> (accepted (N,) bool, cell (N,3) int64; 0 where not accepted)"""
    _, inv_c = cell_size(radius, rings)
    with np.errstate(all="ignore"):
        f = np.floor(np.asarray(pc, F32)[:, :3] * inv_c)
        ok = (np.abs(f) < F32(LIMIT)).all(axis=1)
    return ok, np.where(ok[:, None], f, 0).astype(np.int64)


def accepted(pc, radius, op="knn"):
    return cells_of(pc, radius, rings_of(op, len(pc)))[0]


def table_size(n):
    T = 4096
    while T < 2 * max(n, 1):
        T <<= 1
    return T


def home_slot(cell, T):
    """-> (first-probe slot, the slot the probe sequence moves to when that one holds another cell) of the integer cell (cx, cy, cz) in a
    table of T slots: cloud_hash and cloud_hash2 in Python integers."""
    cx, cy, cz = (int(v) + CLOUD_OFF for v in cell)
    key = (cx << 42) | (cy << 21) | cz
    shift = 64 - (T.bit_length() - 1)
    blk = ((cx >> 3) << 36) | ((cy >> 3) << 18) | (cz >> 3)
    hb = (blk * GOLDEN) & M64
    window = (hb >> (shift + 9)) & 0xFFFFFFFF
    local = ((cx & 7) << 6) | ((cy & 7) << 3) | (cz & 7)
    rot = (hb >> 11) & 511
    return (window << 9) | ((local + rot) & 511), ((key * GOLDEN) & M64) >> shift


# ---- the neighbour list ------------------------------------------------------------------------------------------------------------------
def knn_ref(pc, k, radius, accept=None, chunk=512):
    """Exhaustive search.  -> (idx (N,k) int32, d2 (N,k) float32).  `accept`: which rows take part (default: the kNN op's own rule).
    The order (d2, index) is one unsigned compare of (bits of d2) << 32 | index: d2 is never negative and never NaN among accepted points."""
    P = np.ascontiguousarray(np.asarray(pc, F32)[:, :3])
    N = P.shape[0]
    if accept is None:
        accept = accepted(P, radius, "knn")
    idx, dist = np.full((N, k), -1, np.int32), np.full((N, k), np.inf, F32)
    cand = np.nonzero(accept)[0]
    Q = P[cand]
    r2 = F32(radius) * F32(radius)
    kk = min(k, len(cand))
    for lo in range(0, len(cand), chunk):
        q = Q[lo:lo + chunk]
        with np.errstate(over="ignore"):
            dx, dy, dz = (Q[None, :, a] - q[:, None, a] for a in range(3))
            d2 = (dx * dx + dy * dy) + dz * dz
        keys = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | cand.astype(np.uint64)[None, :]
        best = np.sort(np.partition(keys, kk - 1, axis=1)[:, :kk], axis=1)
        dsel = (best >> np.uint64(32)).astype(np.uint32).view(F32)
        isel = (best & np.uint64(0xFFFFFFFF)).astype(np.int64).astype(np.int32)
        inside = dsel < r2
        rows = cand[lo:lo + chunk]
        idx[rows, :kk] = np.where(inside, isel, -1)
        dist[rows, :kk] = np.where(inside, dsel, F32(np.inf))
    return idx, dist


def cut(knn, k, radius):
    """The list for a smaller k and a radius no larger, from a longer one: its first k entries, cut at the smaller radius."""
    idx, dist = knn
    inside = dist[:, :k] < F32(radius) * F32(radius)
    return np.where(inside, idx[:, :k], -1).astype(np.int32), np.where(inside, dist[:, :k], F32(np.inf))


def outlier_ref(pc, nb_points, radius, accept=None, knn=None):
    """mask[i]: the nb_points-th nearest point (itself included) is inside the radius.  `knn`: a list to take it from (k >= nb_points,
    radius no smaller, every point accepted by both ops)."""
    if knn is None:
        P = np.asarray(pc, F32)
        knn = knn_ref(P, nb_points, radius, accepted(P, radius, "outlier") if accept is None else accept)
    return knn[1][:, nb_points - 1] < F32(radius) * F32(radius)


# ---- normals ------------------------------------------------------------------------------------------------------------------------------
def _neighbourhoods(P, knn, radius):
    """-> (valid (N,k-1) bool: entries 1 .. k-1 while inside the radius, neighbour index (N,k-1), 0 where not valid)"""
    idx, dist = knn
    valid = np.logical_and.accumulate(dist[:, 1:] < F32(radius) * F32(radius), axis=1)
    return valid, np.where(valid, idx[:, 1:], 0)


LEN2_MIN, LEN2_MAX = F32(2.0 ** -100), F32(2.0 ** 100)


def eig32(m, with_len2=False):
    """smallest_eigenvector on a batch (N,3,3) float32, every operation rounded to float32 in the kernel's order.  with_len2: also the
    squared length of the cross product before the guard (rows below LEN2_MIN are where the reference's own formula has no answer)"""
    m = np.asarray(m, F32)
    m0x, m0y, m0z = m[:, 0, 0], m[:, 0, 1], m[:, 0, 2]
    m1x, m1y, m1z = m[:, 1, 0], m[:, 1, 1], m[:, 1, 2]
    m2x, m2y, m2z = m[:, 2, 0], m[:, 2, 1], m[:, 2, 2]
    with np.errstate(all="ignore"):
        off2 = m0y * m0y + m0z * m0z + m1z * m1z
        q = (m0x + m1y + m2z) / F32(3)
        dev2 = (m0x - q) * (m0x - q) + (m1y - q) * (m1y - q) + (m2z - q) * (m2z - q) + F32(2) * off2
        p = np.sqrt(dev2 / F32(6))
        ip = F32(1) / p
        b0x, b0y, b0z = ip * (m0x - q), ip * m0y, ip * m0z
        b1x, b1y, b1z = ip * m1x, ip * (m1y - q), ip * m1z
        b2x, b2y, b2z = ip * m2x, ip * m2y, ip * (m2z - q)
        h = b0x * b1y * b2z + b0y * b1z * b2x + b0z * b1x * b2y - b0z * b1y * b2x - b0y * b1x * b2z - b0x * b1z * b2y
        h = h / F32(2)
        phi = np.arccos(h).astype(F32) / F32(3)                          # NaN where |h| > 1 or h is NaN
        phi = np.where(h <= -1, F32(math.pi / 3.0), np.where(h >= 1, F32(0), phi)).astype(F32)
        lam = (q.astype(F64) + (F32(2) * p).astype(F64) * np.cos(phi.astype(F64) + 2 * math.pi / 3)).astype(F32)
        m0x, m1y, m2z = m0x - lam, m1y - lam, m2z - lam

        def cross(ux, uy, uz, vx, vy, vz):
            return uy * vz - uz * vy, uz * vx - ux * vz, ux * vy - uy * vx
        c01, c02, c12 = cross(m0x, m0y, m0z, m1x, m1y, m1z), cross(m0x, m0y, m0z, m2x, m2y, m2z), cross(m1x, m1y, m1z, m2x, m2y, m2z)
        n01, n02, n12 = (c[0] * c[0] + c[1] * c[1] + c[2] * c[2] for c in (c01, c02, c12))
        take02 = n02 > n01
        take12 = n12 > np.where(take02, n02, n01)
        len2 = np.where(take12, n12, np.where(take02, n02, n01))
        c = [np.where(take12, c12[a], np.where(take02, c02[a], c01[a])) for a in range(3)]
        # the kernel's guard: outside [2^-100, 2^100] the product is rescaled by 2^+-80 (exact) and its length taken again; what is still
        # outside (a zero vector, NaN) is NaN in all three components.  pcproc.cu has no such step: it returns (NaN, NaN, -Inf) and the like.
        scale = np.where(len2 < LEN2_MIN, F32(2.0 ** 80), np.where(len2 > LEN2_MAX, F32(2.0 ** -80), F32(1))).astype(F32)
        c = [v * scale for v in c]
        len2_scaled = np.where(scale != 1, c[0] * c[0] + c[1] * c[1] + c[2] * c[2], len2)
        ln = np.sqrt(len2_scaled)
        out = np.stack([v / ln for v in c], -1)
        out[~((len2_scaled >= LEN2_MIN) & (len2_scaled <= LEN2_MAX))] = np.nan
    return (out.astype(F32), len2) if with_len2 else out.astype(F32)


def dot32(n, P, cam):
    """dot(n, p - cam) in the kernel's order, float32"""
    n, d = np.asarray(n, F32), np.asarray(P, F32)[:, :3] - np.asarray(cam, F32)[None, :]
    with np.errstate(all="ignore"):
        return n[:, 0] * d[:, 0] + n[:, 1] * d[:, 1] + n[:, 2] * d[:, 2]


def normals_ref32(pc, k, radius, cam, knn=None, with_len2=False):
    P = np.ascontiguousarray(np.asarray(pc, F32)[:, :3])
    N = P.shape[0]
    knn = knn_ref(P, k, radius) if knn is None else knn
    valid, nb = _neighbourhoods(P, knn, radius)
    mean, cnt = np.zeros((N, 3), F32), np.zeros(N, F32)
    for j in range(valid.shape[1]):
        v = valid[:, j]
        mean = np.where(v[:, None], mean + P[nb[:, j]], mean)
        cnt = np.where(v, cnt + F32(1), cnt)
    with np.errstate(all="ignore"):
        mean = mean / cnt[:, None]
        cov = np.zeros((N, 3, 3), F32)
        for j in range(valid.shape[1]):
            d = P[nb[:, j]] - mean
            cov = np.where(valid[:, j, None, None], cov + d[:, :, None] * d[:, None, :], cov)
        n, len2 = eig32(cov, True)
        n = np.where((dot32(n, P, cam) > 0)[:, None], -n, n)
    n[cnt < 5] = np.nan
    return (n.astype(F32), len2) if with_len2 else n.astype(F32)


def sign_free_error(a, b):
    """per row: the largest component of a - b or of a + b, whichever is smaller (which way an eigenvector points is settled by the flip
    rule, which has no stable answer when dot(n, p - cam) is a rounding error away from 0); NaN where either row has a NaN"""
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    return np.minimum(np.abs(a - b).max(axis=1), np.abs(a + b).max(axis=1))


def normals_ref64(pc, k, radius, cam, knn=None):
    """-> dict: n64 (N,3) the unit eigenvector (NaN rows: fewer than 5 neighbours), evals (N,3) ascending, gap (N,) = (l_mid - l_min) / l_max
    (0 where l_max is 0), cnt (N,), n32 = normals_ref32, len2 (N,) = eig32's squared length before its guard, e_ref (N,) = sign_free_error(n32, n64)"""
    P = np.ascontiguousarray(np.asarray(pc, F32)[:, :3])
    knn = knn_ref(P, k, radius) if knn is None else knn
    valid, nb = _neighbourhoods(P, knn, radius)
    cnt = valid.sum(axis=1)
    w = valid[:, :, None].astype(F64)
    X = P[nb].astype(F64)                                                   # (N, k-1, 3)
    with np.errstate(all="ignore"):
        mean = (X * w).sum(axis=1) / cnt[:, None]
        D = (X - mean[:, None, :]) * w
        cov = np.einsum("nja,njb->nab", D, D)
        cov[cnt < 5] = np.eye(3)
        evals, vec = np.linalg.eigh(cov)
        n = vec[:, :, 0].copy()
        dt = (n * (P.astype(F64) - np.asarray(cam, F64)[None, :])).sum(axis=1)
        n[dt > 0] *= -1
        gap = np.where(evals[:, 2] > 0, (evals[:, 1] - evals[:, 0]) / evals[:, 2], 0.0)
    n[cnt < 5], evals[cnt < 5], gap[cnt < 5] = np.nan, np.nan, np.nan
    n32, len2 = normals_ref32(P, k, radius, cam, knn, True)
    return dict(n64=n, evals=evals, gap=gap, cnt=cnt, n32=n32, len2=len2, e_ref=sign_free_error(n32, n))


# ---- the bar of the normals ---------------------------------------------------------------------------------------------------------------
# A row is JUDGED against float64 when its gap ratio (l_mid - l_min) / l_max is at least GAP_MIN; below, the smallest eigenvector is not a
# float32 quantity (any direction in the plane of two equal eigenvalues is as good as another) and the row is held to unit length,
# orientation and "NaN or finite" only.  The bar of a judged row:
#       e_gpu <= K_N * e_ref + (U_N / gap) ulp(1)
#   U_N   what separates two honest float32 evaluations of the closed form that differ only in acosf (1 ulp in the HIP math API's table,
#         against the libm of the restatement): phi = acos / 3 moves by at most ulp(acos <= pi) / 3 + ulp(phi) / 2 < 2^-23; lambda = q + 2 p
#         cos(phi + 2 pi / 3) by at most 2 p 2^-23 <= (2 / 3) l_max 2^-23 (p <= l_max / 3 for a positive semi-definite matrix), and one more
#         ulp(l_max) when that moves the rounding of lambda: below 2 l_max 2^-23 together.  A shift d of lambda turns the eigenvector of
#         (M - lambda I) by d / (l_mid - l_min) = 2 ulp(1) / gap.  U_N = 4 is twice that.  For every judged row U_N / gap <= 4 / GAP_MIN.
#   K_N   twice the largest e_gpu / e_ref measured on the GPU over all cases (tests/test_gpu_cloud_envelope.py prints it; its header
#         carries the figure).
#   GAP_MIN is chosen on the CPU (test_cloud_cpu.py::test_gap_threshold_and_e_ref): the share of rows below it stays under 1 % on the
#         non-degenerate kinds (0.04 %), and the restatement has a finite normal on every row at or above it.
GAP_MIN = 1e-2
U_N = 4.0
K_N = 2.0
ULP1 = float(np.spacing(F32(1.0)))           # 2^-23
UNIT_ULPS = 4                                # | |n| - 1 |: three squares, two sums, a square root and three divisions, each half an ulp


def normal_bar(e_ref, gap):
    with np.errstate(all="ignore"):
        return K_N * e_ref + U_N / gap * ULP1


# ---- clouds -------------------------------------------------------------------------------------------------------------------------------
R_KNN, R_OUT = 0.1, 0.05                     # the tracker's own radii (tracker.py:105-113): both give cells of 0.0501
N_SWEEP = 700                                # three workgroups of 256, the last one partly filled
OFFSET_CELLS = (1 << 10, 1 << 13, 1 << 15, 1 << 17, 1 << 19)
KINDS = ("box", "plane_axis", "plane_tilt", "line", "lattice", "sheet")
NON_DEGENERATE = ("box", "plane_tilt", "sheet")          # kinds whose neighbourhoods have a normal to speak of


def base_cloud(kind, n=N_SWEEP, seed=0):
    """(n, 3) float32 near the origin.  Densities put well over 32 points inside R_KNN of most points, so that the k-th distance prunes."""
    g = np.random.default_rng(1000 * KINDS.index(kind) + seed)
    if kind == "box":
        p = g.uniform(-0.2, 0.2, (n, 3))
    elif kind == "plane_axis":                             # exactly coplanar: z = 0, and still exactly coplanar after a translation
        p = np.concatenate([g.uniform(-0.25, 0.25, (n, 2)), np.zeros((n, 1))], 1)
    elif kind == "plane_tilt":                             # a tilted plane with 1 mm of noise
        u, v = np.array([0.8, 0.0, -0.3]), np.array([0.15, 0.8, 0.4])
        nrm = np.cross(u, v) / np.linalg.norm(np.cross(u, v))
        ab = g.uniform(-0.3, 0.3, (n, 2))
        p = ab[:, :1] * u + ab[:, 1:] * v + g.standard_normal((n, 1)) * 1e-3 * nrm
    elif kind == "line":                                   # collinear along x: two of the three box gaps of every cell on the line are 0
        p = np.concatenate([g.uniform(-1.0, 1.0, (n, 1)), np.zeros((n, 2))], 1)
    elif kind == "lattice":                                # 8^3 points 2 cm apart and exact duplicates of some: ties at 0 and on every shell
        a = np.arange(8)
        lat = np.stack(np.meshgrid(a, a, a, indexing="ij"), -1).reshape(-1, 3).astype(F32) * F32(0.02)
        return np.concatenate([lat, lat[g.integers(0, len(lat), n - len(lat))]]).astype(F32)
    elif kind == "sheet":                                  # what a depth image back-projects to: a pixel grid on a curved surface
        m = int(math.ceil(math.sqrt(n)))
        x, y = (v.reshape(-1)[:n] for v in np.meshgrid((np.arange(m) - m / 2) * 0.02, (np.arange(m) - m / 2) * 0.02))
        z = 0.08 * np.sin(4.0 * x) + 0.05 * np.cos(3.0 * y) + g.standard_normal(n) * 2e-3
        p = np.stack([x * (1 + 0.3 * z), y * (1 + 0.3 * z), z], 1)
    else:
        raise KeyError(kind)
    return p.astype(F32)


def offsets():
    """[(name, (mx, my, mz) in cells)]: none, and +- each magnitude along x alone and along all three axes"""
    out = [("0", (0, 0, 0))]
    for m in OFFSET_CELLS:
        for s in (1, -1):
            out.append((f"{'+' if s > 0 else '-'}2^{m.bit_length() - 1}x", (s * m, 0, 0)))
            out.append((f"{'+' if s > 0 else '-'}2^{m.bit_length() - 1}xyz", (s * m, s * m, -s * m if m == 1 << 13 else s * m)))
    return out


def translate(pc, cells, radius=R_KNN, rings=2):
    """pc + float32(cells * c), the sum rounded to float32 (far from the origin the cloud snaps to the float32 lattice there)"""
    c, _ = cell_size(radius, rings)
    t = (np.asarray(cells, F64) * F64(c)).astype(F32)
    out = np.asarray(pc, F32).copy()
    out[:, :3] += t[None, :]
    return out


@functools.lru_cache(maxsize=None)
def sweep(kind):
    """[(name, cloud (N_SWEEP,3), its k = 32 list at R_KNN)] over offsets(): computed once, shared, not modified by callers"""
    out = []
    for name, cells in offsets():
        pc = translate(base_cloud(kind), cells)
        assert accepted(pc, R_KNN, "knn").all() and accepted(pc, R_OUT, "outlier").all()
        out.append((f"{kind} {name}", pc, knn_ref(pc, 32, R_KNN)))
    return out


def face_cloud(cells, seed=0):
    """Points planted ON cell faces: every coordinate float32(m) * c (the product a cell's edge is computed as) for m in -2 .. 2 around
    `cells`, that value's two float32 neighbours, and around 0 both zeros; 500 random points around them."""
    g = np.random.default_rng(77 + seed)
    c, _ = cell_size(R_KNN, 2)
    vals = []
    for ax in range(3):
        v = []
        for m in range(-2, 3):
            e = F32(cells[ax] + m) * c
            v += [e, np.nextafter(e, F32(-np.inf)), np.nextafter(e, F32(np.inf))]
        if cells[ax] == 0:
            v += [F32(-0.0), F32(0.0)]
        vals.append(np.array(v, F32))
    pts = np.stack([vals[a][g.integers(0, len(vals[a]), 200)] for a in range(3)], 1)
    pts[:len(vals[0])] = np.stack([vals[0], vals[1][:len(vals[0])], vals[2][:len(vals[0])]], 1)       # each planted value at least once per axis
    return np.concatenate([pts, translate(g.uniform(-0.12, 0.12, (500, 3)).astype(F32), cells)]).astype(F32)


def limit_cloud(sign=1, stride=3, radius=R_KNN, rings=2):
    """Clusters just inside the accepted range at +-(LIMIT - 1.5) c on x (60 points, all accepted, asserted by the caller) and around the
    origin (200 points), with rows that are not accepted: a cluster at +-(LIMIT + 1.5) c, NaN, +-Inf and 3e38 in each column.  stride 4: a
    fourth column of NaN.  -> (cloud, index of the first refused row)"""
    g = np.random.default_rng(5 + (sign > 0))
    c, _ = cell_size(radius, rings)
    near = g.uniform(-0.15, 0.15, (200, 3)).astype(F32)
    spread = np.concatenate([g.uniform(-0.4, 0.4, (60, 1)), g.uniform(-0.05, 0.05, (60, 2))], 1) * F64(c)
    inside = (spread + np.array([sign * (LIMIT - 1.5) * F64(c), 0, 0])).astype(F32)
    outside = (spread[:20] + np.array([sign * (LIMIT + 1.5) * F64(c), 0, 0])).astype(F32)
    bad = np.tile(near[:12].copy(), (1, 1))
    for i, v in enumerate((np.nan, np.inf, -np.inf, 3e38)):
        for a in range(3):
            bad[3 * i + a, a] = v
    pc = np.concatenate([near, inside, outside, bad]).astype(F32)
    if stride == 4:
        pc = np.concatenate([pc, np.full((len(pc), 1), np.nan, F32)], 1)
    return np.ascontiguousarray(pc), len(near) + len(inside)


def tie_lattice():
    """5^3 points 0.5 apart with radius 1: an interior point has 27 points at d2 < 1 (0, 0.25 x 6, 0.5 x 12, 0.75 x 8) and six at
    d2 == 1.0f == r * r, bit for bit (every coordinate and every product is exact).  -> (cloud, radius)"""
    a = np.arange(-2, 3)
    return (np.stack(np.meshgrid(a, a, a, indexing="ij"), -1).reshape(-1, 3) * 0.5).astype(F32), 1.0


def _blocks_in_one_window(T, want=3, span=12):
    """`want` 8 x 8 x 8 blocks whose cells share one 512-slot window of a T-slot table, (0, 0, 0) first, no two of them adjacent"""
    w0 = home_slot((0, 0, 0), T)[0] >> 9
    found = [(0, 0, 0)]
    for bx in range(-span, span + 1):
        for by in range(-span, span + 1):
            for bz in range(-span, span + 1):
                b = (bx, by, bz)
                if all(max(abs(b[a] - f[a]) for a in range(3)) >= 2 for f in found) and home_slot((8 * bx, 8 * by, 8 * bz), T)[0] >> 9 == w0:
                    found.append(b)
                    if len(found) == want:
                        return found
    raise RuntimeError("no such blocks")


def collision_cloud(n_per_block=400, seed=3):
    """Points in three blocks of cells that hash to the same window: many occupied cells share their home slot with a cell of another
    block, so inserts and look-ups go through the second hash and the linear walk.  -> (cloud, dict of what was constructed:
    T, colliding (occupied cells whose home slot another occupied cell also has), empty_probes (empty cells within 2 rings of an occupied
    one whose home slot is occupied))"""
    g = np.random.default_rng(seed)
    c, _ = cell_size(R_KNN, 2)
    n = 3 * n_per_block
    T = table_size(n)
    blocks = _blocks_in_one_window(T)
    pts = [(g.uniform(0.02, 7.98, (n_per_block, 3)) + 8.0 * np.array(b)) * F64(c) for b in blocks]
    pc = np.concatenate(pts).astype(F32)
    ok, cell = cells_of(pc, R_KNN, 2)
    assert ok.all()
    occ = {tuple(int(v) for v in r) for r in cell}
    by_slot = {}
    for cc in occ:
        by_slot.setdefault(home_slot(cc, T)[0], []).append(cc)
    colliding = sum(len(v) for v in by_slot.values() if len(v) > 1)
    empty_probes, seen = 0, set()
    for cc in list(occ)[:200]:
        for d in ((1, 0, 0), (-1, 0, 0), (0, 2, 0), (0, -1, 1), (2, 2, -2), (0, 0, -1)):
            e = (cc[0] + d[0], cc[1] + d[1], cc[2] + d[2])
            if e not in occ and e not in seen and home_slot(e, T)[0] in by_slot:
                seen.add(e)
                empty_probes += 1
    return pc, dict(T=T, blocks=blocks, cells=len(occ), colliding=colliding, empty_probes=empty_probes)


def degenerate_clouds():
    """name -> (cloud, k, radius): neighbourhoods in which p = 0, 1 / p and a zero-length cross product decide the outcome.  Coordinates
    are multiples of 2^-6 below 1, so every sum, mean, difference and product of the covariance is exact in float32."""
    s = F32(1.0 / 64)
    a = np.arange(6)
    plane = np.stack(np.meshgrid(a, a, indexing="ij"), -1).reshape(-1, 2)
    out = {}
    out["coplanar"] = (np.concatenate([plane * s, np.full((36, 1), 0.5)], 1).astype(F32), 16, 0.1)
    out["collinear"] = (np.stack([np.arange(24) * s, np.full(24, 0.25), np.full(24, -0.5)], 1).astype(F32), 8, 0.1)
    out["coincident"] = (np.tile(np.array([[0.25, -0.5, 0.75]], F32), (12, 1)), 8, 0.1)
    # the eight corners of a cube around a ninth point, and the same around eight more centres (every centre sees exactly its own corners)
    corners = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], F64) * float(s)
    centres = np.array([[i, 0, 0] for i in range(9)], F64)
    out["isotropic"] = (np.concatenate([np.concatenate([cc[None], cc[None] + corners]) for cc in centres]).astype(F32), 9, 0.04)
    return out


def count_clusters(radius=R_KNN, seed=11):
    """Three clusters 10 radii apart with 5, 6 and 7 points (4, 5 and 6 neighbours inside the radius for each of them), each within a
    third of the radius.  -> (cloud, neighbours per row)"""
    g = np.random.default_rng(seed)
    pts, cnt = [], []
    for i, m in enumerate((5, 6, 7)):
        pts.append(g.uniform(-radius / 6, radius / 6, (m, 3)) + np.array([10 * radius * i, 0.3, -0.2]))
        cnt += [m - 1] * m
    return np.concatenate(pts).astype(F32), np.array(cnt)
