"""Seeded maps, clouds and per-point rows for the envelope tests of the tracker's SDF term (tests/test_track_cpu.py on the CPU, which asserts
what the generators promise; tests/test_gpu_track_envelope.py on the GPU).  TEST INFRASTRUCTURE ONLY; everything is a deterministic function
of its seed.  The map is seq_small's (8^3 voxels of 0.4 m) with planted latents (tests/mlp_cases.py)."""
from __future__ import annotations

import numpy as np

from oracle import difusion_oracle as O
from tests import mlp_cases as C
from tests import track_ref as T

F = np.float32
SCALES = (0.3, 4.0)
IDENTITY = (np.eye(3), np.zeros(3))
# kinds of cloud points
INSIDE, INSIDE_POSED, FACE_ID, FACE_POSED, OUTER, UNALLOCATED, FAR, NONFINITE = range(8)


def pose():
    """The posed call's last_pose . delta: 0.27 rad about a skew axis, 0.17 m."""
    g = np.random.default_rng(41)
    phi, rho = g.standard_normal(3), g.standard_normal(3)
    return O.twist_exp(np.concatenate([rho / np.linalg.norm(rho) * 0.17, phi / np.linalg.norm(phi) * 0.27]))


def split_pose():
    """(last, delta) with last . delta == pose() to rounding: delta a small step (6 cm / 3 degrees, like the tracker's), last the rest."""
    g = np.random.default_rng(42)
    dR, dt = O.twist_exp(np.concatenate([g.uniform(-0.035, 0.035, 3), g.uniform(-0.03, 0.03, 3)]))
    R, t = pose()
    lR = R @ dR.T
    return (lR, t - lR @ dt), (dR, dt)


def ulp_shift(v, k):
    """float32 `v` moved by `k` representable values (finite values away from the overflow threshold)."""
    i = np.ascontiguousarray(v, dtype=F).view(np.int32).astype(np.int64)
    i = np.where(i < 0, -(i & 0x7FFFFFFF), i) + k
    return np.where(i < 0, (-i) | 0x80000000, i).astype(np.uint32).view(F)


def gate_edits(om, n):
    """Six voxels whose count is set to exactly ignore_count_th (three: not valid, the gate is `>`) and to its float32 successor (three)."""
    g = np.random.default_rng(43)
    slots = g.choice(n, size=6, replace=False)
    th = F(om.ignore_count_th)
    om.voxel_obs_count[slots[:3]] = th
    om.voxel_obs_count[slots[3:]] = np.nextafter(th, F(np.inf))
    return slots[:3], slots[3:]


def track_map(oracle, ws_seed: int, scale: float):
    """mlp_cases.planted_oracle_map with the count gate's edits -> (OracleMap, n_occupied, latents, frames, (slots at th, slots above))"""
    om, n, lat, frames = C.planted_oracle_map(oracle, ws_seed, scale)
    return om, n, lat, frames, gate_edits(om, n)


def _in_voxel(g, om, ijk):
    return (ijk + 0.05 + 0.9 * g.random(ijk.shape)) * om.voxel_size + om.bound_min.astype(np.float64)[None, :]


def _unpose(Tc, q):
    return (q - np.asarray(Tc[1])[None, :]) @ np.asarray(Tc[0])          # R^T (q - t), float64


def _xn_axis(om, Tc, p, a):
    with np.errstate(all="ignore"):
        return T.posed_xn(om, p, Tc)[1][:, a]


def face_planes(om, axis):
    """float32 of bound_min + j * voxel_size in float64, j = 0 .. n"""
    return (float(om.bound_min[axis]) + np.arange(om.n_xyz[axis] + 1) * float(F(om.voxel_size))).astype(F)


def _face_identity(g, om, n, span=4):
    """Per axis and plane j: the float32 neighbours -span .. span of bound_min + j * voxel_size as the axis coordinate, the other two inside an
    occupied voxel that touches the plane (when there is one)."""
    occ = om._unlinearize_id(om.latent_vecs_pos[:n])
    pts, axis, plane = [], [], []
    for a in range(3):
        for j, v in enumerate(face_planes(om, a)):
            touch = occ[(occ[:, a] == j - 1) | (occ[:, a] == j)]
            for off in range(-span, span + 1):
                ijk = touch[g.integers(0, len(touch))] if len(touch) else g.integers(0, om.n_xyz[0], size=3)
                p = _in_voxel(g, om, ijk[None, :].astype(np.float64))[0].astype(F)
                p[a] = ulp_shift(np.array([v], dtype=F), off)[0]
                pts.append(p); axis.append(a); plane.append(j)
    return np.array(pts, dtype=F), np.array(axis), np.array(plane)


def _face_posed(g, om, n, Tc, per_axis=256, reach=8):
    """Points whose POSED coordinate lies within a few float32 steps of a face of an occupied voxel: the pre-image of a point on the face,
    rounded to float32, then moved by up to `reach` representable values in two of its coordinates until the float32 pose (pose_row's order)
    puts it just below the face, exactly on it, or just above (a third of the points each; the nearest such neighbour wins)."""
    occ = om._unlinearize_id(om.latent_vecs_pos[:n])
    d = np.arange(-reach, reach + 1)
    d1, d2 = (x.reshape(-1) for x in np.meshgrid(d, d, indexing="ij"))
    order = np.argsort(np.abs(d1) + np.abs(d2), kind="stable")
    d1, d2 = d1[order], d2[order]
    pts, axis, plane = [], [], []
    R = np.asarray(Tc[0])
    for a in range(3):
        v = occ[g.integers(0, n, size=per_axis)]
        j = v[:, a] + g.integers(0, 2, size=per_axis)
        q = _in_voxel(g, om, v.astype(np.float64))
        q[:, a] = float(om.bound_min[a]) + j * float(F(om.voxel_size))
        p0 = _unpose(Tc, q).astype(F)
        c = np.argsort(-np.abs(R[a]))[:2]                                 # the two coordinates the posed axis depends on most
        cand = np.repeat(p0[:, None, :], d1.size, axis=1)
        cand[:, :, c[0]] = ulp_shift(cand[:, :, c[0]], d1[None, :])
        cand[:, :, c[1]] = ulp_shift(cand[:, :, c[1]], d2[None, :])
        xn = _xn_axis(om, Tc, cand.reshape(-1, 3), a).reshape(per_axis, -1)
        jj = j.astype(F)[:, None]
        want = np.arange(per_axis) % 3
        hit = np.stack([(xn < jj) & (np.ceil(xn) == jj), xn == jj, (xn > jj) & (np.ceil(xn) == jj + 1)])[want, np.arange(per_axis)]
        first = np.where(hit.any(axis=1), hit.argmax(axis=1), 0)
        pts.append(cand[np.arange(per_axis), first]); axis.append(np.full(per_axis, a)); plane.append(j)
    return np.concatenate(pts).astype(F), np.concatenate(axis), np.concatenate(plane)


_CLOUD = {}


def cloud():
    """-> (xyz (N,3) float32, kind (N,), axis (N,), plane (N,): of face points, else -1).  About 2k points, shuffled; the same for every weight
    set and latent scale (the occupied voxels and the gate's edits depend on seq_small's frames only)."""
    if "c" in _CLOUD:
        return _CLOUD["c"]
    om, n, _, _, _ = track_map(O.OracleNetworks(C.weight_set("shipped")), 0, 0.3)
    g = np.random.default_rng(44)
    Tc = pose()
    occ = om._unlinearize_id(om.latent_vecs_pos[:n]).astype(np.float64)
    parts = []

    def add(kind, p, axis=None, plane=None):
        p = np.asarray(p, dtype=F).reshape(-1, 3)
        parts.append((p, np.full(len(p), kind), np.full(len(p), -1) if axis is None else axis, np.full(len(p), -1) if plane is None else plane))

    add(INSIDE, _in_voxel(g, om, occ[g.integers(0, n, size=500)]))
    add(INSIDE_POSED, _unpose(Tc, _in_voxel(g, om, occ[g.integers(0, n, size=500)])))
    add(FACE_ID, *_face_identity(g, om, n))
    add(FACE_POSED, *_face_posed(g, om, n, Tc))
    # the grid's outer faces, both sides: xn = 0 (outside) and its successor, xn = n (inside) and its successor
    for a in range(3):
        lo, hi = face_planes(om, a)[[0, -1]]
        for v in (lo, np.nextafter(lo, F(np.inf)), np.nextafter(lo, F(-np.inf)), hi, np.nextafter(hi, F(np.inf)), np.nextafter(hi, F(-np.inf))):
            p = _in_voxel(g, om, occ[g.integers(0, n, size=2)]).astype(F)
            p[:, a] = v
            add(OUTER, p, np.full(2, a), np.full(2, 0 if v <= np.nextafter(lo, F(np.inf)) else om.n_xyz[a]))
    free = np.nonzero(om.indexer < 0)[0]
    add(UNALLOCATED, _in_voxel(g, om, om._unlinearize_id(free[g.integers(0, len(free), size=100)]).astype(np.float64)))
    add(FAR, np.concatenate([g.uniform(-50, 50, (24, 3)), g.uniform(-1e30, 1e30, (8, 3)), g.uniform(-3.3, 3.3, (24, 3))]))
    bad = _in_voxel(g, om, occ[g.integers(0, n, size=9)]).astype(F)
    for i, val in enumerate((np.nan, np.inf, -np.inf)):
        for c in range(3):
            bad[3 * i + c, c] = val
    add(NONFINITE, bad)
    xyz, kind, axis, plane = (np.concatenate([p[i] for p in parts]) for i in range(4))
    perm = g.permutation(len(xyz))
    _CLOUD["c"] = (np.ascontiguousarray(xyz[perm]), kind[perm], axis[perm].astype(np.int64), plane[perm].astype(np.int64))
    return _CLOUD["c"]


def voxel_valid(om, ix):
    """(K,3) integer voxel ids -> (K,) bool: inside the grid, allocated, count over the gate"""
    ix = np.asarray(ix, dtype=np.int64)
    ok = np.all((ix >= 0) & (ix < np.asarray(om.n_xyz)[None, :]), axis=1)
    slot = np.where(ok, om.indexer[om._linearize_id(np.where(ok[:, None], ix, 0))], -1)
    ok = slot >= 0
    ok[ok] = om.voxel_obs_count[slot[ok]] > F(om.ignore_count_th)
    return ok


def face_report(om, xyz, axis, plane, Tc):
    """For face points under pose Tc -> (side (K,): -1 below the face / 0 exactly on it / +1 above, as the float32 rule sees it; 2: further
    than one voxel; valid_low, valid_high: whether the voxel below / above the face, the other two indices being the point's own, is valid)."""
    _, xn = T.posed_xn(om, xyz, Tc)
    k = np.arange(len(xyz))
    xa, j = xn[k, axis], plane.astype(F)
    side = np.where(xa == j, 0, np.where((xa < j) & (np.ceil(xa) == j), -1, np.where((xa > j) & (np.ceil(xa) == j + 1), 1, 2)))
    ix = np.ceil(xn).astype(np.int64) - 1
    lo, hi = ix.copy(), ix.copy()
    lo[k, axis], hi[k, axis] = plane - 1, plane
    return side, voxel_valid(om, lo), voxel_valid(om, hi)


# ---- rows for the reduction alone ---------------------------------------------------------------------------------------------------------
def crafted_rows():
    """Rows on the robust kernels' thresholds: std a power of two, sdf = +-k std and its float32 neighbours, so that s = sdf / std is exactly
    +-k, one step inside, one step outside.  -> (sdf, std, expected s) for every k of track_ref.KERNELS"""
    sdf, std, s = [], [], []
    for _, k in T.KERNELS[1:]:
        for sd in (F(0.25), F(0.5), F(2.0)):
            for sign in (F(1), F(-1)):
                for off in (-1, 0, 1):
                    sk = ulp_shift(np.array([k], dtype=F), off)[0]
                    sdf.append(sign * sk * sd); std.append(sd); s.append(sign * sk)
    return np.array(sdf, dtype=F), np.array(std, dtype=F), np.array(s, dtype=F)


def reduce_rows(N: int, seed: int = 45):
    """Per-point views for k_sdf_hg_reduce alone: (sdf (N,), std (N,), grad (N,3), obs (N,3)) float32.  About 30 % of the rows have std == 0 and
    NaN in sdf and grad (they must not reach the sums); the crafted rows sit at the front and again at the very end (the loop's tail)."""
    g = np.random.default_rng([seed, N])
    std = np.exp2(g.uniform(-4.3, 1.0, size=N)).astype(F)
    sdf = (g.standard_normal(N) * std.astype(np.float64) * 1.2).astype(F)
    grad = (g.standard_normal((N, 3)) * 2.5).astype(F)
    obs = g.uniform(-2.0, 2.0, size=(N, 3)).astype(F)
    c_sdf, c_std, _ = crafted_rows()
    nc = len(c_sdf)
    if N >= nc:
        sdf[:nc], std[:nc] = c_sdf, c_std
    dead = g.random(N) < 0.30
    dead[:nc] = False
    if N >= 3 * nc:
        sdf[N - nc:], std[N - nc:] = c_sdf, c_std
        dead[N - nc:] = False
    std[dead] = 0
    sdf[dead] = np.nan
    grad[dead] = np.nan
    return sdf, std, grad, obs
