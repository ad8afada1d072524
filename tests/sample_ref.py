"""numpy restatement of the surface sampler of an indexed mesh (`dif_mesh_sampler_build`, `dif_mesh_sample`, di_fusion_amd/system/mesh.py), written
from the operator's contract (include/difusion.h, DESIGN.md "Sampling an indexed mesh"), not from the kernels: float64 for the doubled areas (every
operation rounded once, as on the device: the library is built without contraction), uint64 with wrap-around for the weights, their prefix sums,
the strata and the hash, float32 for the point.  Vectorised.  The GPU tests hold the kernels to it byte for byte; tests/test_sample_cpu.py holds it
to properties that do not come from any code under test.
"""
import numpy as np

F32 = np.float32
F64 = np.float64
U64 = np.uint64
ABS_LIMIT = F32(2.0 ** 60)           # |coordinate| stays below this (the closest operator's limit)
ONE = 1 << 24                        # the barycentrics are integers over this
BAD_INDEX = 1                        # the status bit
BUILD_NAMES = ("weighted", "weightless", "skipped", "bad_index", "exponent", "status")
SAMPLE_NAMES = ("samples", "status")
QUIET_NAN = np.array([0x7FC00000], dtype=np.uint32).view(F32)[0]


def mix(z):
    """splitmix64 on a uint64 array (or scalar)"""
    with np.errstate(over="ignore"):
        z = np.asarray(z, dtype=U64) + U64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
        return z ^ (z >> U64(31))


def doubled_areas(vertices, triangles):
    """-> (n (K,) f64: |e1 x e2|, 0 for a triangle that is not usable; bad (K,) bool; skipped (K,) bool)"""
    v = np.ascontiguousarray(vertices, dtype=F32).reshape(-1, 3)
    tri = np.ascontiguousarray(triangles, dtype=np.int32).reshape(-1, 3).astype(np.int64)
    V, K = v.shape[0], tri.shape[0]
    bad = ~((tri >= 0) & (tri < V)).all(axis=1)
    p = v[np.where(bad[:, None], 0, tri)] if V else np.zeros((K, 3, 3), dtype=F32)          # (K, corner, axis)
    with np.errstate(all="ignore"):
        skipped = ~bad & ~(np.abs(p) < ABS_LIMIT).all(axis=(1, 2))                           # (NaN fails)
        d = p.astype(F64)
        e1, e2 = d[:, 1] - d[:, 0], d[:, 2] - d[:, 0]
        cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        n = np.sqrt((cx * cx + cy * cy) + cz * cz)
    return np.where(bad | skipped, 0.0, n), bad, skipped


def build(vertices, triangles):
    """-> dict(n, w (K,) u64, prefix (K,) u64, total (int), exponent, counts (list, BUILD_NAMES), bad, skipped)"""
    n, bad, skipped = doubled_areas(vertices, triangles)
    K = n.shape[0]
    m = float(n.max()) if K else 0.0
    e = int(np.frexp(m)[1])
    w = np.floor(np.ldexp(n, 32 - e)).astype(U64)
    prefix = np.cumsum(w, dtype=U64)
    total = int(prefix[-1]) if K else 0
    weighted = int((w > 0).sum())
    counts = [weighted, K - weighted - int(bad.sum()) - int(skipped.sum()), int(skipped.sum()), int(bad.sum()), e, BAD_INDEX if bad.any() else 0]
    return dict(n=n, w=w, prefix=prefix, total=total, exponent=e, counts=counts, bad=bad, skipped=skipped)


def area(b):
    """0.5 T 2^(e - 32)"""
    return float(np.ldexp(float(b["total"]), b["exponent"] - 33))


def strata(total, N):
    """-> (lo (N,) u64, width (N,) u64): stratum j = [b(j), b(j + 1)) with b(j) = q j + (r j) div N"""
    T, n = U64(total), U64(N)
    q, r = T // n, T % n
    j = np.arange(N + 1, dtype=U64)
    b = q * j + (r * j) // n
    return b[:-1], b[1:] - b[:-1]


def draws(N, seed):
    """-> (r0 (N,) u64, r1 (N,) u64)"""
    base = mix(U64(int(seed) & (2 ** 64 - 1)))
    j = np.arange(N, dtype=U64)
    return mix(base ^ mix(U64(2) * j)), mix(base ^ mix(U64(2) * j + U64(1)))


def sample(vertices, triangles, N, seed=0, b=None):
    """-> dict(point (N,3) f32, triangle (N,) i32, barycentric (N,3) f32, counts (list, SAMPLE_NAMES), build)"""
    v = np.ascontiguousarray(vertices, dtype=F32).reshape(-1, 3)
    tri = np.ascontiguousarray(triangles, dtype=np.int32).reshape(-1, 3)
    b = build(v, tri) if b is None else b
    status = b["counts"][5]
    if b["total"] == 0 or N == 0:
        return dict(point=np.full((N, 3), QUIET_NAN, dtype=F32), triangle=np.full((N,), -1, dtype=np.int32),
                    barycentric=np.full((N, 3), QUIET_NAN, dtype=F32), counts=[N if b["total"] else 0, status], build=b)
    lo, width = strata(b["total"], N)
    assert (width >= U64(1)).all()
    r0, r1 = draws(N, seed)
    target = lo + r0 % width
    chosen = np.searchsorted(b["prefix"], target, side="right")                              # the first i with P[i] > t
    u = (r1 >> U64(40)).astype(np.int64)
    w = ((r1 >> U64(16)) & U64(0xFFFFFF)).astype(np.int64)
    fold = u + w > ONE
    u, w = np.where(fold, ONE - u, u), np.where(fold, ONE - w, w)
    bary = np.stack([(ONE - u - w).astype(F32) / F32(ONE), u.astype(F32) / F32(ONE), w.astype(F32) / F32(ONE)], axis=1)
    p = v[tri[chosen].astype(np.int64)]                                                      # (N, corner, axis)
    point = (bary[:, 0, None] * p[:, 0] + bary[:, 1, None] * p[:, 1]) + bary[:, 2, None] * p[:, 2]
    assert bary.dtype == F32 and point.dtype == F32
    return dict(point=point, triangle=chosen.astype(np.int32), barycentric=bary, counts=[N, status], build=b)


def interpolate(triangles, triangle, barycentric, values):
    """`mesh.interpolate`: (b0 x0 + b1 x1) + b2 x2 in float32, NaN where triangle < 0"""
    x = np.asarray(values, dtype=F32)[np.asarray(triangles)[np.maximum(triangle, 0)].astype(np.int64)]
    bb = barycentric if x.ndim == 2 else barycentric[:, :, None]
    out = (bb[:, 0] * x[:, 0] + bb[:, 1] * x[:, 1]) + bb[:, 2] * x[:, 2]
    found = triangle >= 0
    return np.where(found if out.ndim == 1 else found[:, None], out, QUIET_NAN).astype(F32)
