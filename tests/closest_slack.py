"""Adversarial cases for the two margins of the closest-point search (csrc/kernels_closest.hip.h: the query's `slack`, the registration's
widening), and a numpy statement of the search's box test and ring bound with either margin switched off — so that a test can PROVE, on the
CPU, that its cases are answered wrongly without the margins (tests/test_closest_cpu.py) before the GPU is held to the all-pairs answer on
them (tests/test_gpu_closest.py).

Every case is built constructively at coordinates near 1000 (x) or 3000 (y), where a float32 ulp is 6e-5 / 2.4e-4 and the membership rounding
of a cell — floor(fl(x * fl(1 / c))) — reaches an ulp: a float X0 that is BELOW the computed edge fl(j c) of cell j and still a member of
cell j (one j in four has one).  A small triangle T lies in the plane (axis = X0): its computed closest point has exactly that coordinate,
so T's own box lies in cell j only.  The query sits d = 0.4 c below X0 in cell j - 1, facing T's interior; a second triangle T2, in the
query's own cell on the other side, is farther than T by HALF the gap between d^2 and the squared computed distance to the edge of cell j.
With neither margin, cell j's box test fails against T2's d2, and T — the true answer — is never seen.

What cannot be planted, and why.  (1) Either margin alone answers these cases: the widening (16 u m) registers T in cell j - 1 as well, the
slack (8 u m') reaches over the ulp between X0 and the edge.  The two margins stand in series in the proof and overlap in effect; `search`
below shows it (0 wrong with one of them off, all wrong with both off), and the test asserts only what it can prove: both off fails.
(2) A case for the RING bound: it needs a query and a closest point in cells two apart and less than c apart.  Membership is a monotonic
function with period c on the float grid, so such a pair is at least c apart up to the rounding of fl(x * inv_c) — less than an ulp of the
coordinates: a scan of 3,000 cells at either magnitude finds none.  The ring bound shares `slack` with the box test.
"""
import numpy as np

from tests import closest_ref as R

F32 = np.float32
LOC_NB = 16


def ulps(x, n):
    x = F32(x)
    for _ in range(abs(n)):
        x = np.nextafter(x, F32(np.inf if n > 0 else -np.inf))
    return x


def cell_coord(x, inv_c):
    return int(np.floor(F32(x) * inv_c))


def stray_members(j, c, inv_c, sgn):
    """Floats on the wrong side of the computed edge fl(j c) that are members of the cell on the other side all the same.  sgn = +1: below the
    edge and a member of cell j (positive coordinates: fl(1 / c) c > 1 here); sgn = -1: above the edge and a member of cell j - 1 (negative
    coordinates).  -> [X0]"""
    e = F32(j) * c
    home = j if sgn > 0 else j - 1
    return [ulps(e, -sgn * a) for a in (1, 2, 3) if cell_coord(ulps(e, -sgn * a), inv_c) == home]


def _plane_triangle(axis, x0, centre, s=0.004):
    """Three vertices in the plane (axis = x0) around `centre` (the other two coordinates)."""
    o = [k for k in range(3) if k != axis]
    out = np.zeros((3, 3), dtype=F32)
    for row, (du, dv) in enumerate(((-s, -s), (s, -s), (0.0, s))):
        out[row, axis] = x0
        out[row, o[0]] = F32(centre[0] + du)
        out[row, o[1]] = F32(centre[1] + dv)
    return out


def _point(axis, x, centre):
    o = [k for k in range(3) if k != axis]
    p = np.zeros(3, dtype=F32)
    p[axis], p[o[0]], p[o[1]] = x, centre[0], centre[1]
    return p


def _d2(q, tri):
    return F32(R.evaluate(tuple(q), tuple(tri[0]), tuple(tri[1]), tuple(tri[2]), full=False))


def planted_cases(cell=0.05, per_axis=40):
    """-> vertices (6 n, 3), triangles (2 n, 3) — T before T2 in half of the cases, after it in the others —, queries (n, 3)."""
    c = F32(cell)
    inv_c = F32(1) / c
    vs, qs = [], []
    S = 0.004
    for axis, start, flat in ((0, int(1000 / cell), -3000.5), (1, int(3000 / cell), 1000.0)):
        found = 0
        for j in range(start, start + 4000, 9):                                  # nine cells apart: no case sees another within max_distance
            e = F32(j) * c
            for x0 in stray_members(j, c, inv_c, 1)[-1:]:                           # the one farthest beyond the edge
                level = F32(0.5 + 0.5 * len(qs))                                 # and every case on a level of its own
                centre = (flat, level)
                t = _plane_triangle(axis, x0, centre, S)
                qx = F32(x0 - F32(0.4) * c)
                if cell_coord(qx, inv_c) != j - 1:
                    continue
                bound2 = (e - qx) * (e - qx)                                      # the box test of T's cell without slack
                q = _point(axis, qx, centre)
                d2 = _d2(q, t)
                if not d2 < bound2:
                    continue
                # T2 on the other side of the query at the same distance in the plane's direction, and moved sideways so that its lower
                # edge is `side` away: d2' = d2 + side^2, half way between T's d2 and the bound
                side = np.sqrt(float(bound2 - d2) / 2.0)
                t2 = _plane_triangle(axis, F32(qx - (x0 - qx)), (flat, float(level) + S + side), S)
                if not (d2 < _d2(q, t2) < bound2):
                    continue
                first, second = (t, t2) if len(qs) % 2 == 0 else (t2, t)
                vs += [first, second]
                qs.append(q)
                found += 1
            if found >= per_axis:
                break
    v = np.concatenate(vs).astype(F32)
    return v, np.arange(v.shape[0], dtype=np.int32).reshape(-1, 3), np.stack(qs).astype(F32)


# ---- the search, restated: which cells a query looks at ----------------------------------------------------------------------------------
def register(vertices, triangles, cell, widen=True, max_cells=R.MAX_CELLS):
    """cell -> triangle indices, and the large list, as k_loc_classify / k_loc_insert decide them; `widen=False`: the bare vertex box."""
    v = np.ascontiguousarray(vertices, dtype=F32)
    cls, lo, hi = R.classify(v, triangles, cell)
    inv_c = F32(1) / F32(cell)
    grid, large = {}, []
    for t in np.nonzero(cls == R.USABLE)[0]:
        if widen:
            l, h = lo[t].astype(np.int64), hi[t].astype(np.int64)
        else:
            p = v[np.asarray(triangles)[t]]
            l = np.floor(p.min(axis=0) * inv_c).astype(np.int64)
            h = np.floor(p.max(axis=0) * inv_c).astype(np.int64)
        n = h - l + 1
        if n.max() > max_cells or n.prod() > max_cells:
            large.append(int(t))
            continue
        for x in range(l[0], h[0] + 1):
            for y in range(l[1], h[1] + 1):
                for z in range(l[2], h[2] + 1):
                    grid.setdefault((x, y, z), []).append(int(t))
    return grid, large


def search(vertices, triangles, queries, max_distance, cell, slack=True, widen=True):
    """k_loc_query restated in float32 scalars: shells in its order, LOC_NB cells per batch (the bound a batch is tested against is taken
    before the batch), its box test and ring bound, with `slack` or the registration's `widen` switched off.  -> (d2 (N,), triangle (N,))."""
    v = np.ascontiguousarray(vertices, dtype=F32)
    tri = np.asarray(triangles)
    c = F32(cell)
    inv_c = F32(1) / c
    grid, large = register(v, tri, cell, widen)
    r2 = F32(max_distance) * F32(max_distance)
    max_ring = int(np.floor(float(F32(max_distance)) / float(c))) + 1
    out_d2, out_t = np.full(len(queries), np.inf, dtype=F32), np.full(len(queries), -1, dtype=np.int32)

    def visit(q, ts, best):
        for t in sorted(ts):
            key = (_d2(q, v[tri[t]]), t)
            best = min(best, key)
        return best

    with np.errstate(all="ignore"):
        for i, q in enumerate(np.ascontiguousarray(queries, dtype=F32)):
            cq = [cell_coord(q[k], inv_c) for k in range(3)]
            best = visit(q, large, (F32(np.inf), 0x7FFFFFFF))
            sl = F32(2.0 ** -21) * (np.abs(q).max() + F32(max_ring + 2) * c) if slack else F32(0)
            for rho in range(max_ring + 2):
                rng = range(-rho, rho + 1)
                shell = [(dx, dy, dz) for dx in rng for dy in rng for dz in rng if max(abs(dx), abs(dy), abs(dz)) == rho]
                for b0 in range(0, len(shell), LOC_NB):
                    far2 = min(best[0], r2)
                    for d in shell[b0:b0 + LOC_NB]:
                        h = []
                        for k in range(3):
                            g = q[k] - F32(cq[k] + d[k] + 1) * c if d[k] < 0 else F32(cq[k] + d[k]) * c - q[k] if d[k] > 0 else F32(0)
                            h.append(max(g - sl, F32(0)))
                        if (h[0] * h[0] + h[1] * h[1]) + h[2] * h[2] <= far2:
                            best = visit(q, grid.get((cq[0] + d[0], cq[1] + d[1], cq[2] + d[2]), ()), best)
                lb = F32(rho) * c - sl
                if lb > 0 and (r2 < lb * lb or best[0] < lb * lb):
                    break
            if best[1] != 0x7FFFFFFF and best[0] <= r2:
                out_d2[i], out_t[i] = best
    return out_d2, out_t
