"""The spatially tiled map restated in NumPy: integrate under ownership with its boundary change lists, the record and halo-message
exports, the merges, the delta export and the list reset — with the cases and the bar for tests/test_tiling_cpu.py (CPU: pinned against the
oracle) and tests/test_gpu_tiling_envelope.py (GPU: dif_integrate, dif_export_*, dif_merge_*, dif_export_halo_delta, dif_halo_lists_reset on
planted 16^3 maps).  TEST INFRASTRUCTURE ONLY; everything here is a deterministic function of its seed.

OWNERSHIP (read from csrc/kernels_integrate.hip.h; own = [lo, hi) in x, halo = h):
  voxel_count_point   a point whose own voxel has x outside [lo - h, hi + h) gets pt_lin = -1: not counted, not kept, no candidate
  k_prune_mark        the allocation candidates (own voxel and six clamped neighbours) are NOT restricted
  k_focus_gather      the focus test is not restricted; a pair goes only to a neighbour voxel with x in [lo, hi)
CHANGE LISTS (common.hip.h: halo_lists_of, HaloLists::note): left = owned x in [lo, min(lo + h, hi)) if lo > 0, right = owned x in
[max(hi - h, lo), hi) if hi < grid.  AllocFunctor::emit notes every slot it hands out, k_fuse every fused slot that existed before the call.
A list's order comes from atomics: lists are compared as sets, and of a list longer than its cap only size and membership are known.

THE BAR of an additive merge against the float64 weighted mean  m = (z w + z_r w_r) / (w + w_r),  u = 2^-24:
  the GPU computes  p_r = fl(z_r w_r) (the exporter),  p = fl(z w),  s = fl(p + p_r),  q = fl(s / w')  with  w' = fl(w + w_r).
  Integer weights whose sum is below 2^24: w' is exact.  With A = |z| w + |z_r| w_r:
      |p + p_r - (z w + z_r w_r)| <= u A                          (two roundings, each relative to its own product)
      |s - (z w + z_r w_r)|       <= u A + u (1 + u) A            (the sum's rounding is relative to |p + p_r| <= (1 + u) A)
      |q - m|                     <= [(2u + u^2) + u (1 + 2u + u^2)] A / w' = (3u + 3u^2 + u^3) A / w'
  so  |q - m| <= C_INT * u * A / w'  with  C_INT = 3 + 2^-22  (3u^2 + u^3 < 2^-22 u),  plus UNDERFLOW = 2^-148 for results in the subnormal
  range (three operations can round there, 2^-150 each; w' >= 1 in every set, so nothing amplifies them).
  Non-integer weights: w' = (w + w_r)(1 + d), |d| <= u, divides s: one more factor (1 - u)^-1 on the quotient,
      |q - m| <= [(1 + 2u + u^2)(1 + u) / (1 - u) - 1] A / (w + w_r) < (4 + 2^-20) u A / (w + w_r):  C_FRAC = 4 + 2^-20.
  The float64 reference's own error (a few 2^-53) is below a millionth of either.
"""
from __future__ import annotations

import numpy as np

from . import integrate_cases as IC
from . import optim_cases as OC

F32 = np.float32
GRID = OC.GRID
PLANE = GRID * GRID
U = 2.0 ** -24
C_INT, C_FRAC, UNDERFLOW = 3.0 + 2.0 ** -22, 4.0 + 2.0 ** -20, 2.0 ** -148
KIND_DELTA, KIND_RESET = 1, 0


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def i32(a):
    """float32 values as the int32 words a record carries"""
    return np.ascontiguousarray(a, dtype=F32).view(np.int32)


def same_bits(a, b):
    a, b = np.asarray(a, dtype=F32), np.asarray(b, dtype=F32)
    return bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


# ---- integrate under ownership -------------------------------------------------------------------------------------------------------
def is_tiled(own, grid=GRID):
    lo, hi = own
    return hi > lo and (lo > 0 or hi < grid)


def list_ranges(own, halo, grid=GRID):
    """halo_lists_of -> ((l_lo, l_hi), (r_lo, r_hi)) in voxel x; an empty range where there is no neighbour (or no lists at all)"""
    lo, hi = own
    if not is_tiled(own, grid) or halo <= 0:
        return (0, 0), (0, 0)
    left = (lo, min(lo + halo, hi)) if lo > 0 else (0, 0)
    right = (max(hi - halo, lo), hi) if hi < grid else (0, 0)
    return left, right


class TMap(IC.IMap):
    """An IMap with its two boundary change lists (every entry ever noted since the last export, in no order) — the device keeps the first
    `cap` of each and the count of all of them."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.lists = ([], [])

    @classmethod
    def of(cls, pm, capacity=None):
        q = cls(pm.pos[:pm.n], pm.capacity if capacity is None else capacity, grid=pm.grid, voxel=pm.voxel_size)
        n = pm.n
        q.indexer, q.pos[:n] = pm.indexer.copy(), pm.pos[:n]                                     # (slot order: not ascending after an integrate)
        q.obs[:n], q.latent[:n], q.dirty[:n] = pm.obs[:n], pm.latent[:n], pm.dirty[:n]
        q.lists = tuple(list(x) for x in getattr(pm, "lists", ([], [])))
        return q

    def clone(self):
        return TMap.of(self)


def restate_tiled(pm, xyz, normal, prune_min, own=None, halo=0, list_cap=0, th=IC.TH):
    """integrate_cases.restate under the three ownership rules; pm is advanced in place, its lists included (a TMap; an IMap's are not kept).
    -> Restated with, besides restate's fields: noted = (left, right) the slots THIS call noted, lists = (left, right) what the lists hold
    after it as sets, pending = the two counts, kept = how many of each the device keeps under list_cap."""
    G = pm.grid
    lo, hi = (0, G) if own is None or own[1] <= own[0] else own
    plane = G * G
    xyz, normal = np.asarray(xyz, dtype=F32), np.asarray(normal, dtype=F32)
    r = IC.Restated()
    r.N = N = xyz.shape[0]
    lin = IC.voxel_ids(pm, xyz)
    x = lin // plane
    r.pt_lin = lin = np.where((lin >= 0) & (x >= lo - halo) & (x < hi + halo), lin, -1).astype(np.int32)
    valid = lin >= 0
    counts = np.bincount(lin[valid], minlength=G ** 3)
    r.mask = (valid & ((counts[np.where(valid, lin, 0)] > prune_min) if prune_min > 0 else valid)).astype(np.uint8)
    kept = lin[r.mask.astype(bool)].astype(np.int64)
    src = np.unique(kept[pm.indexer[kept] == -1])
    cand = IC.neighbours7(src, G) if src.size else np.zeros(0, dtype=np.int64)
    r.candidates = cand = cand[pm.indexer[cand] == -1]                                           # not restricted to the slab
    r.n_before, r.alloc_new = pm.n, int(cand.size)
    take = cand[:max(0, pm.capacity - pm.n)]
    pm.indexer[take] = pm.n + np.arange(take.size)
    pm.pos[pm.n:pm.n + take.size] = take
    pm.n += int(take.size)
    r.alloc_kept = int(take.size)
    r.overflow = int(r.n_before + r.alloc_new > pm.capacity)
    r.w_old, r.dirty_old = pm.obs.copy(), pm.dirty.copy()
    r.in_set = (pm.obs < F32(th)) & (pm.pos >= 0)
    o, i, slot, rel = OC.gather_pairs(pm, xyz, r.mask, r.in_set)
    tx = pm.pos[slot] // plane                                                                   # the pair's target voxel
    own_pair = (tx >= lo) & (tx < hi)
    r.o, r.i, r.slot, r.rel = o[own_pair], i[own_pair], slot[own_pair], rel[own_pair]
    r.dropped_pairs = int((~own_pair).sum())
    r.key = r.o * N + r.i
    r.rows = np.concatenate([r.rel, normal[r.i]], axis=1).astype(F32).reshape(-1, 6)
    r.M = int(r.slot.size)
    r.uniq, r.inv, r.cnt = np.unique(r.slot, return_inverse=True, return_counts=True)
    r.C, r.items = int(r.uniq.size), (r.M + 31) >> 5
    pm.obs[r.uniq] = (pm.obs[r.uniq] + r.cnt.astype(F32)).astype(F32)
    pm.dirty[r.uniq] = 1
    r.n_after = pm.n
    # the change lists: new slots (AllocFunctor::emit), then fused slots that existed before the call (k_fuse)
    ranges = list_ranges((lo, hi), halo if list_cap > 0 else 0, G)
    new_slots = np.arange(r.n_before, pm.n)
    old_fused = r.uniq[r.uniq < r.n_before]
    lists = getattr(pm, "lists", ([], []))
    r.noted, r.noted_new, r.noted_old = [], [], []
    for side, (a, b) in enumerate(ranges):
        sx = lambda s: pm.pos[s] // plane
        nn = [int(s) for s in new_slots if a <= sx(s) < b]
        no = [int(s) for s in old_fused if a <= sx(s) < b]
        r.noted_new.append(set(nn))
        r.noted_old.append(set(no))
        r.noted.append(set(nn) | set(no))
        lists[side].extend(nn + no)
    r.lists = tuple(set(x) for x in lists)
    r.pending = tuple(len(x) for x in lists)
    r.kept = tuple(min(len(x), list_cap) for x in lists)
    return r


# ---- records ---------------------------------------------------------------------------------------------------------------------------
def records_of(pm, slots, raw):
    """(len(slots), 32) int32: lin | dirty | w | payload[29], payload = float32(z * w) (one multiplication) or z when raw"""
    slots = np.asarray(slots, dtype=np.int64)
    rec = np.zeros((slots.size, 32), dtype=np.int32)
    w = pm.obs[slots].astype(F32)
    rec[:, 0] = pm.pos[slots].astype(np.int32)
    rec[:, 1] = (pm.dirty[slots] != 0).astype(np.int32)
    rec[:, 2] = i32(w)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        pay = pm.latent[slots] if raw else (pm.latent[slots] * w[:, None]).astype(F32)
    rec[:, 3:32] = i32(pay).reshape(-1, 29)
    return rec


def export_records(pm, x_lo, x_hi, raw, max_records):
    """dif_export_records -> (records (count,32), count = C_EXPORT_N, flag: 6 when the range holds more than max_records, else 0)"""
    x_lo, x_hi = max(int(x_lo), 0), min(int(x_hi), pm.grid)
    plane = pm.grid * pm.grid
    lin = pm.pos[:pm.n]
    sel = np.nonzero((lin >= x_lo * plane) & (lin < max(x_hi, x_lo) * plane))[0]                 # slot order
    count = min(sel.size, int(max_records))
    return records_of(pm, sel[:count], raw), count, (6 if sel.size > max_records else 0)


def export_halo_message(pm, x_lo, x_hi, max_records):
    """dif_export_halo -> (header word 0, raw records (count,32), flag); the records start at row 1 of the message"""
    rec, count, flag = export_records(pm, x_lo, x_hi, True, max_records)
    return count, rec, flag


def message(rec, rows, header=None, fill=0):
    """a (1 + rows, 32) halo message around `rec` with header word 0 = `header` (default: the number of records)"""
    msg = np.full((1 + rows, 32), fill, dtype=np.int32)
    msg[0, :4] = 0
    msg[0, 0] = rec.shape[0] if header is None else header
    msg[1:1 + rec.shape[0]] = rec
    return msg


class Source:
    """One record source of a merge: rec (rows,32) int32 and, for a halo message, the device-side count of its header (else None)"""

    def __init__(self, rec, header=None):
        self.rec, self.header = np.ascontiguousarray(rec, dtype=np.int32).reshape(-1, 32), header

    def live(self):
        rows = self.rec.shape[0]
        return self.rec if self.header is None else self.rec[:min(max(int(self.header), 0), rows)]      # MergeSrc::count


def merge(pm, sources, assign):
    """dif_merge_records / dif_merge_halo / dif_merge_halo2 on pm (in place) -> (flag: 1 when the allocation was cut, named: the slots a
    record reached).  In-range ids are distinct across the sources of a call."""
    G3 = pm.grid ** 3
    rec = np.concatenate([s.live() for s in sources]) if sources else np.zeros((0, 32), dtype=np.int32)
    lin = rec[:, 0].astype(np.int64)
    ok = (lin >= 0) & (lin < G3)
    rec, lin = rec[ok], lin[ok]
    assert np.unique(lin).size == lin.size, "records of one call carry distinct ids"
    new = np.unique(lin[pm.indexer[lin] == -1])
    flag = 1 if pm.n + new.size > pm.capacity else 0
    take = new[:max(0, pm.capacity - pm.n)]
    pm.indexer[take] = pm.n + np.arange(take.size)
    pm.pos[pm.n:pm.n + take.size] = take
    pm.n += int(take.size)
    s = pm.indexer[lin]
    got = s >= 0
    rec, s = rec[got], s[got]
    w_r = rec[:, 2].copy().view(F32)
    pay = rec[:, 3:32].copy().view(F32).reshape(-1, 29)
    if assign:
        pm.obs[s], pm.latent[s], pm.dirty[s] = w_r, pay, (rec[:, 1] & 1).astype(np.uint8)
        return flag, s
    with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
        w_old = pm.obs[s].astype(F32)
        w_new = (w_old + w_r).astype(F32)
        z = (((pm.latent[s] * w_old[:, None]).astype(F32) + pay).astype(F32) / w_new[:, None]).astype(F32)
        on = w_r > 0                                                                             # a weight-0 record only allocates
    pm.latent[s[on]] = z[on]
    pm.obs[s] = w_new
    pm.dirty[s[on]] = 1
    return flag, s


def merge_note(sources):
    """k_merge_apply's eight note words: the first four header words of either message (zeros for a source without one)"""
    out = np.zeros(8, dtype=np.int32)
    for k, hdr in enumerate(sources):
        if hdr is not None:
            out[4 * k:4 * k + 4] = hdr[:4]
    return out


def mean64(z, w, z_r, w_r):
    """the float64 weighted mean an additive merge approximates, and A / w' of the bar"""
    z, z_r = np.asarray(z, dtype=np.float64), np.asarray(z_r, dtype=np.float64)
    w, w_r = np.asarray(w, dtype=np.float64)[:, None], np.asarray(w_r, dtype=np.float64)[:, None]
    return (z * w + z_r * w_r) / (w + w_r), (np.abs(z) * w + np.abs(z_r) * w_r) / (w + w_r)


def merge_bar(z, w, z_r, w_r):
    """-> (m64 (n,29), bar (n,29)): integer weights with an exact sum take C_INT, every other row C_FRAC"""
    m, a = mean64(z, w, z_r, w_r)
    w64, wr64 = np.asarray(w, dtype=np.float64), np.asarray(w_r, dtype=np.float64)
    integer = (w64 == np.rint(w64)) & (wr64 == np.rint(wr64)) & (w64 + wr64 < 2.0 ** 24)
    return m, np.where(integer, C_INT, C_FRAC)[:, None] * U * a + UNDERFLOW


# ---- the delta export and the reset ----------------------------------------------------------------------------------------------------
def export_halo_delta(pm, list_cap, max_records, sides=(True, True)):
    """dif_export_halo_delta on pm's lists (emptied where a message goes) -> per side None, or a dict: n (records written), pending, header
    (n, pending, 1), pool (the records of every listed slot, by slot: the message's rows are n of them), exact (n == len(pool): then the
    rows ARE the pool, as a set) — and the flag (8 when a side's pending exceeds its n), and the eight note words (a side's are left alone
    without a message: given as -1 here)."""
    out, flag, note = [], 0, -np.ones(8, dtype=np.int64)
    for side in (0, 1):
        if not sides[side]:
            out.append(None)
            continue
        lst = pm.lists[side]
        pending = len(lst)
        n = min(pending, list_cap, int(max_records))
        uniq = sorted(set(lst))
        d = dict(n=n, pending=pending, header=(n, pending, KIND_DELTA), slots=uniq, pool=records_of(pm, uniq, True), exact=(n == pending))
        note[4 * side:4 * side + 3] = d["header"]
        if pending > n:
            flag = 8
        lst.clear()
        out.append(d)
    return out, flag, note


def halo_lists_reset(pm, headers=(None, None)):
    """dif_halo_lists_reset: headers[side] = the three header words the buffer holds before the call, or None -> (headers after, note)"""
    out, note = [], -np.ones(8, dtype=np.int64)
    for side in (0, 1):
        if headers[side] is None:
            out.append(None)
            continue
        pending = len(pm.lists[side])
        out.append((int(headers[side][0]), pending, KIND_RESET))
        note[4 * side:4 * side + 3] = out[-1]
        pm.lists[side].clear()
    return out, note


# ---- integrate cases -----------------------------------------------------------------------------------------------------------------
class TCase(IC.Case):
    """An integrate_cases.Case under ownership: own, halo, list_cap"""

    def __init__(self, label, pm, frames, prune_min, own, halo, list_cap, img=None):
        super().__init__(label, pm, frames, prune_min, img=img)
        self.own, self.halo, self.list_cap = own, int(halo), int(list_cap)


LIST_CAP = 512
SHORT = 16                      # alloc_overflow: slots the capacity is short of what the frame allocates


def _cloud(g, own, halo, n_per_x=6):
    """Points in every x layer of the grid (so: outside slab + halo, in the halo, in either boundary layer set and between them), 2 to 6 per
    voxel (prune_min = 2 drops the twos), and points ON the faces x = lo - h, lo, hi, hi + h, one ulp above and one below."""
    lo, hi = own
    vox = []
    for x in range(GRID):
        yz = 4 + g.choice(64, size=n_per_x, replace=False)
        for k in yz:
            vox += [(x, 4 + (k - 4) // 8, 4 + (k - 4) % 8)] * int(g.integers(2, 7))
    vox = np.array(vox)
    xyz = OC.points_in(vox, 0.02 + 0.96 * g.random((vox.shape[0], 3)))
    faces = []
    b = np.float64(OC.BOUND_MIN[0])
    for k in sorted({lo - halo, lo, hi, hi + halo}):
        if not 0 <= k <= GRID:
            continue
        f = F32(b + k * OC.VOXEL)
        for px in (f, np.nextafter(f, F32(np.inf)), np.nextafter(f, F32(-np.inf))):
            for rep in range(4):                                       # four each: they pass prune_min = 2 where they share a voxel
                q = OC.points_in([[0, 9, 9]], 0.1 + 0.2 * rep)[0]
                q[0] = px
                faces.append(q)
    xyz = np.concatenate([xyz, np.array(faces, dtype=F32)])
    xyz = xyz[g.permutation(xyz.shape[0])]
    return xyz, OC.unit_normals(g, xyz.shape[0])


def _planted(g, capacity=1024):
    """20 voxels in four x ranges, five each: x < 5, [5, 8), [8, 11), x >= 11; counts on both sides of encoder_count_th.  Slots go in
    ascending id order, so the slots of [8, 11) are 10..14 and those of x >= 11 are 15..19."""
    ijk = []
    for xs in ((1, 2, 3, 4, 4), (5, 5, 6, 7, 7), (8, 9, 9, 10, 10), (11, 12, 13, 14, 15)):
        for x in xs:
            while True:
                v = (x, int(g.integers(4, 12)), int(g.integers(4, 12)))
                if v not in ijk:
                    ijk.append(v)
                    break
    obs = g.choice([0.0, 3.0, IC.TH - 1.0, IC.TH, 900.0], size=len(ijk), p=[0.15, 0.45, 0.2, 0.1, 0.1])
    pm = IC._planted(g, ijk, capacity, obs)
    return TMap.of(pm), np.array(ijk)


def integrate_case(name: str, seed: int = 0) -> TCase:
    g = np.random.default_rng([211, seed, sum(map(ord, name))])
    own, halo, cap, n_frames = {"cut_mid": ((5, 11), 3, LIST_CAP, 1), "thin": ((7, 9), 3, LIST_CAP, 1), "edge_left": ((0, 6), 3, LIST_CAP, 1),
                                "edge_right": ((10, 16), 3, LIST_CAP, 1), "cap": ((5, 11), 3, 4, 1), "second_call": ((5, 11), 3, LIST_CAP, 2),
                                "alloc_overflow": ((5, 11), 3, LIST_CAP, 1)}[name]
    pm, ijk = _planted(g)
    frames = []
    for f in range(n_frames):
        xyz, nrm = _cloud(g, own, halo)
        # every planted voxel is fed (those below the threshold fuse: k_fuse's note site)
        extra = OC.points_in(np.repeat(ijk, 4, axis=0), 0.02 + 0.96 * g.random((4 * ijk.shape[0], 3)))
        frames.append((np.concatenate([xyz, extra]), np.concatenate([nrm, OC.unit_normals(g, extra.shape[0])])))
    if name == "alloc_overflow":
        need = restate_tiled(pm.clone(), *frames[0], 2, own=own, halo=halo, list_cap=cap)
        pm = TMap.of(pm, capacity=need.n_before + need.alloc_new - SHORT)
    return TCase(name, pm, frames, 2, own, halo, cap)


INTEGRATE_CASES = ("cut_mid", "thin", "edge_left", "edge_right", "cap", "second_call", "alloc_overflow")


def frame_case(H: int, W: int, seed: int = 0) -> TCase:
    """integrate_cases.frame_case turned so that image ROWS run along world x: whole 256-point pieces of the frame then lie outside the
    slab + halo (the chunk_any culling).  The slab is the two lowest layers the frame reaches, halo 1: the pieces at the other end of the
    image, and the camera centre (where the zero depths land), are outside."""
    c = IC.frame_case(H, W, seed)
    a, b = np.pi / 2 + 0.15, -0.1
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    pose = np.concatenate([(Rz @ Rx).reshape(-1), [0.05, 0.12, -1.0]]).astype(F32)
    xyz, nrm = IC.unproject32(c.depth, c.normal_cam, pose, c.intr)
    pm = TMap.of(c.pm)
    lin = IC.voxel_ids(pm, xyz)
    xs = lin[lin >= 0] // PLANE
    lo = int(xs.min())
    t = TCase(f"tiled frame {H}x{W}", pm, [(xyz, nrm)], c.prune_min, (lo, lo + 2), 1, LIST_CAP, img=(H, W))
    t.depth, t.normal_cam, t.pose, t.intr = c.depth, c.normal_cam, pose, c.intr
    return t


def culled_pieces(case: TCase):
    """256-point pieces of a frame case none of whose points lies inside the slab + halo -> (culled, pieces)"""
    xyz = case.frames[0][0]
    lin = IC.voxel_ids(case.pm, xyz)
    x = lin // PLANE
    inside = (lin >= 0) & (x >= case.own[0] - case.halo) & (x < case.own[1] + case.halo)
    n = (inside.size + 255) // 256
    any_in = np.array([inside[k * 256:(k + 1) * 256].any() for k in range(n)])
    return int((~any_in).sum()), n


# ---- record sets for export and merge --------------------------------------------------------------------------------------------------
def export_map(seed: int = 0, n: int = 150, capacity: int = 1024):
    """A map with slots on both sides of every x cut, dirty flags, weights of 0, integer and fractional weights, and a voxel that holds a NaN
    payload, -0.0 and a subnormal."""
    g = np.random.default_rng([223, seed, n])
    lin = np.sort(g.choice(GRID ** 3, size=n, replace=False))
    pm = TMap(lin, capacity, latents=(g.standard_normal((n, 29)) * 0.3).astype(F32),
              obs=g.choice([0.0, 1.0, 7.0, 599.0, 600.0, 1234.0, 2.5, 0.375], size=n).astype(F32))
    pm.dirty[:n] = g.integers(0, 2, size=n)
    pm.latent[n // 2, :3] = (IC.NaN_PAYLOAD, F32(-0.0), F32(1e-40))
    return pm


EXPORT_RANGES = ((5, 11), (-4, 7), (9, GRID + 5), (-2, GRID + 2), (8, 8), (9, 3), (0, 1), (GRID - 1, GRID))


class RecordSet:
    """Records for one merge call: sources [(rec, header or None)], and for the bar z_r, w_r of every record (in concatenated order)"""

    def __init__(self, label, pm, sources, z_r, w_r):
        self.label, self.pm, self.sources, self.z_r, self.w_r = label, pm, sources, z_r, w_r


def merge_target(g, n=120, capacity=1024, frac=False):
    lin = np.sort(g.choice(GRID ** 3, size=n, replace=False))
    w = g.choice([0.0, 1.0, 3.0, 17.0, 599.0, 4096.0], size=n) if not frac else 1.0 + 50.0 * g.random(n)
    pm = TMap(lin, capacity, latents=(g.standard_normal((n, 29)) * 0.3).astype(F32), obs=w.astype(F32))
    pm.dirty[:n] = g.integers(0, 2, size=n)
    pm.latent[3, :3] = (IC.NaN_PAYLOAD, F32(-0.0), F32(1e-40))            # slot 3: named only by a w_r = 0 record, or by none
    return pm


def _records(g, lin, w_r, flags=None):
    """records as an exporter writes them from latents z_r and weights w_r -> (rec, z_r)"""
    n = len(lin)
    z_r = (g.standard_normal((n, 29)) * 0.3).astype(F32)
    w_r = np.asarray(w_r, dtype=F32)
    rec = np.zeros((n, 32), dtype=np.int32)
    rec[:, 0] = np.asarray(lin, dtype=np.int64).astype(np.int32)
    rec[:, 1] = g.integers(0, 2, size=n) if flags is None else flags
    rec[:, 2] = i32(w_r)
    rec[:, 3:32] = i32((z_r * w_r[:, None]).astype(F32)).reshape(-1, 29)
    return rec, z_r


def record_set(name, seed: int = 0) -> RecordSet:
    """mixed: records naming existing voxels, new voxels and both, w_r = 0 among them (one on the NaN / -0.0 / subnormal voxel), lin = -1,
    grid and grid - 1.   frac: non-integer weights on both sides.   overrun: more new voxels than the capacity has room for.
    n<k>: k records (existing, new and out-of-range ids).   two: two messages of 1 and 70 rows.   hdr<h>: one message of 40 rows whose header
    says h (-3, 0, rows, rows + 5)."""
    g = np.random.default_rng([227, seed, sum(map(ord, name))])
    G3 = GRID ** 3
    frac = name == "frac"
    pm = merge_target(g, frac=frac, capacity=130 if name == "overrun" else (8192 if name == "n4097" else 1024))
    have = pm.pos[:pm.n]
    free = np.setdiff1d(np.arange(G3 - 1), have)                        # (grid - 1 is placed by hand)
    special = int(pm.pos[3])

    def pick(n_old, n_new, weights):
        old = g.choice(have[have != special], size=n_old, replace=False)
        new = g.choice(free, size=n_new, replace=False)
        lin = g.permutation(np.concatenate([old, new]))
        return lin, g.choice(weights, size=lin.size)

    iw = [0.0, 1.0, 2.0, 9.0, 300.0, 5000.0]
    if name in ("mixed", "frac", "overrun"):
        lin, w = pick(40, 60, 1.0 + 30.0 * g.random(6) if frac else iw)
        lin = np.concatenate([lin, [special, -1, G3, G3 - 1, -2 ** 31, 2 ** 31 - 1]])
        w = np.concatenate([w, [0.0, 5.0, 5.0, 4.0, 1.0, 1.0]])
        rec, z_r = _records(g, lin, w)
        return RecordSet(name, pm, [(rec, None)], z_r, w.astype(F32))
    if name.startswith("n"):
        k = int(name[1:])
        n_old, n_new = min(k // 3, 100), min(k - k // 3, 3900)
        lin, w = pick(n_old, n_new, iw)
        bad = np.where(np.arange(k - lin.size) % 2 == 0, -1 - np.arange(k - lin.size), G3 + np.arange(k - lin.size))
        lin, w = np.concatenate([lin, bad]), np.concatenate([w, np.ones(bad.size)])
        order = g.permutation(k)
        rec, z_r = _records(g, lin[order], w[order])
        return RecordSet(name, pm, [(rec, None)], z_r, w[order].astype(F32))
    if name == "two":
        lin, w = pick(30, 41, iw)
        rec, z_r = _records(g, lin, w)
        return RecordSet(name, pm, [(rec[:1], 1), (rec[1:], 70)], z_r, w.astype(F32))
    if name.startswith("hdr"):
        lin, w = pick(15, 25, iw)
        rec, z_r = _records(g, lin, w)
        return RecordSet(name, pm, [(rec, int(name[3:]))], z_r, w.astype(F32))
    raise KeyError(name)


ROWS_HDR = 40
RECORD_SETS = ("mixed", "frac", "overrun", "n1", "n2", "n63", "n64", "n65", "n4097", "two", "hdr-3", "hdr0", f"hdr{ROWS_HDR}", f"hdr{ROWS_HDR + 5}")


def bar_ratio(pm_before, pm_after, rs: RecordSet):
    """The additive merge of rs on pm_before left pm_after -> the worst |z - m64| / bar over the records that were applied with w_r > 0 (0 if
    none), and how many values that covers"""
    worst, count = 0.0, 0
    at = 0
    for rec, hdr in rs.sources:
        live = Source(rec, hdr).live().shape[0]
        lin = rec[:live, 0].astype(np.int64)
        z_r, w_r = rs.z_r[at:at + live], rs.w_r[at:at + live]
        at += rec.shape[0]
        ok = (lin >= 0) & (lin < pm_after.grid ** 3)
        s_after = np.where(ok, pm_after.indexer[np.where(ok, lin, 0)], -1)
        use = (s_after >= 0) & (w_r > 0)
        if not use.any():
            continue
        s = s_after[use]
        s_before = pm_before.indexer[lin[use]]
        z0 = np.where((s_before >= 0)[:, None], pm_before.latent[np.maximum(s_before, 0)], 0).astype(F32)
        w0 = np.where(s_before >= 0, pm_before.obs[np.maximum(s_before, 0)], 0).astype(F32)
        finite = np.isfinite(z0).all(axis=1)
        m, bar = merge_bar(z0[finite], w0[finite], z_r[use][finite], w_r[use][finite])
        err = np.abs(pm_after.latent[s][finite].astype(np.float64) - m)
        worst = max(worst, float((err / bar).max()))
        count += err.size
    return worst, count


# ---- the closed loop -------------------------------------------------------------------------------------------------------------------
CUT = 8


def loop_clouds(seed: int = 0, n_frames: int = 3, n_points: int = 2000):
    """Three clouds of about 2,000 points on a tilted sheet that crosses the cut at x = 8, dense enough to pass prune_min = 2"""
    g = np.random.default_rng([229, seed])
    frames = []
    for f in range(n_frames):
        x = 3.0 + 10.0 * g.random(n_points)
        y = 4.0 + 8.0 * g.random(n_points)
        z = 6.0 + 0.25 * (x - 8.0) + 0.1 * y + 0.3 * f + 0.05 * g.standard_normal(n_points)
        xyz = (np.stack([x, y, z], axis=1) * OC.VOXEL + np.asarray(OC.BOUND_MIN, dtype=np.float64)).astype(F32)
        frames.append((xyz, OC.unit_normals(g, n_points)))
    return frames
