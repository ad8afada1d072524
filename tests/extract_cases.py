"""Planted maps and the extract chain restated in NumPy, for the tests of dif_extract / dif_extract_streams (tests/test_extract_cpu.py pins
the restatements on the CPU, tests/test_gpu_extract_envelope.py compares the kernels with them).  TEST INFRASTRUCTURE ONLY: neither the package nor
the oracle is imported here, and everything is a deterministic function of its seed.

THE RESTATEMENTS, one per stage of csrc/kernels_extract.hip.h and of the log half of csrc/kernels_mesh.hip.h:
  prepare      map.py:627-637.  The dirty list (lin ids in ascending SLOT order), the batch (the confident voxels among the dirty voxels' clamped
               7-neighbourhoods, each once, in ascending LIN order), vbm; the clamps by max_voxels with their DIF_C_OVERFLOW codes, the deferral
               of the block-totals scan, the halo rule of a tiled map.  Integers only.
  upsample2    map.py:655-665, tri_axis / tri_sample of kernels_extract.hip.h in their order, every fused multiply-add rounded ONCE (fma32).
  log_update   map.py:703-714 on an append-only log: the rows a call writes, alive, tri_start / tri_n, the counters, the caller's copy, the
               dif_pending_export_t record.  THE RULE AT A LIMIT: of a call's T triangles the first n_new = min(T, max_triangles, room in the log)
               are kept; a voxel's previous batch dies only if one of ITS triangles is among them.
"""
from __future__ import annotations

import numpy as np

from . import integrate_cases as IC
from . import optim_cases as OC

F32 = np.float32
GRID = 16
IGNORE_TH = F32(16.0)
TH_NEXT = np.nextafter(IGNORE_TH, F32(np.inf))            # the float32 successor of the threshold: the smallest confident count
FILL = 0xA5                                               # every extract buffer holds this byte before a call

CORNERS = [(x, y, z) for x in (0, 15) for y in (0, 15) for z in (0, 15)]
EDGES = [(0, 0, 7), (0, 7, 0), (7, 0, 0), (15, 15, 8), (15, 8, 15), (8, 15, 15)]
FACES = [(0, 6, 9), (9, 0, 6), (6, 9, 0), (15, 5, 10), (10, 15, 5), (8, 3, 15)]
ROW = [(3, 5, 14), (3, 5, 15), (3, 6, 0), (3, 6, 1)]      # lin 862..865: 862, 863 in bitmap word 26, 864, 865 in word 27; (3,5,15) + z is NOT (3,6,0)
PAIR = [(6, 6, 6), (6, 6, 7)]                             # two dirty voxels that share neighbours (and are each other's)
TRIPLE = [(8, 8, 5), (8, 8, 6), (8, 9, 5)]
AT_TH = (5, 7, 7)                                         # dirty, its own count exactly ignore_count_th: listed, not in the batch, no triangle
BLOB = [(x, y, z) for x in range(4, 11) for y in range(4, 11) for z in range(4, 10)]
LONELY = (13, 2, 2)                                       # dirty, every neighbour unallocated


def _lin(v, grid=GRID):
    return int(OC.lin_of(np.asarray(v), grid))


def wrap_ids(v, grid=GRID):
    """the ids a neighbour WITHOUT its clamp on the y or z axis would name from a voxel on that border (inside the grid's id range)"""
    x, y, z = v
    out = []
    if z == grid - 1: out.append(_lin(v, grid) + 1)
    if z == 0: out.append(_lin(v, grid) - 1)
    if y == grid - 1: out.append(_lin(v, grid) + grid)
    if y == 0: out.append(_lin(v, grid) - grid)
    return [w for w in out if 0 <= w < grid ** 3]


class Case:
    """pm: the planted map (IMap, dirty flags set for frame 0); dirty1 / latent1 / obs1: the second frame's dirty slots and what they change"""


def planted(capacity: int, seed: int = 5, n_extra: int = 0) -> Case:
    """The 16^3 map of the envelope: a few hundred voxels (n_extra more, scattered, for the case that needs B > 1024), ~50 dirty on purpose."""
    g = np.random.default_rng(seed)
    dirty_v = CORNERS + EDGES + FACES + ROW[:3] + PAIR + TRIPLE + [AT_TH, LONELY]
    true_nb = set(IC.neighbours7([_lin(v) for v in dirty_v], GRID).tolist())
    witnesses = sorted({w for v in dirty_v for w in wrap_ids(v)} - true_nb)
    keep = set(map(tuple, PAIR + TRIPLE + [AT_TH]))
    blob = [v for v in BLOB if v in keep or g.random() > 0.08]
    lin = set(_lin(v) for v in dirty_v + ROW + blob) | set(witnesses)
    lin -= set(IC.neighbours7([_lin(LONELY)], GRID).tolist()) - {_lin(LONELY)}
    if n_extra:
        free = np.setdiff1d(np.arange(GRID ** 3), np.fromiter(lin, dtype=np.int64))
        free = np.setdiff1d(free, IC.neighbours7([_lin(LONELY)], GRID))
        lin |= set(g.choice(free, size=n_extra, replace=False).tolist())
    lin = np.array(sorted(lin), dtype=np.int64)
    n = lin.size
    lat = g.standard_normal((n, 29)).astype(F32)
    fixed = g.standard_normal((3, 29)).astype(F32)
    clone = np.arange(n) % 3 == 0                                          # one third of the voxels hold one of three fixed latents
    lat[clone] = fixed[(np.arange(n)[clone] // 3) % 3]
    obs = np.full(n, 1000.0, dtype=F32)
    pm = IC.IMap(lin, capacity, latents=lat, obs=obs, grid=GRID)
    special = set(_lin(v) for v in dirty_v + ROW)
    for s in range(n):
        if int(lin[s]) not in special and int(lin[s]) not in witnesses:
            u = g.random()
            pm.obs[s] = IGNORE_TH if u < 0.12 else TH_NEXT if u < 0.24 else 1000.0
    pm.obs[pm.indexer[_lin(AT_TH)]] = IGNORE_TH
    c = Case()
    c.pm, c.witnesses, c.clone = pm, np.array(witnesses, dtype=np.int64), clone
    more = [v for v in blob if g.random() < 0.1]                          # and a tenth of the blob, wherever it falls
    c.dirty0 = np.unique(np.concatenate([pm.indexer[[_lin(v) for v in dirty_v + more]], [255, 256, 257, n - 1]]))
    pm.dirty[c.dirty0] = 1
    # the second frame: a subset dirty again with other latents; two of them lose their confidence (a voxel outside the batch yields no triangle:
    # its batch of frame 0 is stale and is KEPT, map.py:708-709), the rest are re-meshed and their batches replaced
    again = [pm.indexer[_lin(v)] for v in TRIPLE + PAIR + CORNERS[:3] + [FACES[5], EDGES[0], AT_TH]] + [255, 256, 257]
    c.dirty1 = np.unique(np.array(again, dtype=np.int64))
    c.latent1 = (g.standard_normal((c.dirty1.size, 29)) * 1.5).astype(F32)
    c.unconfident1 = np.array([pm.indexer[_lin(TRIPLE[0])], 256], dtype=np.int64)
    return c


def second_frame(c: Case, pm):
    """apply the second frame's changes to `pm` (a clone of c.pm after the first extract: its dirty flags are clear)"""
    pm.latent[c.dirty1] = c.latent1
    pm.obs[c.unconfident1] = IGNORE_TH
    pm.dirty[c.dirty1] = 1


def grid64(capacity: int = 1024) -> Case:
    """A 64^3 map (8,192 bitmap words: 32 grid_tot blocks of 256 words = 8,192 voxels) with dirty voxels either side of the edge between blocks
    0 and 1 — lin 8191 = (1,63,63) and lin 8192 = (2,0,0) — whose neighbourhoods reach into the other block."""
    G = 64
    a, b = (1, 63, 63), (2, 0, 0)
    vox = [a, b, (1, 0, 0), (3, 0, 0), (2, 1, 0), (2, 0, 1), (1, 62, 63), (1, 63, 62), (0, 63, 63), (2, 63, 63), (2, 0, 2), (40, 40, 40), (40, 40, 41)]
    lin = np.array(sorted(_lin(v, G) for v in vox), dtype=np.int64)
    g = np.random.default_rng(64)
    pm = IC.IMap(lin, capacity, latents=g.standard_normal((lin.size, 29)).astype(F32), grid=G)
    c = Case()
    c.pm = pm
    c.dirty0 = np.sort(pm.indexer[[_lin(v, G) for v in (a, b, (2, 0, 1), (40, 40, 40))]])
    pm.dirty[c.dirty0] = 1
    return c


# ---- the dirty list, the batch, vbm ---------------------------------------------------------------------------------------------------
class Prepared:
    pass


def prepare(pm, no_cache=False, max_voxels=None, own=None, block_totals=False) -> Prepared:
    """What the two scans of an extract leave (k_mark_halo_dirty, the dirty scan of the plan, OccFunctor), and pm.dirty cleared as they clear it.
    own = (x_lo, x_hi): a tiled map.  block_totals: the scan defers instead of overflowing."""
    G, n = pm.grid, pm.n
    mv = n if max_voxels is None else int(max_voxels)
    p = Prepared()
    flagged = np.nonzero(pm.dirty[:n])[0]
    owned = np.ones(pm.capacity, dtype=bool)
    if own is not None:
        owned[:n] = (pm.pos[:n] >= own[0] * G * G) & (pm.pos[:n] < own[1] * G * G)
    halo = flagged[~owned[flagged]]
    listed = (np.arange(n) if no_cache else flagged)
    listed = listed[owned[listed]]
    p.K_total, p.deferred, p.overflow = int(listed.size), 0, 0
    if block_totals and min(7 * p.K_total, n) > mv:                       # nothing at all changes (k_dirty_scan leaves before its first store)
        p.deferred = min(7 * p.K_total, n)
        p.K = p.B = p.B_total = 0
        p.valid_blocks, p.batch, p.occ_slot = np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int32)
        p.vbm = -np.ones(pm.capacity, dtype=np.int32)
        return p
    pm.dirty[:n] = 0
    if p.K_total > mv:
        p.overflow = 2
    p.K = min(p.K_total, mv)
    p.valid_blocks = pm.pos[listed[:p.K]]
    marks = np.concatenate([pm.pos[listed[:p.K]], pm.pos[halo]])
    nb = IC.neighbours7(marks, G) if marks.size else np.zeros(0, dtype=np.int64)
    slot = pm.indexer[nb]
    ok = slot >= 0
    ok[ok] = pm.obs[slot[ok]] > IGNORE_TH                                  # map.py:631
    batch = nb[ok]
    p.B_total = int(batch.size)
    if p.B_total > mv:
        p.overflow = 3                                                     # (written behind code 2 in stream order)
    p.B = min(p.B_total, mv)
    p.batch = batch[:p.B]
    p.occ_slot = pm.indexer[p.batch].astype(np.int32)
    p.vbm = -np.ones(pm.capacity, dtype=np.int32)
    p.vbm[p.occ_slot] = np.arange(p.B, dtype=np.int32)
    return p


# ---- the trilinear x2 -------------------------------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """float32 fma(a, b, c) rounded ONCE: the product is exact in float64, the sum is brought to round-to-odd in float64 (two-sum; 53 bits are
    more than 2 * 24 + 2) and only then rounded to float32 — a float64 sum that landed on a float32 midpoint by its own rounding is told apart."""
    a, b, c = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(c, dtype=np.float64)
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)                                        # s + err = p + c exactly
    inexact = err != 0.0
    toward_zero = inexact & ((err > 0) != (s > 0))                         # the exact sum lies between s and the next double toward zero
    t = np.where(toward_zero, np.nextafter(s, 0.0), s)
    ti = t.view(np.int64).copy()
    ti[inexact] |= 1                                                       # sticky bit: round to odd
    return ti.view(np.float64).astype(F32)


def _mul32(a, b):
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64)).astype(F32)


def tri_axis(l: int, R: int):
    """kernels_extract.hip.h: tri_axis for j = 0..R-1 -> i0, i1, w0, w1"""
    scale = F32(F32(l - 1) / F32(R - 1))
    src = _mul32(scale, np.arange(R, dtype=F32))
    i0 = np.minimum(src.astype(np.int64), l - 1)
    i1 = i0 + (i0 < l - 1)
    w1 = np.clip((src - i0.astype(F32)).astype(F32), F32(0), F32(1))
    return i0, i1, (F32(1) - w1).astype(F32), w1


def upsample2(low, R: int):
    """low (B, l, l, l) float32 -> (B, R, R, R): tri_sample, z innermost, then y, then x; each tap fma(t0, w0, fl(t1 * w1))"""
    out = np.asarray(low, dtype=F32)
    i0, i1, w0, w1 = tri_axis(out.shape[1], R)
    for axis in (3, 2, 1):
        shp = [1, 1, 1, 1]
        shp[axis] = R
        t0, t1 = np.take(out, i0, axis=axis), np.take(out, i1, axis=axis)
        out = fma32(t0, np.broadcast_to(w0.reshape(shp), t0.shape), _mul32(t1, w1.reshape(shp)))
    return out


# ---- the log ----------------------------------------------------------------------------------------------------------------------------
class Log:
    """The device-resident mesh cache as dif_extract keeps it."""

    def __init__(self, map_capacity: int, cache_capacity: int):
        self.cc = int(cache_capacity)
        self.tri, self.id, self.std = np.zeros((self.cc, 3, 3), F32), np.zeros(self.cc, np.int64), np.zeros((self.cc, 3), F32)
        self.alive = np.zeros(self.cc, dtype=np.uint8)
        self.written = np.zeros(self.cc, dtype=bool)                       # rows some call has written
        self.T = self.kept = self.dead = 0
        self.tri_start, self.tri_n = np.zeros(map_capacity, np.int32), np.zeros(map_capacity, np.int32)

    def live(self):
        k = np.nonzero(self.alive[:self.T])[0]
        return self.tri[k], self.id[k], self.std[k]

    def clone(self):
        q = Log(self.tri_n.size, self.cc)
        for name, v in self.__dict__.items():
            setattr(q, name, v.copy() if isinstance(v, np.ndarray) else v)
        return q


def voxel_runs(tid):
    """the canonical triangle list by voxel -> lin id, first triangle, count of each run"""
    tid = np.asarray(tid, dtype=np.int64)
    if tid.size == 0:
        return tid, np.zeros(0, np.int64), np.zeros(0, np.int64)
    first = np.nonzero(np.concatenate([[True], tid[1:] != tid[:-1]]))[0]
    return tid[first], first, np.diff(np.concatenate([first, [tid.size]]))


def log_update(log: Log, indexer, tri, tid, tstd, max_triangles: int, out_capacity: int = 0, no_cache: bool = False, seq: int = 0,
               cut_keeps: bool = True):
    """One extract's marching-cubes output (UNTRUNCATED, canonical order) appended to `log` in place -> a namespace: n_new, whole_cut (lin ids
    of the voxels that lost every new triangle to a limit), overflow (5 or 0), out (the caller's copy: tri, id, std), pending (the
    dif_pending_export_t words pending, kept, n, seq), T.  cut_keeps = False: what the kernels did before the rule was the reference's."""
    r = type("LogResult", (), {})()
    if no_cache:
        log.T = log.dead = 0
        log.tri_n[:] = 0
    kept = log.kept = log.T
    r.T = int(len(tid))
    n_new = min(r.T, int(max_triangles))
    r.overflow = 5 if kept + n_new > log.cc else 0
    n_new = min(n_new, log.cc - kept)
    r.n_new = n_new
    log.tri[kept:kept + n_new], log.id[kept:kept + n_new], log.std[kept:kept + n_new] = tri[:n_new], tid[:n_new], tstd[:n_new]
    log.alive[kept:kept + n_new] = 1
    log.written[kept:kept + n_new] = True
    whole = []
    for v, first, cnt in zip(*voxel_runs(tid)):
        slot = indexer[v]
        n = max(0, min(int(cnt), n_new - int(first)))
        if n == 0:
            whole.append(int(v))
            if cut_keeps:
                continue
        old_s, old_n = int(log.tri_start[slot]), int(log.tri_n[slot])
        log.alive[old_s:old_s + old_n] = 0
        log.dead += old_n
        log.tri_start[slot], log.tri_n[slot] = kept + int(first), n
    r.whole_cut = np.array(whole, dtype=np.int64)
    log.T = kept + n_new
    n_out = min(n_new, int(out_capacity))
    r.out = (log.tri[kept:kept + n_out].copy(), log.id[kept:kept + n_out].copy(), log.std[kept:kept + n_out].copy())
    r.pending = (1 if n_out > 0 else 0, kept, n_out, seq)
    return r


def limit_cases(T0, kept, T1, runs):
    """(max_triangles, cache_capacity) of every limit case of a frame with T triangles behind `kept` log entries; runs = voxel_runs of it"""
    _, first, cnt = runs
    mid = int(first[len(first) // 2])
    return [(T1, 10 ** 6), (T1 - 1, 10 ** 6), (mid, 10 ** 6), (mid + 1, 10 ** 6), (1, 10 ** 6),
            (10 ** 6, kept + T1), (10 ** 6, kept + T1 - 1), (10 ** 6, kept + mid + int(cnt[len(first) // 2]) // 2 + 1), (10 ** 6, kept + 1)]
