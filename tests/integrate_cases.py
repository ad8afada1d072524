"""Planted maps, the integrate chain restated in NumPy, the cases and the bar for the tests of dif_integrate / dif_integrate_frame
(tests/test_ref64_cpu.py on the CPU, tests/test_gpu_integrate_envelope.py on the GPU).  TEST INFRASTRUCTURE ONLY; everything here is a
deterministic function of its seed.

THE RESTATEMENT (restate) walks map.py:366-452 with the oracle's float32 operations, one stage per kernel of csrc/kernels_integrate.hip.h:
voxel ids (ceil((p - b) / vs) - 1; NaN and out-of-grid points are invalid), per-frame counts and the prune mask, the allocation candidates
(own voxel plus six clamped neighbours, the empty ones), allocation in ascending id order under the capacity clamp, the encode set
{obs < encoder_count_th}, the focus test and the eight-offset pairs with their `rel` rows (optim_cases.gather_pairs, which the optimiser's
gather shares).  It is pinned against OracleMap.integrate_keyframe on the CPU.

THE BAR of a fused latent with w_old = 0 (channel c in group g of mlp_cases.ENC_GROUPS):
    |latent_gpu - mean64| <= K_BAR * e_ref(g) + 2^-31 + 2 ulp32(mean64)
  mean64   the float64 mean of Ref64.encoder over the voxel's restated rows;
  e_ref(g) the worst error, over the case's rows, of the float32 oracle's encoder against Ref64.encoder in that group (the error of a mean
           cannot exceed the worst row's); K_BAR is mlp_cases' constant, pinned on the CPU;
  2^-31    half a unit of the 2^-30 fixed point every row is rounded to;  2 ulp: the conversion of the integer sum and the division.
"""
from __future__ import annotations

import struct

import numpy as np

from . import mlp_cases as C
from . import optim_cases as OC

F32 = np.float32
FIX = 2.0 ** 30                           # DIF_FIX_SCALE
DIR_IDS = 14                              # DIF_DIR_IDS: record ids a slot's directory holds before it chains
TH = 600.0                                # encoder_count_th of every case
NaN_PAYLOAD = np.array([0x7FC12345], dtype=np.uint32).view(F32)[0]


class IMap(OC.Planted):
    """A Planted map with what integrate adds to it: the dirty flags, and allocation while it runs."""

    def __init__(self, lin, capacity, latents=None, obs=None, grid=OC.GRID, voxel=OC.VOXEL):
        super().__init__(lin, capacity, latents=latents, obs=obs, grid=grid, voxel=voxel)
        self.dirty = np.zeros(capacity, dtype=np.uint8)

    def clone(self):
        q = IMap(self.pos[:self.n], self.capacity, grid=self.grid, voxel=self.voxel_size)
        q.indexer, q.pos, q.obs, q.latent, q.dirty, q.n = self.indexer.copy(), self.pos.copy(), self.obs.copy(), self.latent.copy(), self.dirty.copy(), self.n
        return q


# ---- the chain, stage by stage ---------------------------------------------------------------------------------------------------
def voxel_ids(pm, xyz):
    """k_voxel_count's pt_lin -> (N,) int32, -1 for NaN / out-of-grid (map.py:366-369)"""
    xyz = np.asarray(xyz, dtype=F32)
    with np.errstate(invalid="ignore", over="ignore"):
        xn = ((xyz - pm.bound_min[None, :]) / F32(pm.voxel_size)).astype(F32)
        c = np.ceil(xn)
        ok = (c >= 1).all(axis=1) & (c <= pm.grid).all(axis=1)
        gid = np.where(ok[:, None], c - 1, 0).astype(np.int64)
    return np.where(ok, OC.lin_of(gid, pm.grid), -1).astype(np.int32)


def neighbours7(lin, grid):
    """the voxels `lin` and their six neighbours clamped to the grid (map.py:545-557), ascending and unique"""
    ijk = np.stack(np.unravel_index(np.asarray(lin, dtype=np.int64), (grid,) * 3), axis=1)
    out = [np.asarray(lin, dtype=np.int64)]
    for d in range(3):
        for s in (-1, 1):
            q = ijk.copy()
            q[:, d] = np.clip(q[:, d] + s, 0, grid - 1)
            out.append(OC.lin_of(q, grid))
    return np.unique(np.concatenate(out))


class Restated:
    """What one integrate call leaves behind, integer state exactly and the rows the encoder sees."""


def restate(pm: IMap, xyz, normal, prune_min: int, th: float = TH) -> Restated:
    """One call on `pm`, which is advanced in place (indexer, pos, n, obs, dirty) — all but the latents: see fuse32."""
    xyz, normal = np.asarray(xyz, dtype=F32), np.asarray(normal, dtype=F32)
    r = Restated()
    r.N = N = xyz.shape[0]
    r.pt_lin = lin = voxel_ids(pm, xyz)
    valid = lin >= 0
    counts = np.bincount(lin[valid], minlength=pm.grid ** 3)                                     # map.py:374
    r.mask = (valid & ((counts[np.where(valid, lin, 0)] > prune_min) if prune_min > 0 else valid)).astype(np.uint8)      # map.py:375
    kept = lin[r.mask.astype(bool)].astype(np.int64)
    src = np.unique(kept[pm.indexer[kept] == -1])                                               # map.py:381-386
    cand = neighbours7(src, pm.grid) if src.size else np.zeros(0, dtype=np.int64)
    r.candidates = cand = cand[pm.indexer[cand] == -1]
    r.n_before, r.alloc_new = pm.n, int(cand.size)
    take = cand[:max(0, pm.capacity - pm.n)]                                                     # the capacity clamp: the lowest ids get the slots
    pm.indexer[take] = pm.n + np.arange(take.size)
    pm.pos[pm.n:pm.n + take.size] = take
    pm.n += int(take.size)
    r.overflow = int(r.n_before + r.alloc_new > pm.capacity)
    r.w_old, r.dirty_old = pm.obs.copy(), pm.dirty.copy()
    r.in_set = (pm.obs < F32(th)) & (pm.pos >= 0)                                               # map.py:407-411
    r.o, r.i, r.slot, r.rel = OC.gather_pairs(pm, xyz, r.mask, r.in_set)
    r.key = r.o * N + r.i                                                                        # the pair list's second word
    r.rows = np.concatenate([r.rel, normal[r.i]], axis=1).astype(F32).reshape(-1, 6)
    r.M = int(r.slot.size)
    r.uniq, r.inv, r.cnt = np.unique(r.slot, return_inverse=True, return_counts=True)
    r.C, r.items = int(r.uniq.size), (r.M + 31) >> 5
    pm.obs[r.uniq] = (pm.obs[r.uniq] + r.cnt.astype(F32)).astype(F32)                            # map.py:450
    pm.dirty[r.uniq] = 1
    r.n_after = pm.n
    return r


def fixed_sums(r: Restated, enc):
    """enc (M,29) float32, a row's encoder output -> (C,29) int64: sum over the voxel's rows of rint(e * 2^30) (k_encode's records, summed)"""
    q = np.rint(np.asarray(enc, dtype=np.float64) * FIX)
    q = np.where(np.isfinite(q), q, 0.0).astype(np.int64)
    out = np.zeros((r.C, 29), dtype=np.int64)
    np.add.at(out, r.inv, q)
    return out


def fuse32(z_old, w_old, Si, cnt):
    """k_fuse's three float32 operations (map.py:449-451) -> the new latents (C,29) and counts (C,)"""
    S = (np.asarray(Si, dtype=np.int64).astype(F32) * F32(1.0 / FIX)).astype(F32)
    w_old = np.asarray(w_old, dtype=F32)
    with np.errstate(invalid="ignore", over="ignore"):
        S = (S + (np.asarray(z_old, dtype=F32) * w_old[:, None]).astype(F32)).astype(F32)
        w_new = (w_old + np.asarray(cnt).astype(F32)).astype(F32)
        return (S / w_new[:, None]).astype(F32), w_new


def nonfinite_rows(rows):
    return ~np.isfinite(rows).all(axis=1)


def runs_of(pair_slot):
    """The run records of a pair list as k_encode cuts it: tiles of 32 consecutive entries, runs of equal slots inside a tile
    -> record id (tile * 32 + rank), slot, length, per run in list order."""
    s = np.asarray(pair_slot, dtype=np.int64)
    k = np.arange(s.size)
    head = np.ones(s.size, dtype=bool)
    head[1:] = (s[1:] != s[:-1]) | (k[1:] % 32 == 0)
    start = np.nonzero(head)[0]
    length = np.diff(np.append(start, s.size))
    tile = start // 32
    rank = np.arange(start.size) - np.searchsorted(tile, tile, side="left")
    return tile * 32 + rank, s[start], length


def workgroup_of(key, N, img=None):
    """the k_focus_gather workgroup that holds point i = key % N: 256 consecutive points, or a 16 x 16 pixel tile of an (H, W) image whose
    sides are multiples of 16"""
    i = np.asarray(key, dtype=np.int64) % N
    if img is not None and img[0] % 16 == 0 and img[1] % 16 == 0:
        return (i // img[1] // 16) * (img[1] // 16) + (i % img[1]) // 16
    return i // 256


def reach(r: Restated, img=None):
    """From the restatement alone: distinct slots of the fullest workgroup, and run records per slot if every (workgroup, slot) pair were
    ONE run (tile cuts only add to it) -> dict"""
    wg = workgroup_of(r.key, r.N, img)
    pairs = np.unique(np.stack([wg, r.slot], axis=1), axis=0) if r.M else np.zeros((0, 2), dtype=np.int64)
    per_wg = np.bincount(pairs[:, 0]) if r.M else np.zeros(1, dtype=np.int64)
    per_slot = np.bincount(pairs[:, 1], minlength=1) if r.M else np.zeros(1, dtype=np.int64)
    return dict(max_slots_per_wg=int(per_wg.max()), min_runs=int(per_slot[per_slot > 0].min()) if r.M else 0, max_runs=int(per_slot.max()))


# ---- the float64 bar ---------------------------------------------------------------------------------------------------------------
_NETS = {}


def nets(ws):
    """-> (Ref64, OracleNetworks) of a weight set (without mlp_cases.Bundle's decoder cases)"""
    if ws not in _NETS:
        from oracle import difusion_oracle as O
        from .ref64 import Ref64
        raw = C.weight_set(ws)
        _NETS[ws] = (Ref64(raw), O.OracleNetworks(raw))
    return _NETS[ws]


def mean_bar(ws, r: Restated):
    """-> mean64 (C,29), the bar (C,29), e_ref per group (8,)"""
    ref, oracle = nets(ws)
    e64 = ref.encoder(r.rows)
    e32 = oracle.encoder(r.rows)
    e_ref = np.array([C.max_err(e32[:, g], e64[:, g]) for g in C.ENC_GROUPS])
    s = np.zeros((r.C, 29), dtype=np.float64)
    np.add.at(s, r.inv, e64)
    mean64 = s / r.cnt[:, None]
    per_ch = np.zeros(29)
    for k, g in enumerate(C.ENC_GROUPS):
        per_ch[g] = e_ref[k]
    return mean64, C.K_BAR * per_ch[None, :] + 2.0 ** -31 + 2.0 * OC.spacing32(mean64), e_ref


# ---- cases -------------------------------------------------------------------------------------------------------------------------
class Case:
    """pm: the planted map before frame 0; frames: [(xyz, normal)]; prune_min; label; capacity is pm's"""

    def __init__(self, label, pm, frames, prune_min, img=None):
        self.label, self.pm, self.frames, self.prune_min, self.img = label, pm, frames, int(prune_min), img


def _planted(g, ijk, capacity, obs, grid=OC.GRID, voxel=OC.VOXEL):
    ijk = np.asarray(ijk, dtype=np.int64).reshape(-1, 3)
    lin = OC.lin_of(ijk, grid)
    order = np.argsort(lin)
    return IMap(lin, capacity, latents=(g.standard_normal((ijk.shape[0], 29)) * 0.3).astype(F32), obs=np.asarray(obs, dtype=F32)[order], grid=grid, voxel=voxel)


def faces_case(n: int, prune_min: int = 0, seed: int = 0):
    """Points exactly on voxel faces, at bound_min (invalid) and bound_max (the last voxel), one ulp inside and outside of each, NaN and
    +-Inf coordinates, -0.0, and ordinary points; n of them, the special ones first in a seeded order."""
    g = np.random.default_rng([73, seed, n])
    b = np.asarray(OC.BOUND_MIN, dtype=np.float64)
    top = (b + OC.GRID * OC.VOXEL).astype(F32)
    pool = []
    for k in (0, 1, 5, 8, 15, 16):                                     # faces of the grid and inside it
        f = (b + k * OC.VOXEL).astype(F32)
        for p in (f, np.nextafter(f, F32(np.inf)), np.nextafter(f, F32(-np.inf))):
            for d in range(3):
                q = OC.points_in([[5, 8, 11]], 0.37)[0]
                q[d] = p[d]
                pool.append(q)
            pool.append(p.copy())                                      # all three coordinates on the face: a voxel corner
    pool += [b.astype(F32), top, np.nextafter(top, F32(np.inf)), np.nextafter(top, F32(-np.inf))]
    for bad in (np.nan, np.inf, -np.inf):
        for d in range(3):
            q = OC.points_in([[7, 7, 7]], 0.5)[0]
            q[d] = bad
            pool.append(q)
    pool.append(np.array([-0.0, -0.0, -0.0], dtype=F32))              # xn = 8: the face between voxels 7 and 8
    pool.append(np.array([-0.0, 0.0, 0.1], dtype=F32))
    pool = np.array(pool, dtype=F32)
    pool = pool[g.permutation(pool.shape[0])]
    extra = OC.points_in(g.integers(4, 12, size=(max(n, 1), 3)), g.random((max(n, 1), 3)))
    xyz = np.concatenate([pool, pool[:40], extra])[:n]
    if n == 1:
        xyz = np.array([top], dtype=F32)                              # the one point: bound_max itself
    pm = _planted(g, [(7, 7, 7), (8, 8, 8), (15, 15, 15), (5, 8, 11)], 1024, [3.0, 700.0, TH - 1.0, TH])
    return Case(f"faces N={n} prune={prune_min}", pm, [(xyz, OC.unit_normals(g, n))], prune_min)


FACES_N = (1, 63, 64, 65, 255, 256, 257)


def runs_case(prune_min: int = 4, seed: int = 0):
    """300 consecutive points of one voxel (a run longer than a wave, across the workgroup edge at 256), runs that start at lane 0
    (point 320) and at lane 63 (point 383), voxels with exactly prune_min and prune_min + 1 points (4 and 5), and singles in between."""
    g = np.random.default_rng([79, seed])
    layout = [((6, 6, 6), 300), ((2, 3, 4), 4), ((9, 2, 2), 5), ((1, 1, 1), 1), ((12, 12, 3), 10),      # 320 points so far
              ((3, 9, 9), 63),                                                                              # a run from lane 0 of wave 5
              ((10, 10, 10), 70),                                                                           # from lane 63 of wave 5 into wave 7
              ((2, 3, 5), 4), ((2, 3, 6), 5), ((14, 1, 7), 17), ((6, 6, 7), 40), ((6, 6, 6), 9)]
    vox = np.concatenate([np.tile(np.array(v), (c, 1)) for v, c in layout])
    starts = np.cumsum([0] + [c for _, c in layout])
    assert starts[1] == 300 and starts[5] == 320 and starts[6] == 383
    n = vox.shape[0]
    xyz = OC.points_in(vox, 0.02 + 0.96 * g.random((n, 3)))
    pm = _planted(g, [(6, 6, 7), (12, 12, 3), (14, 14, 14)], 1024, [10.0, TH + 50.0, 5.0])
    return Case(f"runs prune={prune_min}", pm, [(xyz, OC.unit_normals(g, n))], prune_min)


def corners_case(seed: int = 0):
    """New voxels at the eight grid corners and on edges: clamped neighbours coincide with the voxel itself (three times in a corner)."""
    g = np.random.default_rng([83, seed])
    e = OC.GRID - 1
    vox = [(a, b, c) for a in (0, e) for b in (0, e) for c in (0, e)] + [(0, 0, 7), (0, 7, e), (7, e, e), (e, 0, 9), (0, 8, 8), (e, e, 1), (0, 1, 0)]
    vox = np.repeat(np.array(vox), 3, axis=0)
    n = vox.shape[0]
    xyz = OC.points_in(vox, 0.02 + 0.96 * g.random((n, 3)))
    pm = _planted(g, [(0, 0, 1), (e, e, e - 1), (8, 8, 8)], 1024, [20.0, 900.0, 1.0])
    return Case("corners", pm, [(xyz, OC.unit_normals(g, n))], 2)


def alloc64_case(seed: int = 0):
    """64^3 (8,192 bitmap words: the allocation scan takes k_scan_pass2 over 32 blocks of 256 words = two x-planes each, with
    k_prune_mark's block totals): 45 point voxels, no two neighbours, spread over the whole x range, on a map that already holds 40."""
    g = np.random.default_rng([89, seed])
    grid, voxel = 64, 0.05
    cells = np.stack(np.meshgrid(np.arange(1, 63, 3), np.arange(2, 62, 5), np.arange(2, 62, 5), indexing="ij"), axis=-1).reshape(-1, 3)
    pick = cells[np.sort(g.choice(cells.shape[0], size=85, replace=False))]
    have, new = pick[:85:2][:40], pick[1:85:2][:42]
    new = np.concatenate([new, [(0, 0, 0), (63, 63, 63), (31, 63, 0)]])
    pm = _planted(g, have, 1024, g.choice([5.0, TH - 1.0, TH, 900.0], size=have.shape[0]), grid=grid, voxel=voxel)
    vox = np.concatenate([np.repeat(new, 3, axis=0), np.repeat(have[:10], 3, axis=0)])
    n = vox.shape[0]
    xyz = OC.points_in(vox, 0.02 + 0.96 * g.random((n, 3)), voxel)
    return Case("alloc64", pm, [(xyz, OC.unit_normals(g, n))], 2)


def overflow_case(seed: int = 0):
    """The corners' cloud on a map whose capacity is 8 short of what the frame allocates"""
    c = corners_case(seed)
    q = c.pm.clone()
    need = restate(q, *c.frames[0], c.prune_min)
    cap = need.n_before + need.alloc_new - 8
    pm = IMap(c.pm.pos[:c.pm.n], cap, latents=c.pm.latent[:c.pm.n], obs=c.pm.obs[:c.pm.n])
    return Case("overflow", pm, c.frames, c.prune_min)


def threshold_case(seed: int = 0, n_frames: int = 3):
    """Planted counts th - 1, th and th + 1 (th = encoder_count_th as float32).  A voxel at th - 1 takes rows in frame 0, crosses, and is
    left alone from frame 1 on; a point inside a voxel at th + 1 (outside the set) beside one at th - 1 passes the focus test and feeds
    the neighbour alone."""
    g = np.random.default_rng([97, seed])
    th = float(F32(TH))
    vox = [(4, 4, 4), (4, 4, 5), (4, 4, 6), (8, 8, 8), (8, 8, 9), (11, 3, 3), (11, 3, 4), (2, 12, 12)]
    obs = [th - 1, th + 1, th, th - 1, th - 1, th + 1, th, 10.0]
    pm = _planted(g, vox, 1024, obs)
    pm.latent[pm.indexer[OC.lin_of([2, 12, 12])], :3] = (NaN_PAYLOAD, F32(-0.0), F32(1e-40))
    frames = []
    for f in range(n_frames):
        src = np.repeat(np.array([(4, 4, 5), (4, 4, 4), (4, 4, 6), (8, 8, 8), (8, 8, 9), (11, 3, 3), (11, 3, 4), (13, 13, 2)]), 6, axis=0)
        n = src.shape[0]
        frames.append((OC.points_in(src, 0.02 + 0.96 * g.random((n, 3))), OC.unit_normals(g, n)))
    return Case("threshold", pm, frames, 2)


CHAIN_N, CHAIN_PAD = 8192, 37


def chain_case(seed: int = 0, n_frames: int = 3, nonfinite: bool = False):
    """N = 8,192: 7,412 points in random order over a 3 x 3 x 3 block (every block voxel is fed by all 30 workgroups of the shuffled part:
    more runs than the 14 its directory holds), 40 isolated voxels of 3 to 6 points among them, and a tail of 600 points in 600 different
    voxels, in order (its workgroups see more than the 256 slots of k_focus_gather's table).  prune_min_vox_obs = 0: the tail's points
    stand alone.  A voxel far from all of it holds a NaN payload, -0.0 and a subnormal and is never in the update list."""
    g = np.random.default_rng([101, seed])
    iso = OC.isolated_voxels(60, g)
    iso = iso[((iso < 4) | (iso > 10)).any(axis=1)][:40]
    assert iso.shape[0] == 40
    pm = _planted(g, [(14, 14, 14), (1, 14, 1)], 4096, [TH + 1.0, TH])
    pm.latent[pm.indexer[OC.lin_of([14, 14, 14])], :3] = (NaN_PAYLOAD, F32(-0.0), F32(1e-40))
    frames = []
    for f in range(n_frames):
        per = g.integers(3, 7, size=40)
        iso_pts = np.repeat(iso, per, axis=0)
        n_block = CHAIN_N - 600 - iso_pts.shape[0]
        block = 6 + g.integers(0, 3, size=(n_block, 3))
        head = np.concatenate([block, iso_pts])
        head = head[g.permutation(head.shape[0])]
        cells = np.stack(np.unravel_index(g.choice(OC.GRID ** 3, size=600, replace=False), (OC.GRID,) * 3), axis=1)
        vox = np.concatenate([head, cells])
        xyz = OC.points_in(vox, 0.02 + 0.96 * g.random((CHAIN_N, 3)))
        nrm = OC.unit_normals(g, CHAIN_N)
        if nonfinite and f == 0:
            for k, (i, d, v) in enumerate([(11, 0, np.nan), (1000, 1, np.inf), (4097, 2, -np.inf), (7000, 1, np.nan), (CHAIN_N - 300, 0, np.inf)]):
                nrm[i, d] = v
        frames.append((xyz, nrm))
    return Case("chain" + ("/non-finite normals" if nonfinite else ""), pm, frames, 0)


def unproject32(depth, normal_cam, pose, intr):
    """csrc/kernels_points.hip.h: unproject_point, operation for operation in float32 -> xyz (H*W,3), normal (H*W,3); NaN where depth is"""
    H, W = depth.shape
    fx, fy, cx, cy = (F32(v) for v in intr)
    R, t = np.asarray(pose[:9], dtype=F32), np.asarray(pose[9:], dtype=F32)
    v, u = np.meshgrid(np.arange(H, dtype=F32), np.arange(W, dtype=F32), indexing="ij")
    d = depth.astype(F32)
    with np.errstate(invalid="ignore"):
        x = (((u - cx) / fx) * d).astype(F32)
        y = (((v - cy) / fy) * d).astype(F32)
        rot = lambda k, a, b, c: ((R[k] * a + R[k + 1] * b).astype(F32) + R[k + 2] * c).astype(F32)
        p = np.stack([(rot(k, x, y, d) + t[k // 3]).astype(F32) for k in (0, 3, 6)], axis=-1)
        a, b, c = (normal_cam[..., k].astype(F32) for k in range(3))
        nv = np.stack([rot(k, a, b, c) for k in (0, 3, 6)], axis=-1)
    nv[np.isnan(d)] = np.nan
    return p.reshape(-1, 3).astype(F32), nv.reshape(-1, 3).astype(F32)


def frame_case(H: int, W: int, seed: int = 0):
    """A depth image of a tilted wall about 1.3 in front of a camera with a non-trivial pose, NaN holes and zeros in the depth (a zero
    depth is a valid point at the camera centre).  32 x 48: both sides multiples of 16, k_focus_gather walks 16 x 16 tiles; 24 x 40: the
    flat walk."""
    g = np.random.default_rng([103, seed, H, W])
    intr = (40.0, 42.0, W / 2 - 0.5, H / 2 - 0.25)
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    depth = (1.3 + 0.012 * (u - W / 2) - 0.009 * (v - H / 2) + 0.02 * g.standard_normal((H, W))).astype(F32)
    depth[g.random((H, W)) < 0.06] = np.nan
    depth[g.random((H, W)) < 0.02] = 0.0
    depth[3:6, 7:12] = np.nan
    ncam = OC.unit_normals(g, H * W).reshape(H, W, 3)
    a, b = 0.3, -0.2
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    pose = np.concatenate([(Rz @ Rx).reshape(-1), [0.11, -0.07, -1.0]]).astype(F32)
    xyz, nrm = unproject32(depth, ncam, pose, intr)
    pm = _planted(g, [(8, 8, 9), (8, 7, 9), (3, 3, 3)], 2048, [TH - 1.0, TH + 1.0, 5.0])
    c = Case(f"frame {H}x{W}", pm, [(xyz, nrm)], 4, img=(H, W))
    c.depth, c.normal_cam, c.pose, c.intr = depth, ncam, pose, intr
    return c


def frame_descriptor(depth_ptr: int, normal_ptr: int, pose) -> bytes:
    """dif_frame_t: two device pointers and the pose, 64 bytes"""
    return struct.pack("<QQ12f", depth_ptr, normal_ptr, *[float(x) for x in pose])


WEIGHT_SETS = ("shipped", "hostile_a")
