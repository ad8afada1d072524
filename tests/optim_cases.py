"""Planted maps, the gather restated in NumPy, the cases and the bar for the latent optimiser's tests (tests/test_ref64_cpu.py on the CPU,
tests/test_gpu_optim_envelope.py on the GPU).  TEST INFRASTRUCTURE ONLY; everything here is a deterministic function of its seed.

THE BAR of a per-voxel gradient sum G[u, c] (channel c of voxel u; `nll_bar`):
    e_gpu <= K_NLL * e_ref + rows(u) * 2^-41 + 1 ulp of G + U_NLL ulp of S[u, c]
  e_ref  the worst error, over the case's voxels and channels, of the float32 oracle's per-voxel sums (OracleNetworks.decoder_nll_grad,
         np.add.at) against float64 (Ref64.decoder_nll_grad);
  2^-41  per row: k_optim_grad rounds every row's gradient to a multiple of 2^-40 before its exact integer sum;
  1 ulp  the conversion of the integer sum back to float32 (k_optim_adam) rounds once; a whole ulp covers a binade edge;
  S      sum over the voxel's rows of |sdf-head part| + |uncertainty-head part| of the row's gradient: what a relative error of the
         upstream heads a, b acts on (the parts may cancel in G, their errors do not).
"""
from __future__ import annotations

import numpy as np

from . import mlp_cases as C

F32 = np.float32
GRID = 16
BOUND_MIN = (-1.6, -1.6, -1.6)
VOXEL = 0.2
ENC_TH = 600.0
FIX_HALF = 2.0 ** -41                     # half a unit of DIF_OPT_FIX_SCALE = 2^40

# K of the gradient bar: twice the largest ratio between the worst errors (against float64) of three honest float32 evaluations of the
# per-voxel gradient sums of the cases below: the oracle (BLAS order), torch float32 autograd, strict left-to-right accumulation.
# Measured on the CPU by tests/test_ref64_cpu.py::test_k_of_the_bar (rows "nll gradient" of profiles/mlp_envelope_k.md); never from a kernel.
#   largest ratio measured: 2.96 (hostile_b, N(0,0.3): 7.03e-7 oracle, 2.40e-7 torch, 7.11e-7 sequential; and hostile_b, "pu near 10");
#   torch's threaded float32 sums move it between 2.8 and 3.0 from run to run
K_NLL = 6.0
# U_NLL: the ulp errors the HIP math API documents for the device functions, as they enter the two upstream heads of mlp.hip.h
#   a = inv_n * (-(g - mu) / var) * (1 - sdf^2),     b = inv_n * (1 / std - diff^2 / (var * std)) * 0.5 * sigmoid(pu)
# with sdf = tanhf(ps) (1 ulp), std = 0.05 + 0.5 * (pu > 20 ? pu : log1pf(expf(pu))) (expf 1 + log1pf 1 = 2 ulp), sigmoid = 1 / (1 + expf(-pu))
# (expf 1 ulp).  logf enters the loss only, not a or b.
#   a:  mu carries tanhf once (1), 1 - sdf^2 twice (2), var = std^2 carries std twice (4)                                  -> 7
#   b:  the larger term diff^2 / (var * std) carries tanhf twice (2) and std three times (6), the sigmoid expf once (1)    -> 9
# Each is relative to the head's own magnitude, hence to its part of the row's gradient (the chain behind a, b is linear): U_NLL ulp of S.
# (Where diff = g - mu cancels, tanhf's error is absolute: at most ulp(0.2) = 2^-26 against a diff of up to 0.4, which the count covers.)
U_NLL = 9.0


def spacing32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(F32)).astype(np.float64)


def nll_bar(e_ref: float, rows_u, G64, S, k=None):
    """(U,29) bar of the per-voxel gradient sums; rows_u (U,): rows of each voxel."""
    return (K_NLL if k is None else k) * e_ref + np.asarray(rows_u, dtype=np.float64)[:, None] * FIX_HALF + spacing32(G64) + U_NLL * spacing32(S)


# ---- planted maps ---------------------------------------------------------------------------------------------------------------
class Planted:
    """The state of a grid^3 map (16^3 unless said otherwise) with the voxels `lin` allocated in ascending id order (allocate_block,
    map.py:310-319), as NumPy arrays."""

    def __init__(self, lin, capacity: int, latents=None, obs=None, optimized=None, grid: int = GRID, voxel: float = VOXEL):
        lin = np.sort(np.asarray(lin, dtype=np.int64))
        assert np.unique(lin).size == lin.size and lin.size <= capacity
        self.n, self.capacity, self.grid = int(lin.size), int(capacity), int(grid)
        self.bound_min, self.voxel_size = np.asarray(BOUND_MIN, dtype=F32), voxel
        self.indexer = -np.ones(self.grid ** 3, dtype=np.int64)
        self.indexer[lin] = np.arange(self.n)
        self.pos = -np.ones(capacity, dtype=np.int64)
        self.pos[:self.n] = lin
        self.obs = np.zeros(capacity, dtype=F32)
        self.obs[:self.n] = 1000.0 if obs is None else obs
        self.optimized = np.zeros(capacity, dtype=np.uint8)
        if optimized is not None:
            self.optimized[:self.n] = optimized
        self.latent = np.zeros((capacity, 29), dtype=F32)
        if latents is not None:
            self.latent[:self.n] = latents

    def in_set(self):
        """(capacity,) bool: map.py:465-467"""
        return (self.obs >= F32(ENC_TH)) & (self.optimized == 0) & (self.pos > 0)

    def slot_of(self, ijk):
        return self.indexer[lin_of(ijk, self.grid)]


def lin_of(ijk, grid: int = GRID):
    ijk = np.asarray(ijk, dtype=np.int64)
    return ijk[..., 2] + grid * ijk[..., 1] + grid * grid * ijk[..., 0]


def points_in(ijk, frac, voxel: float = VOXEL):
    """World points at fraction `frac` (in (0, 1]) of voxels `ijk` -> float32 (N,3)"""
    return ((np.asarray(ijk, dtype=np.float64) + frac) * voxel + np.asarray(BOUND_MIN, dtype=np.float64)).astype(F32)


# ---- the gather (map.py:459-497), restated with the oracle's float32 operations ------------------------------------------------------
OFFSETS = np.array([[(-0.5, 0.5)[(o >> 2) & 1], (-0.5, 0.5)[(o >> 1) & 1], (-0.5, 0.5)[o & 1]] for o in range(8)], dtype=F32)      # map.py:186-189


def gather_pairs(pm: Planted, xyz, mask, in_set=None):
    """The (offset, point) pairs that become rows, in the reference's order (offset-major, then point order)
    -> o (R,), i (R,), slot (R,) int64, rel (R,3) float32 (the unperturbed position relative to the row's voxel).
    in_set (capacity,) bool: the slots that take rows — the optimiser's set (pm.in_set(), map.py:465-467) unless given; integrate's gather
    (map.py:389-433) is the same walk over its encode set {obs < encoder_count_th} (tests/integrate_cases.py)."""
    GRID = pm.grid
    xyz = np.asarray(xyz, dtype=F32)
    with np.errstate(invalid="ignore", over="ignore"):
        xn = ((xyz - pm.bound_min[None, :]) / F32(pm.voxel_size)).astype(F32)            # map.py:366-367
        c = np.ceil(xn)
        ok = np.asarray(mask).astype(bool) & (c >= 1).all(axis=1) & (c <= GRID).all(axis=1)      # NaN fails every comparison
        gid = np.where(ok[:, None], c - 1, 0).astype(np.int64)
    in_set = pm.in_set() if in_set is None else np.asarray(in_set, dtype=bool)
    status = np.zeros(GRID ** 3, dtype=bool)
    status[pm.pos[in_set]] = True
    # get_pruned_surface (map.py:389-399): the point's own voxel or one of its six neighbours, clamped to the grid, is in the set
    exp = status.copy()
    ijk = np.stack(np.unravel_index(np.nonzero(status)[0], (GRID,) * 3), axis=1)
    for d in range(3):
        for s in (-1, 1):
            q = ijk.copy()
            q[:, d] = np.clip(q[:, d] + s, 0, GRID - 1)
            exp[lin_of(q, GRID)] = True
    focus = ok & exp[lin_of(gid, GRID)]
    idx = np.nonzero(focus)[0]
    pxn = xn[idx]
    o_all, i_all, s_all, r_all = [], [], [], []
    for o, off in enumerate(OFFSETS):                                                    # map.py:479-493
        g = np.clip(np.ceil((pxn + off[None, :]).astype(F32)) - F32(1), 0, GRID - 1).astype(F32)
        rel = ((pxn - g).astype(F32) - F32(0.5)).astype(F32)
        lin = lin_of(g.astype(np.int64), GRID)
        m = status[lin]
        o_all.append(np.full(int(m.sum()), o, dtype=np.int64))
        i_all.append(idx[m])
        s_all.append(pm.indexer[lin][m])
        r_all.append(rel[m])
    return np.concatenate(o_all), np.concatenate(i_all), np.concatenate(s_all), np.concatenate(r_all).reshape(-1, 3)


def gather_rows(pm: Planted, xyz, normal, mask, noise):
    """-> row_slot (R,) int32, row_xyz (R,3), row_sdf (R,) float32: row k takes noise[k] (map.py:489-490)"""
    o, i, slot, rel = gather_pairs(pm, xyz, mask)
    sdf = (np.asarray(noise[:slot.size], dtype=F32) * F32(0.05)).astype(F32)
    row_xyz = (rel + (sdf[:, None] * np.asarray(normal, dtype=F32)[i]).astype(F32)).astype(F32)
    return slot.astype(np.int32), row_xyz, sdf


def noise_in_row_order(pm, xyz, mask, table):
    """table (N,8): the perturbation sample of every (point, offset) -> the 8N-float noise array whose k-th entry belongs to row k"""
    o, i, _, _ = gather_pairs(pm, xyz, mask)
    out = np.zeros(8 * xyz.shape[0], dtype=F32)
    out[:o.size] = table[i, o]
    return out


# ---- cases ----------------------------------------------------------------------------------------------------------------------
def planted_noise(g, shape, tail=0.01):
    """N(0,1) samples of which about `tail` lie beyond 4 sigma (|0.05 * noise| > 0.2, the target's clamp, needs one)"""
    t = g.standard_normal(shape)
    far = g.random(shape) < tail
    return np.where(far, np.sign(t) * (4.0 + np.abs(g.standard_normal(shape))), t).astype(F32)


def unit_normals(g, n):
    v = g.standard_normal((n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)


class Case:
    """One optimiser run: a planted map, the points (already filtered), the noise in row order, and the float64 / float32 statements of
    its first gradient."""

    def __init__(self, b, pm, xyz, normal, table, label, cap=0.05, filter_points=True):
        self.b, self.pm, self.label = b, pm, label
        mask = np.ones(xyz.shape[0], dtype=np.uint8)
        dropped = np.zeros(xyz.shape[0], dtype=bool)
        if filter_points:
            o, i, slot, rel = gather_pairs(pm, xyz, mask)
            sdf = (table[i, o] * F32(0.05)).astype(F32)
            rows = np.concatenate([pm.latent[slot], (rel + (sdf[:, None] * normal[i]).astype(F32)).astype(F32)], axis=1)
            on_kink = self.rows_on_a_kink(b, rows)
            dropped[np.unique(i[on_kink])] = True
            self.kink_rows = float(on_kink.mean())
        self.dropped = float(dropped.mean())
        assert self.dropped <= cap, f"{label}: {self.dropped:.2%} of the candidate points sit on a kink"
        self.xyz, self.normal, table = xyz[~dropped], normal[~dropped], table[~dropped]
        self.mask = np.ones(self.xyz.shape[0], dtype=np.uint8)
        self.noise = noise_in_row_order(pm, self.xyz, self.mask, table)
        self.row_slot, self.row_xyz, self.row_sdf = gather_rows(pm, self.xyz, self.normal, self.mask, self.noise)
        self.n_rows = int(self.row_slot.size)
        self.uniq, self.inv = np.unique(self.row_slot, return_inverse=True)
        self.rows_u = np.bincount(self.inv, minlength=self.uniq.size)

    @staticmethod
    def rows_on_a_kink(b, rows):
        """rows whose gradient float32 cannot be held to: a hidden pre-activation inside Bundle.grad_keep's margin, or |sdf| within the
        sdf bar (K_BAR * e_ref of the rows' sdf + 1 ulp) of the clamp at 0.2"""
        sdf64 = b.ref.decoder(rows)[0]
        e_sdf = C.max_err(b.oracle.decoder(rows)[0][:, 0], sdf64)
        return ~b.grad_keep(rows) | (np.abs(np.abs(sdf64) - 0.2) < C.bar(e_sdf, 1.0, C.U_SDF))

    def rows_at(self, z_u):
        """decoder rows [latent of the row's voxel | row_xyz] for the per-voxel latents z_u (U,29)"""
        return np.concatenate([np.asarray(z_u)[self.inv], self.row_xyz], axis=1)

    def sums(self, per_row):
        out = np.zeros((self.uniq.size,) + per_row.shape[1:], dtype=per_row.dtype)
        np.add.at(out, self.inv, per_row)
        return out

    def grad64(self, z_u=None):
        """float64 at the per-voxel latents z_u (default: the planted ones) -> dict(G (U,29), S (U,29), loss (scalar), loss_abs, r: per row)"""
        z_u = self.pm.latent[self.uniq] if z_u is None else z_u
        r = self.b.ref.decoder_nll_grad(self.rows_at(np.asarray(z_u, dtype=np.float64)), self.row_sdf, self.n_rows)
        return dict(G=self.sums(r["grad"][:, :29]), S=self.sums(r["grad_abs"][:, :29]), loss=float(r["loss"].sum()), loss_abs=float(np.abs(r["loss"]).sum()), r=r)

    def grad32(self, z_u=None):
        """the float32 oracle's -> G (U,29) float32, loss"""
        z_u = self.pm.latent[self.uniq] if z_u is None else z_u
        loss, gx, _, _ = self.b.oracle.decoder_nll_grad(self.rows_at(np.asarray(z_u, dtype=F32)).astype(F32), self.row_sdf, self.n_rows)
        return self.sums(gx[:, :29]), loss

    def e_ref(self, z_u=None, keep=None):
        g64, g32 = self.grad64(z_u)["G"], self.grad32(z_u)[0]
        keep = slice(None) if keep is None else keep
        return C.max_err(g32[keep], g64[keep])


def block_case(ws: str, scale: float, seed: int = 0, side: int = 5, n_points: int = 1000, capacity: int = 1024):
    """A side^3 block of allocated voxels in the middle of the grid, latents N(0, scale).  Half of them are in the optimisation set; the
    others are below encoder_count_th or already optimised, so a point gives about four rows, in different voxels (a voxel's rows are
    scattered over the tiles), and 8 rows of a dropped point cost less of the cap.  A quarter of the voxels take, of eight N(0, scale)
    draws, the one whose float64 sdf pre-activation at the voxel's centre is smallest: random decoders (and large latents) saturate
    tanh nearly everywhere, and the clamp's inside, |sdf| <= 0.2, has to be reached too."""
    b = C.bundle(ws)
    g = np.random.default_rng([41, seed, C.WEIGHT_SETS.index(ws), int(scale * 10)])
    lo = 4
    ijk = np.stack(np.meshgrid(*[np.arange(lo, lo + side)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    nv = ijk.shape[0]
    draws = (g.standard_normal((nv, 8, 29)) * scale).astype(F32)
    ps = b.ref.decoder(np.concatenate([draws.reshape(-1, 29), np.zeros((nv * 8, 3), dtype=F32)], axis=1))[2].reshape(nv, 8)
    pick = np.where(g.random(nv) < 0.25, np.abs(ps).argmin(axis=1), 0)
    kind = g.integers(0, 4, size=nv)                          # 0, 1: in the set; 2: too few observations; 3: optimised before
    pm = Planted(lin_of(ijk), capacity, latents=draws[np.arange(nv), pick], obs=np.where(kind == 2, 100.0, 1000.0).astype(F32),
                 optimized=(kind == 3).astype(np.uint8))
    inner = ijk[((ijk > lo) & (ijk < lo + side - 1)).all(axis=1)]
    vox = inner[g.integers(0, inner.shape[0], size=n_points)]
    xyz = points_in(vox, 0.02 + 0.96 * g.random((n_points, 3)))
    return Case(b, pm, xyz, unit_normals(g, n_points), planted_noise(g, (n_points, 8)), f"{ws}/N(0,{scale:g})")


def isolated_voxels(n_voxels: int, g):
    """ijk of `n_voxels` voxels no two of which are neighbours (every second cell of the inner grid), none on lin id 0"""
    cells = np.stack(np.meshgrid(*[np.arange(1, GRID - 1, 2)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    return cells[np.sort(g.choice(cells.shape[0], size=n_voxels, replace=False))]


def one_octant_points(ijk, rel):
    """Points of voxels `ijk` at relative position `rel` in (-0.5, 0.5): with isolated set voxels each point gives exactly one row, in its
    own voxel.  Rows come offset-major, and which offset leads to the point's own voxel depends on the octant it lies in: with every
    `rel` in ONE octant (all components positive) rows equal points, in point order."""
    return points_in(ijk, 0.5 + np.asarray(rel, dtype=np.float64))


def large_pu_case(seed: int = 0, n_voxels: int = 96, per_voxel: int = 12, capacity: int = 1024):
    """Shipped weights reach pu > 20 only along rare latent directions: isolated voxels take the latents of decoder_rows_large_pu's
    (20, 88] rows, and their points sit near those rows' own xyz."""
    b = C.bundle("shipped")
    g = np.random.default_rng([43, seed])
    src = b.dec["pu(20,88]"][g.choice(C.N_ROWS, size=n_voxels, replace=False)]
    ijk = isolated_voxels(n_voxels, g)
    pm = Planted(lin_of(ijk), capacity, latents=src[:, :29])
    order = np.argsort(lin_of(ijk))          # Planted sorts by lin id; isolated_voxels is already ascending in cell index = lin order
    assert np.array_equal(order, np.arange(n_voxels))
    rel = np.clip(np.repeat(src[:, 29:], per_voxel, axis=0) + 0.02 * g.standard_normal((n_voxels * per_voxel, 3)), -0.45, 0.45)
    xyz = one_octant_points(np.repeat(ijk, per_voxel, axis=0), rel)
    n = xyz.shape[0]
    return Case(b, pm, xyz, unit_normals(g, n), planted_noise(g, (n, 8)), "shipped/large pu")


def near_switch_case(ws: str, seed: int = 0, n_voxels: int = 96, per_voxel: int = 12, capacity: int = 1024):
    """Where softplus' derivative still differs from 1 by more than float32 resolves: isolated voxels with the latents of the
    n_voxels rows of the "pu(10,20]" case whose float64 pu is smallest (10.2 .. 11), points near those rows' own xyz.  A switch to
    `1` placed at 10 instead of 20 is off by e^-10 = 4.5e-5 of the uncertainty head's part there; above 12 float32 no longer sees it."""
    b = C.bundle(ws)
    g = np.random.default_rng([71, seed])
    src = b.dec["pu(10,20]"][np.argsort(b.dec64["pu(10,20]"][3])[:n_voxels]]
    ijk = isolated_voxels(n_voxels, g)
    pm = Planted(lin_of(ijk), capacity, latents=src[:, :29])
    rel = np.clip(np.repeat(src[:, 29:], per_voxel, axis=0) + 0.02 * g.standard_normal((n_voxels * per_voxel, 3)), -0.45, 0.45)
    xyz = one_octant_points(np.repeat(ijk, per_voxel, axis=0), rel)
    n = xyz.shape[0]
    return Case(b, pm, xyz, unit_normals(g, n), planted_noise(g, (n, 8)), f"{ws}/pu near 10")


ONE_STEP = [(ws, s) for ws in C.WEIGHT_SETS for s in (0.3, 4.0)]
NEAR_SWITCH = -10.0                       # the "scale" that names near_switch_case in one_step_case
_CASES = {}


def one_step_case(ws, scale):
    if (ws, scale) not in _CASES:
        _CASES[ws, scale] = large_pu_case() if ws == "large_pu" else near_switch_case(ws) if scale == NEAR_SWITCH else block_case(ws, scale)
    return _CASES[ws, scale]


# ---- scenes for the gather ------------------------------------------------------------------------------------------------------
def messy_scene(n_points: int, capacity: int, seed: int):
    """A map and points that meet every clause of the gather: set voxels on all six grid faces and in corners (clamped neighbours), an
    allocated voxel at lin id 0 (never optimised, map.py:467), voxels below encoder_count_th and already optimised ones mixed in,
    neighbours that are not allocated, and points with mask 0, NaN coordinates or positions outside the grid (also exactly on a voxel
    boundary).  -> Planted, xyz (N,3), normal (N,3), mask (N,) uint8, noise (8N,)"""
    g = np.random.default_rng([47, seed, n_points])
    e = GRID - 1
    faces = [(0, 5, 5), (e, 5, 5), (5, 0, 5), (5, e, 5), (5, 5, 0), (5, 5, e), (0, 0, 0), (e, e, e), (0, e, 0), (0, 0, 1), (1, 5, 5), (5, 1, 5), (3, 12, 3)]
    cluster = [(i, j, k) for i in (8, 9, 10) for j in (8, 9, 10) for k in (8, 9, 10)]
    ijk = np.array(sorted(set(faces + cluster)), dtype=np.int64)
    nv = ijk.shape[0]
    kind = g.choice(4, size=nv, p=[0.35, 0.35, 0.15, 0.15])            # 0, 1: in the set; 2: too few observations; 3: optimised before
    kind[: len(faces)] = np.where(g.random(len(faces)) < 0.8, 0, kind[: len(faces)])      # (sorted order mixes these; most face voxels stay in the set)
    pm = Planted(lin_of(ijk), capacity, latents=(g.standard_normal((nv, 29)) * 0.3).astype(F32), obs=np.where(kind == 2, 599.0, 600.0).astype(F32),
                 optimized=(kind == 3).astype(np.uint8))
    # points in allocated voxels and in their (often unallocated, sometimes out-of-grid) neighbours
    base = ijk[g.integers(0, nv, size=n_points)] + g.integers(-1, 2, size=(n_points, 3)) * (g.random((n_points, 1)) < 0.4)
    frac = g.random((n_points, 3))
    frac = np.where(g.random((n_points, 3)) < 0.05, g.choice([0.5, 1.0], size=(n_points, 3)), np.maximum(frac, 1e-3))
    xyz = points_in(base, frac)
    bad = g.random(n_points)
    xyz[bad < 0.03, g.integers(0, 3)] = np.nan
    far = (bad >= 0.03) & (bad < 0.06)
    xyz[far] = (xyz[far] + g.choice(np.array([-1e6, -3.3, 3.3, np.inf], dtype=F32), size=(int(far.sum()), 3))).astype(F32)
    mask = (g.random(n_points) >= 0.1).astype(np.uint8)
    return pm, xyz, unit_normals(g, n_points), mask, planted_noise(g, 8 * n_points)


def isolated_scene(n_rows: int, capacity: int, seed: int, n_voxels: int = 3, ws_latents=None):
    """`n_voxels` isolated set voxels and n_rows points inside them: rows equal points, in point order"""
    g = np.random.default_rng([53, seed, n_rows])
    ijk = isolated_voxels(n_voxels, g)
    pm = Planted(lin_of(ijk), capacity, latents=(g.standard_normal((n_voxels, 29)) * 0.3).astype(F32) if ws_latents is None else ws_latents)
    vox = g.integers(0, n_voxels, size=n_rows)
    xyz = one_octant_points(ijk[vox], 0.02 + 0.43 * g.random((n_rows, 3)))
    return pm, xyz, unit_normals(g, n_rows), np.ones(n_rows, dtype=np.uint8), planted_noise(g, 8 * n_rows), vox
