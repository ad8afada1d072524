"""The extract chain (dif_extract / dif_extract_streams: csrc/kernels_extract.hip.h, the marching-cubes and log half of csrc/kernels_mesh.hip.h)
stage by stage and plan by plan: its lists, its idle state, its refine list, its log and every limit, bit for bit against the restatements of
tests/extract_cases.py (pinned on the CPU by tests/test_extract_cpu.py).  Every call goes through ctypes on planted maps; every buffer a call may
write sits between guard words and holds the fill byte 0xA5 (or its idle value) before the call.  Nothing here has a tolerance but the one
comparison test_gpu_map.py already makes (the triangles against the C marching cubes on the GPU's own cubes, 1e-5).

THE PLANS (extract_plan, csrc/difusion.hip) AND HOW A TEST KNOWS WHICH ONE RAN
  dirty scan   BlockTotals: capacity 8192 with dirty_tot (it DEFERS where the others overflow with code 2: test_max_voxels_limits);
               BoundedTotals: capacity 1024 with dirty_tot (one workgroup: k_scan_single) and capacity 5000 (k_scan_pass2_fixed over dirty_tot);
               Generic: dirty_tot NULL (capacity 5000 / 8192: two launches, block_tmp is written) or no_cache.
  decode       Exact: VH = 0, low_* and fold_table untouched; TwoLevel (r = 8): low_* written; FusedF32 / FusedX6: low_* untouched, fold_table
               written iff the chain folds (FusedX6 always; FusedF32 with fold_table = NULL does not).  The two pipes differ in their cubes' bits.
  marching     CountScanEmit: tri_offset written; CountEmit: tri_offset untouched and the refine list overwritten by the parked corners;
  cubes        OnePass: tri_offset untouched and the refine list intact behind VH (so the refine list is inspected under OnePass, or where no voxel
               of the call has corners to park: test_two_level_r8).
"""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from di_fusion_amd import _lib
from di_fusion_amd.network import utility as net_util
from oracle import difusion_oracle as O
from tests import extract_cases as EC
from tests import integrate_cases as IC
from tests import mlp_cases as C
from tests.test_gpu_optim_envelope import DEV, _guarded, _guards_intact, bits

pytestmark = pytest.mark.gpu
F32 = np.float32
MAX_STD = 0.15
AMPLE = 10 ** 6
SCANS = ("block", "bounded", "generic1k", "generic8k")
CAPACITY = dict(block=8192, generic8k=8192, bounded=1024, generic1k=1024, bounded5k=5000, generic5k=5000)
DECODES = ("fused_x6", "fused_f32", "fused_f32_fold", "exact")
CHAINS = ("onepass", "count_emit", "count_scan_emit")
PER_CALL = ("valid_blocks", "occ_slot", "low_sdf", "low_std", "cube_sdf", "cube_std", "refine_list", "tri_count", "tri_offset", "block_tmp", "fold_table",
            "out_tri", "out_id", "out_std", "counters_out")
IDLE_ZERO = ("grid_bits", "grid_tot", "chunk_sum", "mc_status")


@pytest.fixture(scope="module")
def nets():
    cache = {}

    def get(ws, x6):
        if (ws, x6) not in cache:
            cache[ws, x6] = net_util.networks_from_arrays(C.weight_set(ws), x6=x6)
        return cache[ws, x6]
    return get


@pytest.fixture(scope="module")
def case1k():
    return EC.planted(1024)


@pytest.fixture(scope="module")
def case8k():
    return EC.planted(8192)


def _t(a, dt=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(DEV)


def _filled(a):
    """every byte of `a` is still the fill byte"""
    return bool((np.ascontiguousarray(a).view(np.uint8) == EC.FILL).all())


class Device:
    """A planted map on the GPU with its extract buffers, every one of them guarded, and calls of the extract entry points on it."""

    def __init__(self, pm, model, r=4, dirty_tot=True, max_voxels=None, cache_capacity=4096, out_capacity=16, chunk=True, status=True, fold=True,
                 own=None, rows=None):
        """rows: the rows the per-voxel buffers HAVE where that is more than the max_voxels the call states (a later call may then state more)"""
        self.pm, self.model, self.r, self.has_tot = pm, model, r, bool(dirty_tot)
        cap, G = pm.capacity, pm.grid ** 3
        stated = int(pm.n if max_voxels is None else max_voxels)
        self.mv = mv = max(stated, int(rows or 0))
        self.R3, self.l3, self.cc, self.oc = (2 * r) ** 3, r ** 3, int(cache_capacity), int(out_capacity)
        i32, i64, f32, u8 = torch.int32, torch.int64, torch.float32, torch.uint8
        shapes = dict(latent=(cap * 29, f32), obs=(cap, f32), dirty=(cap, u8), indexer=(G, i64), pos=(cap, i64), counters=(_lib.C_COUNT, i32),
                      grid_bits=((G + 31) // 32, i32), grid_tot=(1024, i32), vbm=(cap, i32), tri_start=(cap, i32), tri_n=(cap, i32),
                      dirty_tot=((cap + 255) // 256, i32), pending=(32, i32),
                      valid_blocks=(mv, i64), occ_slot=(mv, i32), low_sdf=(mv * self.l3, f32), low_std=(mv * self.l3, f32), cube_sdf=(mv * self.R3, f32),
                      cube_std=(mv * self.R3, f32), refine_list=(mv * self.R3, i32), tri_count=(mv, i32), tri_offset=(mv, i32), block_tmp=(4096, i32),
                      cache_tri=(self.cc * 9, f32), cache_id=(self.cc, i64), cache_std=(self.cc * 3, f32), cache_alive=(self.cc, u8),
                      counters_out=(_lib.C_COUNT, i32), out_tri=(self.oc * 9, f32), out_id=(self.oc, i64), out_std=(self.oc * 3, f32),
                      chunk_sum=((mv + 255) // 256 + (mv + 65535) // 65536, i32), fold_table=(mv * 256, f32), mc_status=((mv + 3) // 4 + 256, i32))
        self.guard, self.names = {}, tuple(shapes)
        for name, (n, dt) in shapes.items():
            self.guard[name], view = _guarded(max(n, 1), dt)
            view.view(u8).fill_(EC.FILL)
            setattr(self, name, view[:n] if n else view[:0])
        for name in IDLE_ZERO + ("counters", "tri_n", "pending", "dirty_tot"):
            getattr(self, name).zero_()
        self.vbm.fill_(-1)
        self.indexer.copy_(_t(pm.indexer))
        self.pos.copy_(_t(pm.pos))
        self.upload(pm)
        self.counters[_lib.C_N_OCCUPIED] = pm.n
        m = _lib.DifMap()
        m.nx = m.ny = m.nz = pm.grid
        m.bound_min = (ctypes.c_float * 3)(*[float(v) for v in pm.bound_min])
        m.voxel_size, m.prune_min_vox_obs, m.ignore_count_th, m.encoder_count_th, m.capacity = float(pm.voxel_size), 0, float(EC.IGNORE_TH), 600.0, cap
        for field, name in (("indexer", "indexer"), ("latent_vecs", "latent"), ("latent_vecs_pos", "pos"), ("voxel_obs_count", "obs"), ("dirty", "dirty"),
                            ("counters", "counters"), ("grid_bits", "grid_bits"), ("grid_tot", "grid_tot"), ("vbm", "vbm"), ("tri_start", "tri_start"),
                            ("tri_n", "tri_n"), ("pending_export", "pending")):
            setattr(m, field, _lib.ptr(getattr(self, name)))
        if dirty_tot:
            m.dirty_tot = _lib.ptr(self.dirty_tot)
        m.own_x_lo, m.own_x_hi, m.halo = (0, pm.grid, 0) if own is None else (own[0], own[1], 1)
        self.cmap = m
        b = _lib.DifExtractBuffers()
        b.max_voxels, b.cache_capacity, b.out_capacity = stated, self.cc, self.oc          # (a test may state a cache_capacity below the rows there are)
        for name in ("valid_blocks", "occ_slot", "low_sdf", "low_std", "cube_sdf", "cube_std", "refine_list", "tri_count", "tri_offset", "block_tmp",
                     "cache_tri", "cache_id", "cache_std", "cache_alive", "counters_out"):
            setattr(b, name, _lib.ptr(getattr(self, name)))
        if self.oc:
            b.out_tri, b.out_id, b.out_std = _lib.ptr(self.out_tri), _lib.ptr(self.out_id), _lib.ptr(self.out_std)
        if chunk:
            b.chunk_sum = _lib.ptr(self.chunk_sum)
        if chunk and status:
            b.mc_status = _lib.ptr(self.mc_status)
        if fold:
            b.fold_table = _lib.ptr(self.fold_table)
        self.cbuf = b

    def upload(self, pm):
        """latents, counts and dirty flags of `pm` (and the flags' block totals, which whoever sets flags keeps)"""
        self.latent.copy_(_t(pm.latent).reshape(-1))
        self.obs.copy_(_t(pm.obs))
        self.dirty.copy_(_t(pm.dirty))
        pad = np.zeros(self.dirty_tot.numel() * 256, dtype=np.int64)
        if self.has_tot:
            pad[:pm.capacity] = pm.dirty
        self.dirty_tot.copy_(_t(pad.reshape(-1, 256).sum(axis=1), np.int32))

    def prime(self, max_triangles=AMPLE, defer=False, stamp=1):
        for name in PER_CALL:
            getattr(self, name).view(torch.uint8).fill_(EC.FILL)
        self.cbuf.max_triangles, self.cbuf.defer_export, self.cbuf.stamp = int(max_triangles), int(defer), stamp
        return self.model.packed.weights_struct(DEV)

    def snapshot(self):
        torch.cuda.synchronize()
        for name in self.names:
            assert _guards_intact(self.guard[name]), f"the call wrote outside its {name}"
        r = SimpleNamespace(**{name: getattr(self, name).cpu().numpy() for name in self.names})
        c = r.counters_out
        r.K, r.B, r.VH, r.T, r.overflow, r.deferred = (int(c[k]) for k in (_lib.C_K, _lib.C_B, _lib.C_VH, _lib.C_T, _lib.C_OVERFLOW, _lib.C_DEFERRED))
        r.cache_T, r.kept, r.dead = int(c[_lib.C_CACHE_T]), int(c[_lib.C_CACHE_KEPT]), int(c[_lib.C_CACHE_DEAD])
        assert int(r.counters[_lib.C_OVERFLOW]) == 0 and int(c[_lib.C_STAMP]) == self.cbuf.stamp          # reported once, then cleared
        assert [int(r.counters[k]) for k in (_lib.C_K, _lib.C_B, _lib.C_VH, _lib.C_T, _lib.C_CACHE_T, _lib.C_CACHE_KEPT, _lib.C_CACHE_DEAD, _lib.C_DEFERRED)] == \
               [r.K, r.B, r.VH, r.T, r.cache_T, r.kept, r.dead, r.deferred]
        assert 0 <= r.K <= self.cbuf.max_voxels and 0 <= r.B <= self.cbuf.max_voxels and 0 <= r.VH <= r.B * self.R3 and 0 <= r.kept <= r.cache_T <= self.cbuf.cache_capacity
        r.latent = r.latent.reshape(-1, 29)
        r.cube_sdf, r.cube_std = r.cube_sdf.reshape(-1, self.R3), r.cube_std.reshape(-1, self.R3)
        r.log = (r.cache_tri.reshape(-1, 3, 3), r.cache_id, r.cache_std.reshape(-1, 3))
        return r

    def extract(self, fast=1, no_cache=0, **kw):
        w = self.prime(**kw)
        _lib.check(_lib.load().dif_extract(ctypes.byref(self.cmap), ctypes.byref(w), ctypes.byref(self.cbuf), self.r, fast, MAX_STD, no_cache, 1,
                                           _lib.stream_ptr()), "dif_extract")
        return self.snapshot()

    def export_pending(self):
        _lib.check(_lib.load().dif_export_pending(ctypes.byref(self.cmap), _lib.stream_ptr()), "dif_export_pending")
        torch.cuda.synchronize()

    def compact(self):
        """dif_mesh_cache_compact -> the live entries (tri, id, std)"""
        g = [_guarded(self.cc * k, dt) for k, dt in ((9, torch.float32), (1, torch.int64), (3, torch.float32))]
        gs, scratch = _guarded(4096, torch.int32)
        _lib.check(_lib.load().dif_mesh_cache_compact(ctypes.byref(self.cmap), ctypes.byref(self.cbuf), _lib.ptr(g[0][1]), _lib.ptr(g[1][1]), _lib.ptr(g[2][1]),
                                                      self.cc, _lib.ptr(scratch), _lib.stream_ptr()), "dif_mesh_cache_compact")
        torch.cuda.synchronize()
        assert all(_guards_intact(x[0]) for x in g) and _guards_intact(gs)
        n = int(self.counters[_lib.C_CACHE_LIVE])
        return g[0][1].cpu().numpy().reshape(-1, 3, 3)[:n], g[1][1].cpu().numpy()[:n], g[2][1].cpu().numpy().reshape(-1, 3)[:n]


def make(case, nets, scan="bounded", decode="fused_x6", chain="onepass", ws="shipped", **kw):
    """a Device whose buffers make extract_plan choose (scan, decode, chain) -> (Device, the arguments `fast` / `r` of its calls)"""
    x6 = decode == "fused_x6"
    dev = Device(case.pm.clone(), nets(ws, x6), r=kw.pop("r", 4), dirty_tot=scan in ("block", "bounded", "bounded5k"), chunk=chain != "count_scan_emit",
                 status=chain == "onepass", fold=decode in ("fused_x6", "fused_f32_fold"), **kw)
    assert case.pm.capacity == CAPACITY[scan]
    return dev, (0 if decode == "exact" else 1)


def case_of(scan, case1k, case8k):
    return case8k if scan in ("block", "generic8k") else case1k


# ---- the checks -------------------------------------------------------------------------------------------------------------------------
def check_idle(res, label, deferred_from=None):
    for name in IDLE_ZERO:
        assert not getattr(res, name).any(), f"{label}: {name} is not back at zero"          # (mc_status: the look-back words AND the eight ticket words)
    assert (res.vbm == -1).all(), f"{label}: vbm"
    if deferred_from is None:
        assert not res.dirty.any() and not res.dirty_tot.any(), f"{label}: dirty flags / block totals"
    else:
        assert np.array_equal(res.dirty, deferred_from.dirty) and res.dirty_tot.sum() == deferred_from.dirty.sum(), label


def check_lists(res, p, label):
    assert (res.K, res.B, res.deferred, res.overflow) == (p.K, p.B, p.deferred, p.overflow), (label, res.K, res.B, res.deferred, res.overflow)
    assert np.array_equal(res.valid_blocks[:p.K], p.valid_blocks) and np.array_equal(res.occ_slot[:p.B], p.occ_slot), label
    assert _filled(res.valid_blocks[p.K:]) and _filled(res.occ_slot[p.B:]), f"{label}: rows past K / B were written"


def check_plan_traces(res, dev, scan, decode, chain, label):
    """which plan ran, from what it wrote (module docstring)"""
    assert _filled(res.block_tmp) == (scan not in ("generic8k", "generic5k")), f"{label}: block_tmp"          # (the triangle scan of a few hundred voxels is one workgroup)
    assert _filled(res.low_sdf) and _filled(res.low_std), f"{label}: low_*"
    assert _filled(res.fold_table) == (decode in ("exact", "fused_f32")), f"{label}: fold_table"
    assert (res.VH == 0) == (decode == "exact"), label
    assert _filled(res.tri_offset) == (chain != "count_scan_emit"), f"{label}: tri_offset"
    if res.B:
        assert _filled(res.fold_table.reshape(-1, 256)[res.B:]) and _filled(res.cube_sdf[res.B:]) and _filled(res.cube_std[res.B:]), f"{label}: rows past B"
    if res.T:
        assert parks_corners(res, dev) == (chain != "onepass"), f"{label}: corners parked in the refine list"
    if chain == "onepass":
        assert _filled(res.refine_list[res.VH:]), f"{label}: the refine list behind VH"
    assert _filled(res.tri_count[res.K:]), f"{label}: tri_count past K"


def parks_corners(res, dev):
    """a word among the rows of the call's K voxels that is neither the fill nor a refine entry: a blended corner parked between the two passes"""
    w = res.refine_list[:res.K * dev.R3].astype(np.int64)
    return bool(((w != np.int64(np.array([EC.FILL] * 4, np.uint8).view(np.int32)[0])) & ((w < 0) | (w >= res.B * dev.R3))).any())


def check_refine_list(res, dev, label):
    """distinct entries in [0, B R^3), nothing behind VH, every sample that is not listed at or beyond the threshold"""
    lst = res.refine_list[:res.VH].astype(np.int64)
    assert res.VH > 0 and lst.min() >= 0 and lst.max() < res.B * dev.R3 and np.unique(lst).size == lst.size, f"{label}: the refine list"
    assert _filled(res.refine_list[res.VH:]), f"{label}: the refine list behind VH"
    listed = np.zeros(res.B * dev.R3, dtype=bool)
    listed[lst] = True
    assert (np.abs(res.cube_sdf[:res.B].reshape(-1)[~listed]) >= F32(0.05)).all(), f"{label}: an unlisted sample below the threshold"
    return listed.reshape(res.B, dev.R3)


def check_triangles(res, pm, p, dev, label):
    """the call's new triangles against the C marching cubes on the GPU's own cubes (the bar of test_gpu_map.py) -> T"""
    R = 2 * dev.r
    vbm = p.vbm if p.B else np.zeros(0, np.int32)
    wt, wi, ws = O.marching_cubes_interp(pm.indexer.reshape((pm.grid,) * 3), p.valid_blocks, vbm, res.cube_sdf[:p.B].reshape(-1, R, R, R),
                                         res.cube_std[:p.B].reshape(-1, R, R, R), int(4e6), [pm.grid] * 3, MAX_STD)
    assert res.T == wi.size, (label, res.T, wi.size)
    lo, hi = res.kept, res.cache_T
    assert hi - lo == res.T and np.array_equal(res.log[1][lo:hi], wi), label
    want = (wt * F32(pm.voxel_size)).astype(F32) + pm.bound_min
    if res.T:
        assert np.abs(res.log[0][lo:hi] - want).max() < 1e-5 and np.abs(res.log[2][lo:hi] - ws).max() < 1e-5, label
    return res.T


def same_mesh_state(a, b, label):
    """two runs left the same log, bookkeeping and counters, bit for bit"""
    assert (a.K, a.B, a.VH, a.T, a.cache_T, a.kept, a.dead, a.overflow) == (b.K, b.B, b.VH, b.T, b.cache_T, b.kept, b.dead, b.overflow), label
    n = a.cache_T
    for x, y in zip(a.log, b.log):
        assert np.array_equal(x[:n].view(np.uint8), y[:n].view(np.uint8)), f"{label}: the log"
    m = min(a.tri_n.size, b.tri_n.size)                                  # (the same map at capacity 1024 and 8192: the slots are the same)
    assert np.array_equal(a.cache_alive[:n], b.cache_alive[:n]) and np.array_equal(a.tri_n[:m], b.tri_n[:m]), f"{label}: alive / tri_n"
    assert not a.tri_n[m:].any() and not b.tri_n[m:].any(), f"{label}: tri_n"
    assert np.array_equal(a.tri_start[:m][a.tri_n[:m] > 0], b.tri_start[:m][a.tri_n[:m] > 0]), f"{label}: tri_start"
    assert np.array_equal(a.tri_count[:a.K], b.tri_count[:a.K]), f"{label}: tri_count"
    assert np.array_equal(a.valid_blocks[:a.K], b.valid_blocks[:a.K]) and np.array_equal(a.occ_slot[:a.B], b.occ_slot[:a.B]), label
    assert np.array_equal(bits(a.cube_sdf[:a.B]), bits(b.cube_sdf[:a.B])) and np.array_equal(bits(a.cube_std[:a.B]), bits(b.cube_std[:a.B])), f"{label}: cubes"


def two_frames(case, dev, fast, label, scan, decode, chain, full_checks):
    """frame 0 and the second frame on `dev` -> their snapshots"""
    out = []
    pm = case.pm.clone()
    for f in range(2):
        if f == 1:
            EC.second_frame(case, pm)
            dev.upload(pm)
        before = pm.clone()
        p = EC.prepare(pm)
        res = dev.extract(fast=fast)
        lab = f"{label} frame {f}"
        check_lists(res, p, lab)
        check_idle(res, lab)
        check_plan_traces(res, dev, scan, decode, chain, lab)
        if full_checks:
            if decode != "exact" and chain == "onepass":
                check_refine_list(res, dev, lab)
            assert check_triangles(res, before, p, dev, lab) > (100 if f == 0 else 10)
        out.append(res)
    return out


# ---- the tests --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("decode", DECODES)
def test_every_plan_two_frames(decode, nets, case1k, case8k):
    """4 dirty scans x 3 marching-cubes chains under one decode chain, two frames each (the second replaces batches and keeps stale ones): the
    lists against the restatement, the idle state, the guards, the traces of the plan; the scan choice changes nothing and the three
    marching-cubes chains leave the same log, bookkeeping and counters bit for bit; the triangles are the C marching cubes' on the GPU's cubes."""
    ref = None
    for scan in SCANS:
        for chain in CHAINS:
            case = case_of(scan, case1k, case8k)
            dev, fast = make(case, nets, scan, decode, chain)
            label = f"{scan}/{decode}/{chain}"
            frames = two_frames(case, dev, fast, label, scan, decode, chain, full_checks=ref is None)
            if ref is None:
                ref = frames
                again = (frames[0].tri_n > 0) & np.isin(np.arange(case.pm.capacity), case.dirty1)
                stale = again & (frames[1].tri_start < frames[1].kept) & (frames[1].tri_n == frames[0].tri_n)
                replaced = again & (frames[1].tri_start >= frames[1].kept)
                assert stale.any() and replaced.any() and frames[1].dead > 0, label
                print(f"  {label}: K {frames[0].K}/{frames[1].K}  B {frames[0].B}/{frames[1].B}  VH {frames[0].VH}/{frames[1].VH}  T {frames[0].T}/{frames[1].T}  "
                      f"replaced {int(replaced.sum())} stale {int(stale.sum())} dead {frames[1].dead}")
            for f in range(2):
                same_mesh_state(frames[f], ref[f], f"{label} frame {f} against {SCANS[0]}/{decode}/{CHAINS[0]}")


@pytest.mark.parametrize("r", (1, 2, 3))
def test_small_resolutions(r, nets, case1k, case8k):
    """r = 1, 2, 3 (R^3 = 8, 64, 216: lattices smaller than a tile, l^3 < 32 leaves the pair's second wave without a tile) on the fused chains and
    the exact one, under every dirty scan, the three marching-cubes chains against each other"""
    for decode in DECODES:
        ref = None
        for scan in ("bounded", "block", "generic1k", "generic8k"):
            case = case_of(scan, case1k, case8k)
            for chain in CHAINS:
                dev, fast = make(case, nets, scan, decode, chain, r=r)
                p = EC.prepare(case.pm.clone())
                res = dev.extract(fast=fast)
                label = f"r={r}/{scan}/{decode}/{chain}"
                check_lists(res, p, label)
                check_idle(res, label)
                if decode != "exact" and chain == "onepass" and res.VH:
                    check_refine_list(res, dev, label)
                if ref is None:
                    ref = res
                    check_triangles(res, case.pm, p, dev, label)
                same_mesh_state(res, ref, label)


def test_two_level_r8(nets, case1k, case8k):
    """r = 8: the lattice is too large for the fused kernel (TwoLevel: low lattice, k_upsample_mark, refine), marching cubes by CountEmit and
    CountScanEmit (extract_plan refuses OnePass beyond 64 cells).  Frame A: dirty voxels that are not confident themselves — they pull their
    neighbours into the batch and park no corners, so the whole refine list is visible: it equals {|sv| < 0.05f} of the restated upsample of the
    GPU's own low values, and every unlisted sample is -sv / dv bit for bit.  Frame B: the planted frame under the four dirty scans, the two chains
    and the scans against each other."""
    model = nets("shipped", True)
    pm = case1k.pm.clone()
    pm.dirty[:] = 0
    quiet = np.concatenate([case1k.dirty0[np.isin(case1k.dirty0, np.nonzero(pm.pos // 256 >= 4)[0])][:12], [pm.indexer[EC._lin(EC.AT_TH)]]])
    pm.obs[quiet] = EC.IGNORE_TH
    pm.dirty[quiet] = 1
    for chain in ("count_emit", "count_scan_emit"):
        dev = Device(pm.clone(), model, r=8, chunk=chain == "count_emit", status=True)
        p = EC.prepare(pm.clone())
        res = dev.extract()
        label = f"two-level r=8 {chain}, unconfident dirty voxels"
        check_lists(res, p, label)
        check_idle(res, label)
        assert res.T == 0 and res.B >= 20 and not _filled(res.low_sdf[:res.B * 512]) and _filled(res.low_sdf[res.B * 512:]) and _filled(res.low_std[res.B * 512:])
        listed = check_refine_list(res, dev, label)
        sv = EC.upsample2(res.low_sdf[:res.B * 512].reshape(-1, 8, 8, 8), 16).reshape(res.B, -1)
        dv = EC.upsample2(res.low_std[:res.B * 512].reshape(-1, 8, 8, 8), 16).reshape(res.B, -1)
        assert np.array_equal(listed, np.abs(sv) < F32(0.05)), f"{label}: the listed set"
        assert np.array_equal(bits(res.cube_sdf[:res.B][~listed]), bits(-sv[~listed])) and np.array_equal(bits(res.cube_std[:res.B][~listed]), bits(dv[~listed])), label
        print(f"  {label}: B {res.B} VH {res.VH}")
    ref = None
    for scan in SCANS:
        case = case_of(scan, case1k, case8k)
        for chain in ("count_emit", "count_scan_emit"):
            dev = Device(case.pm.clone(), model, r=8, dirty_tot=scan in ("block", "bounded"), chunk=chain == "count_emit", status=True, cache_capacity=16384)
            p = EC.prepare(case.pm.clone())
            res = dev.extract()
            label = f"two-level r=8 {scan}/{chain}"
            check_lists(res, p, label)
            check_idle(res, label)
            assert not _filled(res.low_sdf[:res.B * 512]) and _filled(res.tri_offset) == (chain == "count_emit")
            assert _filled(res.block_tmp) == (scan != "generic8k"), label
            if ref is None:
                ref = res
                assert check_triangles(res, case.pm, p, dev, label) > 400
            same_mesh_state(res, ref, label)


@pytest.mark.parametrize("scan", ("bounded", "generic1k", "block", "streams"))
def test_grid64_two_total_blocks(scan, nets):
    """A 64^3 grid: 8,192 bitmap words in 32 grid_tot blocks of 256, so the batch scan is k_scan_pass2 over the totals the MARKERS kept — a bit
    counted twice, or into the wrong block, moves B and every later block's rows.  Dirty voxels at lin 8191 and 8192 mark neighbours in each
    other's block; (2,0,0) and (2,0,1) are each other's neighbours and sit on the y = 0 border, where a clamped neighbour is the voxel itself.
    bounded / generic1k: the flat mark_confident_nbhd (DirtyFunctor::emit); block: its copy hoisted into dirty_scan_body (k_dirty_scan at
    capacity 8192); streams: the same through dif_extract_streams (k_dirty_scan_batch, k_scan_pass2_batch), two maps with different batches."""
    case = EC.grid64(1024 if scan in ("bounded", "generic1k") else 8192)
    p = EC.prepare(case.pm.clone())
    dirty_lin = case.pm.pos[case.dirty0]
    assert set((p.batch // 8192).tolist()) >= {0, 1} and sum(IC.neighbours7([v], 64).size for v in dirty_lin) > IC.neighbours7(dirty_lin, 64).size
    if scan != "streams":
        for chain in CHAINS:
            dev, fast = make(case, nets, scan, "fused_x6", chain, r=2)
            res = dev.extract()
            assert res.grid_bits.size == 8192
            check_lists(res, p, f"grid64 {scan}/{chain}")
            check_idle(res, f"grid64 {scan}/{chain}")
        return
    model = nets("shipped", True)
    other = case.pm.clone()
    other.dirty[other.indexer[EC._lin((2, 0, 0), 64)]] = 0
    q = EC.prepare(other.clone())
    assert 0 < q.B < p.B and set((q.batch // 8192).tolist()) >= {0, 1}
    devs = [Device(case.pm.clone(), model, r=2), Device(other.clone(), model, r=2)]
    frames = (_lib.DifStreamFrame * 2)()
    for j, d in enumerate(devs):
        w = d.prime()
        frames[j].map, frames[j].buf = ctypes.pointer(d.cmap), ctypes.pointer(d.cbuf)
    _lib.check(_lib.load().dif_extract_streams(frames, 2, ctypes.byref(w), 2, MAX_STD, 1, _lib.stream_ptr()), "dif_extract_streams")
    for j, (d, want) in enumerate(zip(devs, (p, q))):
        res = d.snapshot()
        check_lists(res, want, f"grid64 streams, map {j}")
        check_idle(res, f"grid64 streams, map {j}")


def test_tiled_and_no_cache(nets, case1k):
    """own_x = [4, 11): dirty halo voxels are not listed and their neighbourhoods are in the batch (k_mark_halo_dirty + the Generic scan);
    no_cache lists every slot; both against the restatement, idle afterwards"""
    for chain in CHAINS:
        dev, fast = make(case1k, nets, "bounded", "fused_x6", chain, own=(4, 11))
        p = EC.prepare(case1k.pm.clone(), own=(4, 11))
        res = dev.extract()
        assert 0 < p.K < case1k.dirty0.size
        check_lists(res, p, f"tiled {chain}")
        check_idle(res, f"tiled {chain}")
        check_triangles(res, case1k.pm, p, dev, f"tiled {chain}")
        dev, fast = make(case1k, nets, "bounded", "fused_x6", chain, cache_capacity=32768)
        p = EC.prepare(case1k.pm.clone(), no_cache=True)
        res = dev.extract(no_cache=1)
        check_lists(res, p, f"no_cache {chain}")
        check_idle(res, f"no_cache {chain}")
        assert res.K == case1k.pm.n and res.kept == 0 and check_triangles(res, case1k.pm, p, dev, f"no_cache {chain}") > 1000


@pytest.mark.parametrize("decode", ("fused_x6", "fused_f32", "fused_f32_fold"))
def test_fused_cubes_do_not_depend_on_where_a_voxel_runs(decode, nets):
    """1,300 voxels, a third of them clones of three latents, no_cache: B > 4 pairs x every CU, so k_decode_voxels takes a SECOND ROUND (no cap
    of max_voxels reaches one on a smaller batch: the launch has a workgroup per four rows).  Voxels with the same latent have bit-identical
    cubes and the same refine sub-list whatever their batch index, wave pair or round; a dirty-subset extract of the same map gives every
    voxel it shares with the no_cache extract the same bits."""
    case = EC.planted(8192, n_extra=1200)
    pm = case.pm
    dev, fast = make(case, nets, "generic8k", decode, "onepass", cache_capacity=65536)
    res = dev.extract(no_cache=1)
    p = EC.prepare(pm.clone(), no_cache=True)
    check_lists(res, p, decode)
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    n_pairs = 4 * min((dev.mv + 3) // 4, cus)
    assert res.B > n_pairs, f"one round only: B {res.B}, {n_pairs} pairs"
    listed = check_refine_list(res, dev, decode)
    uniq, first, inv = np.unique(pm.latent[res.occ_slot[:res.B]], axis=0, return_index=True, return_inverse=True)
    inv = inv.reshape(-1)
    groups = np.bincount(inv)
    assert (groups > 50).sum() == 3 and np.unique(np.nonzero(groups[inv] > 50)[0] // n_pairs).size == 2          # clones in both rounds
    assert np.array_equal(bits(res.cube_sdf[:res.B]), bits(res.cube_sdf[first][inv])) and np.array_equal(bits(res.cube_std[:res.B]), bits(res.cube_std[first][inv]))
    assert np.array_equal(listed, listed[first][inv]), f"{decode}: clones with different refine sub-lists"
    sub, _ = make(case, nets, "generic8k", decode, "onepass", cache_capacity=65536)
    part = sub.extract()
    shared, ia, ib = np.intersect1d(res.occ_slot[:res.B], part.occ_slot[:part.B], return_indices=True)
    assert shared.size == part.B > 100
    assert np.array_equal(bits(res.cube_sdf[ia]), bits(part.cube_sdf[ib])) and np.array_equal(bits(res.cube_std[ia]), bits(part.cube_std[ib])), decode
    print(f"  {decode}: B {res.B} in {-(-res.B // n_pairs)} rounds of {n_pairs} pairs, VH {res.VH}, clone groups {sorted(groups[groups > 50].tolist())}")


def test_zero_crossing_weights(nets, case1k):
    """the planted frame under a hostile weight set whose surface crosses the map ("+zc"): lists, idle state, the chains against each other"""
    ref = None
    for chain in CHAINS:
        dev, fast = make(case1k, nets, "bounded", "fused_x6", chain, ws="hostile_a+zc", cache_capacity=65536)
        p = EC.prepare(case1k.pm.clone())
        res = dev.extract()
        check_lists(res, p, chain)
        check_idle(res, chain)
        if ref is None:
            ref = res
            check_refine_list(res, dev, chain)
            check_triangles(res, case1k.pm, p, dev, chain)
        same_mesh_state(res, ref, f"hostile_a+zc {chain}")


# ---- limits -----------------------------------------------------------------------------------------------------------------------------
def _new_rows(res):
    """the (untruncated) triangles a call appended"""
    assert res.T == res.cache_T - res.kept
    return tuple(x[res.kept:res.cache_T].copy() for x in res.log)


def _check_log(res, log, r, dev, label):
    """the log and its bookkeeping against the restatement; rows behind the STATED capacity (the buffers are longer) and rows no call appended
    keep the fill byte"""
    assert (res.cache_T, res.kept, res.dead, res.T, res.overflow) == (log.T, log.kept, log.dead, r.T, r.overflow), (label, res.cache_T, res.kept, res.dead, res.T, res.overflow)
    for got, want in zip(res.log, (log.tri, log.id, log.std)):
        assert np.array_equal(got[:log.cc][log.written].view(np.uint8), want[log.written].view(np.uint8)), f"{label}: log rows"
        assert _filled(got[:log.cc][~log.written]) and _filled(got[log.cc:]), f"{label}: a log row outside what the calls appended was written"
    assert np.array_equal(res.cache_alive[:log.T], log.alive[:log.T]), f"{label}: alive"
    assert _filled(res.cache_alive[:log.cc][~log.written]) and _filled(res.cache_alive[log.cc:]), f"{label}: alive outside the appended rows"
    assert np.array_equal(res.tri_n, log.tri_n) and np.array_equal(res.tri_start[log.tri_n > 0], log.tri_start[log.tri_n > 0]), f"{label}: tri_start / tri_n"


LOG_ROWS = 32768          # rows of the log buffers in the limit tests; the capacity a call STATES is the case's


@pytest.mark.parametrize("chain", CHAINS)
def test_triangle_limits(chain, nets, case1k):
    """max_triangles = T, T - 1, a voxel's first triangle, one past it, 1; cache_capacity = kept + T, one less, mid-voxel, kept + 1 (code 5);
    out_capacity 7, copied by the last kernel, by the one-pass kernel, or deferred and carried out by dif_export_pending — on the first frame
    and on the second (batches to replace).  The log, alive, tri_start / tri_n, the counters, the caller's copy and the pending record equal
    the restatement (the reference's rule: a voxel cut off whole keeps its old batch); dif_mesh_cache_compact returns the restated live
    entries; a no_cache extract that follows on the same map, with the whole log at its disposal, gives the mesh of an unlimited run."""
    pm0 = case1k.pm.clone()
    pm1 = case1k.pm.clone()
    pm1.dirty[:] = 0
    EC.second_frame(case1k, pm1)
    free, _ = make(case1k, nets, "bounded", "fused_x6", chain, cache_capacity=LOG_ROWS)
    rows0 = _new_rows(free.extract())
    nc0 = _new_rows(free.extract(no_cache=1))
    free.upload(pm1)
    rows1 = _new_rows(free.extract())
    nc1 = _new_rows(free.extract(no_cache=1))
    T0 = rows0[1].size
    assert nc1[1].size > 1000 and not np.array_equal(nc0[1], nc1[1])
    n_cases = whole = 0
    for frame, rows, nc in ((0, rows0, nc0), (1, rows1, nc1)):
        kept = 0 if frame == 0 else T0
        for i, (mt, cc) in enumerate(EC.limit_cases(T0, kept, rows[1].size, EC.voxel_runs(rows[1]))):
            defer = i % 3 == 2
            cap = min(cc, 4096)
            dev, _ = make(case1k, nets, "bounded", "fused_x6", chain, cache_capacity=LOG_ROWS, out_capacity=7)
            dev.cbuf.cache_capacity = cap
            log = EC.Log(pm0.capacity, cap)
            label = f"{chain} frame {frame} max_triangles {mt} cache_capacity {cap}{' deferred' if defer else ''}"
            if frame == 1:
                first = dev.extract()
                EC.log_update(log, pm0.indexer, *rows0, AMPLE, out_capacity=7)
                _check_log(first, log, SimpleNamespace(T=T0, overflow=0), dev, label + " (frame 0)")
                dev.upload(pm1)
            prev_n = log.tri_n.copy()
            r = EC.log_update(log, pm0.indexer, *rows, mt, out_capacity=7, seq=5)
            res = dev.extract(max_triangles=mt, defer=defer, stamp=5)
            check_idle(res, label)
            _check_log(res, log, r, dev, label)
            n_out = r.out[1].size
            if defer:
                assert _filled(res.out_tri) and _filled(res.out_id) and _filled(res.out_std), f"{label}: a deferred copy was written by the extract"
                assert tuple(int(x) for x in res.pending[:4]) == r.pending, (label, res.pending[:4], r.pending)
                dev.export_pending()
                res = dev.snapshot()
                assert int(res.pending[0]) == 0, label
            else:
                assert not res.pending.any(), label
            assert np.array_equal(bits(res.out_tri[:n_out * 9]), bits(r.out[0].reshape(-1))) and np.array_equal(res.out_id[:n_out], r.out[1]), f"{label}: out rows"
            assert np.array_equal(bits(res.out_std[:n_out * 3]), bits(r.out[2].reshape(-1))), f"{label}: out_std"
            assert _filled(res.out_tri[n_out * 9:]) and _filled(res.out_id[n_out:]) and _filled(res.out_std[n_out * 3:]), f"{label}: rows past the copy"
            live = dev.compact()
            for got, want in zip(live, log.live()):
                assert got.shape == want.shape and np.array_equal(got.view(np.uint8), want.view(np.uint8)), f"{label}: dif_mesh_cache_compact"
            whole += int((prev_n[pm0.indexer[r.whole_cut]] > 0).sum())
            n_cases += 1
            dev.cbuf.cache_capacity = LOG_ROWS
            after = dev.extract(no_cache=1)
            check_idle(after, label + ", then no_cache")
            for got, want in zip(_new_rows(after), nc):
                assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), f"{label}: the no_cache mesh afterwards"
    assert n_cases == 18 and whole > 0, f"{chain}: no limit case cut off a whole voxel that held a batch"
    print(f"  {chain}: {n_cases} limit cases, T {T0} / {rows1[1].size}, {whole} voxels cut off whole that held a batch")


def _sparse(case):
    """the planted map with only its isolated voxels dirty (corners, edges, faces, the lonely one) and one of them below the threshold: the
    batch is SMALLER than the dirty list, so max_voxels = K - 1 cuts the list (code 2) and not the batch (code 3, which the scan behind it
    would write over the 2)"""
    c = SimpleNamespace(pm=case.pm.clone())
    pm = c.pm
    pm.dirty[:] = 0
    slots = pm.indexer[[EC._lin(v) for v in EC.CORNERS + EC.EDGES + EC.FACES + [EC.LONELY]]]
    pm.dirty[slots] = 1
    pm.obs[slots[-1]] = EC.IGNORE_TH
    return c


def test_max_voxels_limits(nets, case1k, case8k):
    """max_voxels = K - 1 on the Generic and Bounded scans: code 2 on a dirty set whose batch is smaller than it, the first K - 1 dirty voxels
    listed and marked, every flag consumed; on the planted frame (B > K) the batch is cut too and the code left is 3.  max_voxels = B - 1:
    code 3.  BlockTotals at min(7 K, n) == max_voxels: it runs; one row short of it: it defers — NOTHING has changed but K = B = T = 0 and
    DIF_C_DEFERRED.  All on the three marching-cubes chains, which agree."""
    full = EC.prepare(case1k.pm.clone())
    K, B, n = full.K, full.B, case1k.pm.n
    need = min(7 * K, n)
    sparse1k, sparse8k = _sparse(case1k), _sparse(case8k)
    Ks = EC.prepare(sparse1k.pm.clone()).K
    rows = [("generic1k", sparse1k, Ks - 1, 2), ("bounded", sparse1k, Ks - 1, 2), ("generic8k", sparse8k, Ks - 1, 2),
            ("generic1k", case1k, K - 1, 3), ("bounded", case1k, K - 1, 3), ("bounded", case1k, B - 1, 3), ("generic8k", case8k, B - 1, 3),
            ("block", case8k, need, 0), ("block", case8k, need - 1, -1)]
    unlimited = {}
    for scan, case, mv, code in rows:
        if id(case) not in unlimited:                       # the mesh of a no_cache extract of this map that no limit touched
            free, _ = make(case, nets, scan, "fused_x6", "onepass", cache_capacity=LOG_ROWS)
            unlimited[id(case)] = _new_rows(free.extract(no_cache=1))
        ref = None
        for chain in CHAINS:
            # (the buffers have a row per voxel, for the no_cache extract that follows; the call STATES max_voxels = mv, and every row behind that
            # must keep the fill byte)
            dev, _ = make(case, nets, scan, "fused_x6", chain, max_voxels=mv, rows=case.pm.n, cache_capacity=LOG_ROWS)
            before = {name: getattr(dev, name).cpu().numpy().copy() for name in ("tri_n", "cache_alive")}
            p = EC.prepare(case.pm.clone(), max_voxels=mv, block_totals=scan == "block")
            res = dev.extract()
            label = f"{scan}/{chain} max_voxels {mv}"
            check_lists(res, p, label)
            if code >= 0:
                assert p.overflow == code and p.deferred == 0 and p.K == min(p.K_total, mv) and p.B == min(p.B_total, mv), (label, p.overflow)
                assert code != 2 or (p.K_total == mv + 1 and p.B_total <= mv), label
                check_idle(res, label)
                check_triangles(res, case.pm, p, dev, label)
            else:
                assert p.deferred == need and res.deferred == need and (res.K, res.B, res.VH, res.T, res.cache_T) == (0, 0, 0, 0, 0), label
                check_idle(res, label, deferred_from=case.pm)
                assert np.array_equal(res.tri_n, before["tri_n"]) and np.array_equal(res.cache_alive, before["cache_alive"]), label
                for name in ("cube_sdf", "cube_std", "refine_list", "fold_table", "valid_blocks", "occ_slot", "cache_tri", "cache_id", "cache_std", "tri_count"):
                    assert _filled(getattr(res, name)), f"{label}: a deferred extract wrote {name}"
            if ref is None:
                ref = res
            same_mesh_state(res, ref, label)
            for name in ("valid_blocks", "occ_slot", "tri_count", "cube_sdf", "cube_std"):
                assert _filled(getattr(res, name)[mv:]), f"{label}: {name} behind the stated max_voxels"
            assert _filled(res.fold_table.reshape(-1, 256)[mv:]) and _filled(res.refine_list[mv * dev.R3:]), f"{label}: rows behind the stated max_voxels"
            # the log of the cut call against the restatement (fed the call's own new rows: it is their bookkeeping that is compared), the
            # compaction, and a no_cache extract with a row per voxel afterwards: the mesh of a run that met no limit
            log = EC.Log(case.pm.capacity, dev.cc)
            r = EC.log_update(log, case.pm.indexer, *_new_rows(res), AMPLE, out_capacity=dev.oc)
            _check_log(res, log, SimpleNamespace(T=r.T, overflow=max(code, 0)), dev, label)
            for got, want in zip(dev.compact(), log.live()):
                assert got.shape == want.shape and np.array_equal(got.view(np.uint8), want.view(np.uint8)), f"{label}: dif_mesh_cache_compact"
            dev.cbuf.max_voxels = dev.mv
            after = dev.extract(no_cache=1)
            check_idle(after, label + ", then no_cache")
            assert after.K == case.pm.n and after.overflow == 0, label
            for got, want in zip(_new_rows(after), unlimited[id(case)]):
                assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), f"{label}: the no_cache mesh afterwards"


def test_bounded_totals_beyond_one_workgroup(nets):
    """Capacity 5000 (above 4096, no multiple of 256): BoundedTotals goes through k_scan_pass2_fixed, a workgroup per 256 slots over dirty_tot —
    the planted dirty slots 255, 256, 257 lie either side of its first block edge.  Two frames on the three marching-cubes chains, against the
    restatement and against the Generic scan of the same map (two launches: block_tmp is written)."""
    case = EC.planted(5000)
    ref = None
    for scan in ("bounded5k", "generic5k"):
        for chain in CHAINS:
            dev, fast = make(case, nets, scan, "fused_x6", chain)
            assert dev.dirty_tot.numel() == 20
            label = f"{scan}/{chain}"
            frames = two_frames(case, dev, fast, label, scan, "fused_x6", chain, full_checks=ref is None)
            if ref is None:
                ref = frames
            for f in range(2):
                same_mesh_state(frames[f], ref[f], f"{label} frame {f}")


def test_one_pass_ticket_mode(nets, case1k, mc_grid_cap):
    """dif_test_mc_grid_cap(2): two workgroups for ~15 groups of four voxels, so the one-pass kernel hands groups out through its ticket words;
    the same log as the uncapped launch, at a limit too, and the ticket words back at zero"""
    for mt in (AMPLE, 40):
        ref, _ = make(case1k, nets, "bounded", "fused_x6", "onepass")
        want = ref.extract(max_triangles=mt)
        mc_grid_cap(2)
        dev, _ = make(case1k, nets, "bounded", "fused_x6", "onepass")
        got = dev.extract(max_triangles=mt)
        mc_grid_cap(0)
        check_idle(got, f"ticket mode, max_triangles {mt}")
        assert got.K > 8 and got.T > 100
        same_mesh_state(got, want, f"ticket mode, max_triangles {mt}")


# ---- several maps in one launch -----------------------------------------------------------------------------------------------------------
def _stream_maps(case8k):
    """ordinary; an empty dirty set; one that defers (1,300 voxels, min(7 K, n) above the shared max_voxels); one that truncates"""
    empty = SimpleNamespace(pm=case8k.pm.clone())
    empty.pm.dirty[:] = 0
    big = EC.planted(8192, n_extra=1000)
    other = EC.planted(8192, seed=9)
    return dict(ordinary=(case8k, AMPLE), empty=(empty, AMPLE), defers=(big, AMPLE), truncates=(other, 50))


@pytest.mark.parametrize("names", (("ordinary", "empty"), ("ordinary", "empty", "truncates"), ("truncates", "defers", "ordinary"), ("defers", "empty", "ordinary")))
def test_streams(names, nets, case8k):
    """dif_extract_streams with S = 2 and 3: every map's buffers, log and counters equal, bit for bit, what dif_extract leaves on that map alone
    (refine-list ENTRIES as a set: their order inside the list depends on which workgroup reserved first); every refine list is well formed."""
    maps = _stream_maps(case8k)
    mv = 400
    model = nets("shipped", True)
    solo, devs = [], []
    for name in names:
        case, mt = maps[name]
        d = Device(case.pm.clone(), model, max_voxels=mv)
        solo.append(d.extract(max_triangles=mt))
        devs.append(Device(case.pm.clone(), model, max_voxels=mv))
    frames = (_lib.DifStreamFrame * len(names))()
    w = None
    for j, (name, d) in enumerate(zip(names, devs)):
        w = d.prime(max_triangles=maps[name][1])
        frames[j].map, frames[j].buf = ctypes.pointer(d.cmap), ctypes.pointer(d.cbuf)
    _lib.check(_lib.load().dif_extract_streams(frames, len(names), ctypes.byref(w), 4, MAX_STD, 1, _lib.stream_ptr()), "dif_extract_streams")
    got = [d.snapshot() for d in devs]
    ran = [s.B for s in solo if s.K]
    assert len(set(ran)) == len(ran) >= 1, ran          # the maps that run decode batches of different sizes
    for name, d, a, b in zip(names, devs, got, solo):
        label = f"{name} in {names}"
        case = maps[name][0]
        if name == "defers":
            assert a.deferred == min(7 * int(case.pm.dirty.sum()), case.pm.n) > mv and a.K == 0
            check_idle(a, label, deferred_from=case.pm)
        else:
            check_idle(a, label)
            assert a.deferred == 0 and (a.K == 0) == (name == "empty") and (a.T > maps[name][1]) == (name == "truncates"), label
        same_mesh_state(a, b, label)
        if a.VH:
            check_refine_list(a, d, label)
            assert np.array_equal(np.sort(a.refine_list[:a.VH]), np.sort(b.refine_list[:b.VH])), f"{label}: refine entries"
        for buf in ("fold_table", "tri_count", "out_tri", "out_id", "out_std", "counters_out", "pending", "cache_alive"):
            x, y = getattr(a, buf), getattr(b, buf)
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), f"{label}: {buf}"
