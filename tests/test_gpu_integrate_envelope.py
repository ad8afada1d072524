"""The integrate chain (dif_integrate / dif_integrate_frame: csrc/kernels_integrate.hip.h) stage by stage: its integer state bit for bit
against a NumPy restatement, its per-voxel sums exactly, its fusion bit for bit, and the fused value against a float64 reference.

The restatement, the cases and THE BAR are in tests/integrate_cases.py (pinned against OracleMap.integrate_keyframe by
tests/test_ref64_cpu.py).  The calls go through ctypes on planted maps whose every written buffer sits between guard words; the workspace
(pt_lin, the pair list, the run records and their chain links) is read through dif_test_integrate_views.

WHAT IS REACHED WHERE
  k_voxel_count / k_unproject_voxel_count   pt_lin, frame_count          every test (faces: the voxel faces and the grid's; frame: both point sources)
  k_prune_mark                              mask, candidates, totals     runs (count == prune_min), corners (clamped neighbours), alloc64 (block totals)
  the allocation scan                       indexer, latent_vecs_pos     k_scan_single (16^3), k_scan_pass2 (alloc64), the capacity clamp (overflow)
  k_focus_gather                            the pair list                threshold (obs == th), chain (the loose tail), frame (tile and flat walk)
  k_encode<X6>                              the run records              _check_sums: every record and every slot's sum, exactly
  k_fuse                                    latents, counts, flags       _check_fusion: bit for bit, the directory's overflow chain included (chain)
"""
import ctypes

import numpy as np
import pytest
import torch

from di_fusion_amd import _lib
from di_fusion_amd.network import utility as net_util
from tests import integrate_cases as IC
from tests import mlp_cases as C
from tests import optim_cases as OC
from tests.test_gpu_optim_envelope import DEV, GUARD, _guarded, _guards_intact, bits  # noqa: F401

pytestmark = pytest.mark.gpu
PIPES = ("bf16x6", "f32")
F32 = np.float32
REC_POS = np.array([((f >> 2) & 1) * 16 + (f & 3) + 4 * (f >> 3) for f in range(29)])      # where feature f sits in a run record (k_fuse)
REC_COUNT_POS = 29


@pytest.fixture(scope="module")
def nets():
    cache = {}

    def get(ws, pipe):
        if (ws, pipe) not in cache:
            cache[ws, pipe] = net_util.networks_from_arrays(C.weight_set(ws), x6=(pipe == "bf16x6"))
        return cache[ws, pipe]
    return get


def _kernel(pipe):
    return "k_encode<true> / encoder_tile_x6" if pipe == "bf16x6" else "k_encode<false> / encoder_tile"


def _t(a, dt=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(DEV)


class Device:
    """An IMap on the GPU (every buffer a call writes is guarded) and calls of dif_integrate / dif_integrate_frame on it."""

    NAMES = ("latent", "obs", "dirty", "upd_list", "rec_dir", "indexer", "pos", "frame_count", "grid_bits", "grid_tot", "alloc_bits", "alloc_tot",
             "counters", "dirty_tot")

    def __init__(self, pm: IC.IMap, model, prune_min: int, th: float = IC.TH, own=None, halo: int = 0, list_cap: int = 0):
        """own = (x_lo, x_hi), halo, list_cap: a slab of a spatially tiled map with its boundary change lists (tests/test_gpu_tiling_envelope.py)"""
        self.pm, self.model, cap, G = pm, model, pm.capacity, pm.grid ** 3
        self.words, self.n_blk = (G + 31) // 32, (cap + 255) // 256
        shapes = dict(latent=(cap * 29, torch.float32), obs=(cap, torch.float32), dirty=(cap, torch.uint8), upd_list=(cap, torch.int32),
                      rec_dir=(cap * 16, torch.int32), indexer=(G, torch.int64), pos=(cap, torch.int64), frame_count=(G, torch.int32),
                      grid_bits=(self.words, torch.int32), grid_tot=(1024, torch.int32), alloc_bits=(self.words, torch.int32),
                      alloc_tot=(1024, torch.int32), counters=(_lib.C_COUNT, torch.int32), dirty_tot=(self.n_blk, torch.int32))
        if list_cap > 0:
            shapes["halo_list"] = (2 * list_cap, torch.int32)
            self.NAMES = Device.NAMES + ("halo_list",)
        self.guard = {}
        for name, (n, dt) in shapes.items():
            self.guard[name], view = _guarded(n, dt)
            view.zero_()
            setattr(self, name, view)
        self.latent.copy_(_t(pm.latent).reshape(-1))
        self.obs.copy_(_t(pm.obs))
        self.indexer.copy_(_t(pm.indexer))
        self.pos.copy_(_t(pm.pos))
        self.dirty.copy_(_t(pm.dirty))                      # (with its block totals: the planted maps of the tiling tests carry dirty flags)
        pad = np.zeros(self.n_blk * 256, dtype=np.int32)
        pad[:cap] = pm.dirty
        self.dirty_tot.copy_(_t(pad.reshape(-1, 256).sum(axis=1), np.int32))
        self.upd_list.fill_(-7)
        self.counters[_lib.C_N_OCCUPIED] = pm.n
        m = _lib.DifMap()
        m.nx = m.ny = m.nz = pm.grid
        m.bound_min = (ctypes.c_float * 3)(*[float(v) for v in pm.bound_min])
        m.voxel_size = float(pm.voxel_size)
        m.prune_min_vox_obs, m.ignore_count_th, m.encoder_count_th, m.capacity = int(prune_min), 16.0, float(th), cap
        for field, name in (("indexer", "indexer"), ("latent_vecs", "latent"), ("latent_vecs_pos", "pos"), ("voxel_obs_count", "obs"), ("dirty", "dirty"),
                            ("counters", "counters"), ("frame_count", "frame_count"), ("grid_bits", "grid_bits"), ("grid_tot", "grid_tot"),
                            ("rec_dir", "rec_dir"), ("upd_list", "upd_list"), ("dirty_tot", "dirty_tot"), ("alloc_bits", "alloc_bits"), ("alloc_tot", "alloc_tot")):
            setattr(m, field, _lib.ptr(getattr(self, name)))
        m.own_x_lo, m.own_x_hi, m.halo, m.frame_seq = 0, pm.grid, 0, 0          # one map, no halo lists, no pending export, one queue
        if own is not None:
            m.own_x_lo, m.own_x_hi, m.halo = int(own[0]), int(own[1]), int(halo)
        if list_cap > 0:
            self.halo_list.fill_(-9)
            m.halo_list, m.halo_list_cap = _lib.ptr(self.halo_list), int(list_cap)
        self.cmap = m

    def state(self):
        """latents (capacity,29) and counts as NumPy arrays: what the next call starts from"""
        return self.latent.cpu().numpy().reshape(-1, 29).copy(), self.obs.cpu().numpy().copy()

    def call(self, xyz=None, normal=None, frame=None, with_xyz=True):
        """dif_integrate on (xyz, normal), or dif_integrate_frame on a frame case (its world points written out, or not kept: with_xyz)
        -> a namespace of everything the call left behind, as NumPy arrays"""
        lib = _lib.load()
        N = int(xyz.shape[0]) if frame is None else frame.img[0] * frame.img[1]
        nb = int(lib.dif_integrate_workspace_bytes(N))
        assert nb > 0
        g_ws, ws = _guarded(nb, torch.uint8)
        ws.fill_(0xA5)                                     # stale workspace contents must not matter
        g_mask, mask = _guarded(N, torch.uint8)
        mask.fill_(0x5A)
        w = self.model.packed.weights_struct(DEV)
        extra = [("workspace", g_ws), ("mask", g_mask)]
        r = type("Result", (), {})()
        if frame is None:
            d_xyz, d_nrm = _t(xyz, F32), _t(normal, F32)
            _lib.check(lib.dif_integrate(ctypes.byref(self.cmap), ctypes.byref(w), _lib.ptr(d_xyz), _lib.ptr(d_nrm), N, _lib.ptr(mask), _lib.ptr(ws), nb,
                                         _lib.stream_ptr()), "dif_integrate")
        else:
            H, W = frame.img
            depth, ncam = _t(frame.depth, F32), _t(frame.normal_cam, F32)
            desc = _t(np.frombuffer(IC.frame_descriptor(depth.data_ptr(), ncam.data_ptr(), frame.pose), dtype=np.uint8).copy())
            g_x, d_xyz = _guarded(N * 3, torch.float32)
            g_n, d_nrm = _guarded(N * 3, torch.float32)
            extra += [("xyz_world", g_x), ("normal_world", g_n)]
            fx, fy, cx, cy = frame.intr
            _lib.check(lib.dif_integrate_frame(ctypes.byref(self.cmap), ctypes.byref(w), _lib.ptr(desc), H, W, fx, fy, cx, cy, _lib.ptr(d_xyz) if with_xyz else None,
                                               _lib.ptr(d_nrm) if with_xyz else None, _lib.ptr(mask), _lib.ptr(ws), nb, _lib.stream_ptr()), "dif_integrate_frame")
            torch.cuda.synchronize()
            r.xyz_world, r.normal_world = d_xyz.cpu().numpy().reshape(-1, 3), d_nrm.cpu().numpy().reshape(-1, 3)
        torch.cuda.synchronize()
        for name, buf in extra + [(k, self.guard[k]) for k in self.NAMES]:
            assert _guards_intact(buf), f"the call wrote outside its {name}"
        views = _lib.DifIntegrateViews()
        _lib.check(lib.dif_test_integrate_views(N, _lib.ptr(ws), ctypes.byref(views)), "dif_test_integrate_views")

        def view(name, count, dtype):
            off = getattr(views, name) - ws.data_ptr()
            size = torch.empty((), dtype=dtype).element_size()
            assert 0 <= off and off + count * size <= nb, name
            return ws[off:off + count * size].view(dtype).cpu().numpy()

        r.N = N
        r.counters = c = self.counters.cpu().numpy()
        r.M, r.C = int(c[_lib.C_M]), int(c[_lib.C_C])
        assert 0 <= r.M <= 8 * N and 0 <= r.C <= self.pm.capacity
        r.pt_lin = view("pt_lin", N, torch.int32)
        r.pairs = view("pair_list", 2 * r.M, torch.int32).view(np.uint32).reshape(-1, 2).astype(np.int64)
        tiles = (r.M + 31) // 32
        r.rec = view("rec", tiles * 32 * 32, torch.int64).reshape(-1, 32)
        r.rec_next = view("rec_next", tiles * 32, torch.int32)
        r.mask = mask.cpu().numpy()
        for name in self.NAMES:
            setattr(r, name, getattr(self, name).cpu().numpy())
        r.latent = r.latent.reshape(-1, 29)
        return r


# ---- the checks ---------------------------------------------------------------------------------------------------------------------
def _check_integer_state(res, r, pm, label, img=None):
    """res: what the GPU left; r: the restatement of the same call; pm: the restated map after it"""
    c = res.counters
    assert np.array_equal(res.pt_lin, r.pt_lin), label
    assert np.array_equal(res.mask, r.mask), label
    assert not res.frame_count.any() and not res.alloc_bits.any() and not res.alloc_tot.any() and not res.grid_bits.any() and not res.grid_tot.any(), label
    assert np.array_equal(res.indexer, pm.indexer) and np.array_equal(res.pos, pm.pos), label
    want = {_lib.C_N_OCCUPIED: pm.n, _lib.C_ALLOC_NEW: r.alloc_new, _lib.C_M: r.M, _lib.C_C: r.C, _lib.C_ITEMS: r.items, _lib.C_OVERFLOW: r.overflow}
    assert {k: int(c[k]) for k in want} == want, label
    assert np.array_equal(np.sort(res.upd_list[:r.C]), r.uniq), label
    assert np.array_equal(res.dirty, pm.dirty), label
    pad = np.zeros(res.dirty_tot.size * 256, dtype=np.int64)
    pad[:pm.capacity] = pm.dirty
    assert np.array_equal(res.dirty_tot, pad.reshape(-1, 256).sum(axis=1)), label
    assert not res.rec_dir.any(), label
    assert np.array_equal(res.obs.view(np.uint32), pm.obs.view(np.uint32)), label
    # the pair list: the restatement's pairs as a multiset (a pair's second word is unique, so: as a set, slot by slot)
    order_g, order_r = np.argsort(res.pairs[:, 1], kind="stable"), np.argsort(r.key, kind="stable")
    assert np.array_equal(res.pairs[order_g, 1], r.key[order_r]) and np.array_equal(res.pairs[order_g, 0], r.slot[order_r]), label
    # every workgroup's entries are one range of the list; inside it a slot's entries are one run, but for the loose tail of a workgroup
    # that met more than 256 slots: there the first 256 runs are the table's, and no later entry belongs to one of their slots
    wg = IC.workgroup_of(res.pairs[:, 1], r.N, img)
    loose = 0
    if r.M:
        cut = np.nonzero(np.diff(wg))[0] + 1
        assert cut.size + 1 == np.unique(wg).size, label
        for seg in np.split(res.pairs[:, 0], cut):
            runs = seg[np.concatenate([[True], seg[1:] != seg[:-1]])]
            distinct = np.unique(seg).size
            if distinct <= 256:
                assert runs.size == distinct, label
            else:
                assert np.unique(runs[:256]).size == 256, label
                n_grouped = int(np.isin(seg, runs[:256]).sum())
                assert np.isin(seg[:n_grouped], runs[:256]).all(), label
                loose += seg.size - n_grouped
    return loose


def _check_sums(res, r, model, label):
    """Every run record (located from the pair list read back: tile * 32 + the run's rank) holds the exact sum of its rows'
    rint(e * 2^30), e the same pipe's k_encode_rows output for the restated row, and its length in word 29 -> (C,29) int64 per-slot sums,
    runs per slot (aligned with r.uniq)"""
    if r.M == 0:
        return np.zeros((0, 29), dtype=np.int64), np.zeros(0, dtype=np.int64)
    enc = model.encoder(_t(r.rows, F32)).cpu().numpy()
    finite = ~IC.nonfinite_rows(r.rows)
    assert np.isfinite(enc[finite]).all() and np.abs(enc[finite]).max() < C.ENC_LIMIT, label
    q = np.where(finite[:, None], np.rint(np.where(finite[:, None], enc, 0).astype(np.float64) * IC.FIX), 0).astype(np.int64)
    order = np.argsort(r.key, kind="stable")
    row_of_entry = order[np.searchsorted(r.key[order], res.pairs[:, 1])]
    rec_id, rslot, rlen = IC.runs_of(res.pairs[:, 0])
    start = np.concatenate([[0], np.cumsum(rlen)[:-1]])
    want = np.add.reduceat(q[row_of_entry], start, axis=0)
    recs = res.rec[rec_id]
    n_bad = rlen - np.add.reduceat(finite[row_of_entry].astype(np.int64), start)            # poisoned rows per run (see test_nonfinite_normals)
    assert np.array_equal(recs[:, REC_COUNT_POS], rlen + (n_bad << 40)), label
    clean = n_bad == 0
    wrong = (recs[:, REC_POS] != want)[clean]
    assert not wrong.any(), f"{label}: {int(wrong.any(axis=1).sum())} of {rec_id.size} run records differ from the exact sums of their rows"
    u = np.searchsorted(r.uniq, rslot)
    Si = np.zeros((r.C, 29), dtype=np.int64)
    np.add.at(Si, u, recs[:, REC_POS])
    cnt = np.bincount(u, weights=rlen, minlength=r.C).astype(np.int64)
    assert np.array_equal(cnt, r.cnt), label
    slot_clean = np.bincount(u, weights=n_bad, minlength=r.C) == 0
    assert np.array_equal(Si[slot_clean], IC.fixed_sums(r, np.where(finite[:, None], enc, 0))[slot_clean]), label
    return Si, np.bincount(u, minlength=r.C)


def _check_fusion(res, r, Si, z_prev, w_prev, label, poisoned=None):
    """k_fuse restated in float32 from the exact sums and the GPU's own previous latents and counts: equal bits; every other latent keeps its"""
    z, w = IC.fuse32(z_prev[r.uniq], w_prev[r.uniq], Si, r.cnt)
    if poisoned is not None:
        z[poisoned] = np.nan
    got = res.latent[r.uniq]
    same = (bits(got) == bits(z)) | (np.isnan(got) & np.isnan(z))
    assert same.all(), f"{label}: {int((~same).any(axis=1).sum())} of {r.C} fused voxels differ from the float32 restatement of k_fuse"
    assert np.array_equal(bits(res.obs[r.uniq]), bits(w)), label
    other = np.ones(res.latent.shape[0], dtype=bool)
    other[r.uniq] = False
    assert np.array_equal(bits(res.latent[other]), bits(z_prev[other])), label


def _check_bar(res, r, ws, pipe, label, fails, table):
    """voxels with w_old = 0 under integrate_cases' bar"""
    fresh = r.w_old[r.uniq] == 0
    if not fresh.any():
        return
    mean64, limit, e_ref = IC.mean_bar(ws, r)
    err = np.abs(res.latent[r.uniq].astype(np.float64) - mean64)[fresh]
    per_group = [float(err[:, g].max()) / e for g, e in zip(C.ENC_GROUPS, e_ref)]
    over = err > limit[fresh]
    table.append((label, int(fresh.sum()), max(per_group)))
    print(f"  {label:44s} [{_kernel(pipe)}] {int(fresh.sum()):5d} fresh voxels  largest e_gpu/e_ref {max(per_group):5.2f}  worst err/bar {float((err / limit[fresh]).max()):5.2f}")
    if over.any():
        fails.append(f"{label}: {int(over.sum())} values over the bar, worst err/bar {float((err / limit[fresh]).max()):.2f}")


def _run_case(case, ws, pipe, nets, check_bar=True):
    """Every frame of a case through dif_integrate, all checks -> per frame (result, restatement, runs per slot, loose rows)"""
    model = nets(ws, pipe)
    pm = case.pm.clone()
    dev = Device(pm, model, case.prune_min)
    out, fails, table = [], [], []
    for f, (xyz, nrm) in enumerate(case.frames):
        label = f"{case.label}/{ws}/{pipe} frame {f}"
        z_prev, w_prev = dev.state()
        r = IC.restate(pm, xyz, nrm, case.prune_min)
        res = dev.call(xyz, nrm)
        loose = _check_integer_state(res, r, pm, label)
        Si, n_runs = _check_sums(res, r, model, label)
        if r.M:
            _check_fusion(res, r, Si, z_prev, w_prev, label)
            if check_bar:
                _check_bar(res, r, ws, pipe, label, fails, table)
        else:
            assert np.array_equal(bits(res.latent), bits(z_prev)), label
        out.append((res, r, n_runs, loose))
    assert not fails, "\n".join(fails)
    return out


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ws", IC.WEIGHT_SETS)
@pytest.mark.parametrize("pipe", PIPES)
def test_faces(ws, pipe, nets):
    """Points on voxel faces and the grid's outer faces, one ulp to either side, NaN, +-Inf, -0.0, at N = 1, 63, 64, 65, 255, 256, 257
    (a wave and a workgroup, one short and one over), with prune_min_vox_obs 0 and 1."""
    for n in IC.FACES_N:
        for prune in (0, 1):
            _run_case(IC.faces_case(n, prune), ws, pipe, nets)


@pytest.mark.parametrize("ws", IC.WEIGHT_SETS)
@pytest.mark.parametrize("pipe", PIPES)
def test_runs_corners_alloc64(ws, pipe, nets):
    """runs: a run of 300 equal voxel ids (longer than a wave, across a workgroup edge), runs from lane 0 and lane 63, voxels with exactly
    prune_min and prune_min + 1 points, and the same cloud unpruned.  corners: clamped neighbours coincide with the voxel, and the bitmap
    totals still equal the set bits (or the ordered scan would hand out wrong slots).  alloc64: the multi-block scan (k_scan_pass2 with
    k_prune_mark's block totals) on a map that already holds 40 voxels."""
    for case in (IC.runs_case(4), IC.runs_case(0), IC.corners_case(), IC.alloc64_case()):
        (res, r, _, _), = _run_case(case, ws, pipe, nets)
        assert r.M > 0 and r.alloc_new > 0
        if case.label == "alloc64":
            assert np.unique(r.candidates // 32 // 256).size >= 3 and res.alloc_bits.size > 4096


@pytest.mark.parametrize("ws", IC.WEIGHT_SETS)
@pytest.mark.parametrize("pipe", PIPES)
def test_overflow(ws, pipe, nets):
    """A capacity 8 short of what the frame allocates: DIF_C_OVERFLOW, n_occupied == capacity, the lowest ids allocated and the rest
    left at -1, nothing written past the capacity (AllocFunctor::emit and k_focus_gather's commit both test it)."""
    case = IC.overflow_case()
    (res, r, _, _), = _run_case(case, ws, pipe, nets)
    assert r.overflow == 1 and res.counters[_lib.C_OVERFLOW] == 1 and res.counters[_lib.C_N_OCCUPIED] == case.pm.capacity
    assert (res.indexer[r.candidates[-8:]] == -1).all() and (res.indexer[r.candidates[:-8]] >= 0).all()


@pytest.mark.parametrize("ws", IC.WEIGHT_SETS)
@pytest.mark.parametrize("pipe", PIPES)
def test_threshold(ws, pipe, nets):
    """obs == encoder_count_th exactly is outside the encode set, th - 1 inside; a voxel that crosses th in frame 0 is left alone in
    frames 1 and 2; a point of a voxel outside the set beside one inside it feeds that neighbour.  Three frames, the fusion bit for bit
    each time from the GPU's own previous state; the planted NaN payload, -0.0 and subnormal of an untouched voxel keep their bits."""
    case = IC.threshold_case()
    out = _run_case(case, ws, pipe, nets)
    s = lambda v: case.pm.indexer[OC.lin_of(v)]
    assert s([4, 4, 4]) in out[0][1].uniq and s([4, 4, 6]) not in out[0][1].uniq and s([4, 4, 4]) not in out[1][1].uniq
    assert np.array_equal(bits(out[2][0].latent[s([2, 12, 12])]), bits(case.pm.latent[s([2, 12, 12])]))


@pytest.mark.parametrize("ws", IC.WEIGHT_SETS)
@pytest.mark.parametrize("pipe", PIPES)
def test_chain(ws, pipe, nets):
    """8,192 points: the 27 voxels of a block fed by every workgroup (their directories overflow into the rec_next chain), 40 isolated
    voxels (a few runs each), a tail whose workgroups meet more than 256 slots (k_focus_gather's loose rows), a partly filled last tile;
    frames 0, 1 and 2.  Reach is asserted from the pair list read back."""
    out = _run_case(IC.chain_case(), ws, pipe, nets)
    res, r, n_runs, loose = out[0]
    assert n_runs.max() > IC.DIR_IDS and n_runs.min() <= IC.DIR_IDS and loose > 0 and r.M % 32 != 0, (n_runs.max(), n_runs.min(), loose)
    wg_slots = np.unique(np.stack([IC.workgroup_of(res.pairs[:, 1], r.N), res.pairs[:, 0]], axis=1), axis=0)
    assert np.bincount(wg_slots[:, 0]).max() > 256
    print(f"  chain/{ws}/{pipe}: M {r.M}, C {r.C}, runs per slot {n_runs.min()}..{n_runs.max()}, {int((n_runs > IC.DIR_IDS).sum())} chained slots, {loose} loose rows")
    assert out[1][1].M > 0 and out[2][1].M > 0 and (out[1][1].w_old[out[1][1].uniq] > 0).any()


@pytest.mark.parametrize("pipe", PIPES)
def test_order_independence(pipe, nets):
    """The chain case's first frame under three permutations of its points, N padded with 37 invalid rows: latents, counts, dirty flags
    and indexer bit for bit the same (the sums are integers)."""
    case = IC.chain_case(n_frames=1)
    xyz, nrm = case.frames[0]
    g = np.random.default_rng(107)
    xyz = np.concatenate([xyz, np.full((IC.CHAIN_PAD, 3), np.nan, dtype=F32)])
    nrm = np.concatenate([nrm, OC.unit_normals(g, IC.CHAIN_PAD)])
    model, outs = nets("shipped", pipe), []
    for k in range(3):
        perm = np.arange(xyz.shape[0]) if k == 0 else g.permutation(xyz.shape[0])
        res = Device(case.pm.clone(), model, case.prune_min).call(xyz[perm], nrm[perm])
        outs.append(res)
    for res in outs[1:]:
        for name in ("latent", "obs"):
            assert np.array_equal(bits(getattr(res, name)), bits(getattr(outs[0], name))), f"{name} [{_kernel(pipe)}]"
        assert np.array_equal(res.dirty, outs[0].dirty) and np.array_equal(res.indexer, outs[0].indexer) and np.array_equal(res.pos, outs[0].pos)
    assert outs[0].M > 20000


@pytest.mark.parametrize("hw", ((32, 48), (24, 40)))
@pytest.mark.parametrize("ws", IC.WEIGHT_SETS)
@pytest.mark.parametrize("pipe", PIPES)
def test_frame(pipe, ws, hw, nets):
    """dif_integrate_frame on a depth image with NaN holes, zeros and a non-trivial pose: 32 x 48 walks 16 x 16 pixel tiles in
    k_focus_gather, 24 x 40 the flat 256-point pieces.  With xyz_world / normal_world given (they equal dif_unproject_transform's output)
    and with both NULL (the later stages recompute the points from the depth pixel): all checks of the other cases either way, and the
    same bits as dif_integrate on the H * W points."""
    case = IC.frame_case(*hw)
    model, lib = nets(ws, pipe), _lib.load()
    H, W = hw
    xyz, nrm = case.frames[0]
    d_x, d_n = torch.empty((H * W, 3), device=DEV), torch.empty((H * W, 3), device=DEV)
    R, t = (ctypes.c_float * 9)(*[float(v) for v in case.pose[:9]]), (ctypes.c_float * 3)(*[float(v) for v in case.pose[9:]])
    depth, ncam = _t(case.depth, F32), _t(case.normal_cam, F32)          # (held until the call has run)
    _lib.check(lib.dif_unproject_transform(_lib.ptr(depth), _lib.ptr(ncam), _lib.ptr(d_x), _lib.ptr(d_n), H, W, *case.intr, R, t,
                                           _lib.stream_ptr()), "dif_unproject_transform")
    torch.cuda.synchronize()
    same = lambda a, b: bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())
    assert same(d_x.cpu().numpy(), xyz) and same(d_n.cpu().numpy(), nrm), "the NumPy restatement of unproject_point"
    (flat, r, _, _), = _run_case(case, ws, pipe, nets)
    assert (r.pt_lin < 0).sum() == np.isnan(case.depth).sum() and r.M > 1000 and r.alloc_new > 20
    for with_xyz in (True, False):
        label = f"{case.label}/{ws}/{pipe} xyz_world {'given' if with_xyz else 'NULL'}"
        pm = case.pm.clone()
        dev = Device(pm, model, case.prune_min)
        z_prev, w_prev = dev.state()
        r = IC.restate(pm, xyz, nrm, case.prune_min)
        res = dev.call(frame=case, with_xyz=with_xyz)
        _check_integer_state(res, r, pm, label, img=case.img)
        Si, _ = _check_sums(res, r, model, label)
        _check_fusion(res, r, Si, z_prev, w_prev, label)
        if with_xyz:
            assert same(res.xyz_world, xyz) and same(res.normal_world, nrm), label
        else:
            assert (res.xyz_world.view(np.uint32) == 0x7FC0DEAD).all() and (res.normal_world.view(np.uint32) == 0x7FC0DEAD).all(), label
        for name in ("latent", "obs"):
            assert np.array_equal(bits(getattr(res, name)), bits(getattr(flat, name))), label
        assert np.array_equal(res.dirty, flat.dirty) and np.array_equal(res.indexer, flat.indexer), label


@pytest.mark.parametrize("ws", IC.WEIGHT_SETS)
@pytest.mark.parametrize("pipe", PIPES)
def test_nonfinite_normals(ws, pipe, nets):
    """Five points of the chain case with a finite position and one NaN or +-Inf normal component.  The reference, the oracle and
    k_encode_rows make NaN of such a row, so every latent channel of every voxel it feeds is NaN; counts, mask, pair list and every
    other voxel are what they are without the poison, bit for bit.
    By reading, before the flag existed: the tile loop of k_encode converted whatever encoder_tile made of such a row with
    __float2ll_rn and summed it, and k_fuse divided by the count: finite numbers in up to eight voxels.
    By reading, now: k_encode flags a row with a non-finite input at the gather (as k_encode_rows does at its load: computed, relu1's integer
    max and the conversion to fixed point would turn the row into zeros, saturated or arbitrary finite numbers) and adds 2^40 per such row
    to the run length in record word 29; k_fuse splits the word, counts with the low 40 bits and stores NaN where the high part is set."""
    model = nets(ws, pipe)
    clean, dirty_case = IC.chain_case(n_frames=1), IC.chain_case(n_frames=1, nonfinite=True)
    (xyz, nrm), (xyz_p, nrm_p) = clean.frames[0], dirty_case.frames[0]
    bad_points = np.nonzero(~np.isfinite(nrm_p).all(axis=1))[0]
    assert bad_points.size == 5 and np.array_equal(bits(xyz), bits(xyz_p)) and np.isfinite(xyz[bad_points]).all()
    ref = Device(clean.pm.clone(), model, clean.prune_min).call(xyz, nrm)
    pm = dirty_case.pm.clone()
    dev = Device(pm, model, dirty_case.prune_min)
    z_prev, w_prev = dev.state()
    r = IC.restate(pm, xyz_p, nrm_p, dirty_case.prune_min)
    res = dev.call(xyz_p, nrm_p)
    label = f"{dirty_case.label}/{ws}/{pipe}"
    _check_integer_state(res, r, pm, label)
    bad_rows = IC.nonfinite_rows(r.rows)
    assert np.array_equal(np.unique(r.i[bad_rows]), bad_points) and bad_rows.sum() >= 5
    poisoned = np.zeros(r.C, dtype=bool)
    poisoned[r.inv[bad_rows]] = True
    assert 5 <= poisoned.sum() <= 40
    got = res.latent[r.uniq]
    assert np.isnan(got[poisoned]).all(), f"{label}: {int((~np.isnan(got[poisoned])).any(axis=1).sum())} of {int(poisoned.sum())} voxels fed by a non-finite row hold finite numbers"
    Si, _ = _check_sums(res, r, model, label)
    _check_fusion(res, r, Si, z_prev, w_prev, label, poisoned)
    keep = np.ones(res.latent.shape[0], dtype=bool)
    keep[r.uniq[poisoned]] = False
    assert np.array_equal(bits(res.latent[keep]), bits(ref.latent[keep])), label
    assert np.array_equal(bits(res.obs), bits(ref.obs)) and np.array_equal(res.mask, ref.mask) and np.array_equal(res.dirty, ref.dirty), label
    assert np.array_equal(res.indexer, ref.indexer), label
