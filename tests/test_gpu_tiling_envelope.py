"""The spatially tiled map on planted 16^3 slabs through the C ABI: dif_integrate / dif_integrate_frame under ownership with the boundary
change lists, dif_export_records / dif_export_halo, dif_merge_records / dif_merge_halo / dif_merge_halo2, dif_export_halo_delta and
dif_halo_lists_reset — bit for bit against the NumPy restatements of tests/tiling_cases.py (pinned against the oracle by
tests/test_tiling_cpu.py), the additive merge also against the float64 weighted mean under THE BAR derived there.  Every buffer a call
writes sits between guard words, checked after every call.

WHAT IS REACHED WHERE
  voxel_count_point's px_lo / px_hi, k_focus_gather's ownership gate      test_tiled_integrate (every case), test_tiled_frame (with chunk_any)
  HaloLists::note in AllocFunctor::emit and in k_fuse (s < first_new)      test_tiled_integrate: second_call (both sites, no slot twice), alloc_overflow
  halo_lists_of's clamps and missing sides                                 thin (both lists hold every owned voxel), edge_left, edge_right
  the list cap, flag 8                                                     cap
  ExportFunctor (clamps, empty range, flag 6, both scans)                  test_export_records_and_halo
  k_merge_mark / k_merge_apply (ids, w_r = 0, capacity, headers, 2 sources) test_merge
  k_export_halo_delta / k_halo_lists_reset                                 test_tiled_integrate (on the state every case leaves), test_delta_refusals
"""
import ctypes
import time

import numpy as np
import pytest
import torch

from di_fusion_amd import _lib
from tests import integrate_cases as IC
from tests import test_gpu_integrate_envelope as IE
from tests import tiling_cases as TC
from tests.test_gpu_integrate_envelope import nets  # noqa: F401
from tests.test_gpu_optim_envelope import _guarded, _guards_intact

pytestmark = pytest.mark.gpu
PIPES = IE.PIPES
F32 = np.float32
FILL = 0x5B5B5B5B
T0 = time.perf_counter()
WORST = {"ratio": 0.0, "values": 0}


def _buf(n_words, fill=FILL):
    g, v = _guarded(n_words, torch.int32)
    v.fill_(fill)
    return g, v


def _upload(a):
    """an int32 array in a guarded buffer (a kernel that read past it would read guard words, not foreign memory)"""
    a = np.ascontiguousarray(a, dtype=np.int32).reshape(-1)
    g, v = _guarded(max(a.size, 1), torch.int32)
    if a.size:
        v[:a.size].copy_(torch.from_numpy(a))
    return g, v


def _dev_intact(dev, extra=()):
    torch.cuda.synchronize()
    for name, buf in list(extra) + [(k, dev.guard[k]) for k in dev.NAMES]:
        assert _guards_intact(buf), f"the call wrote outside its {name}"


def _snapshot(dev):
    """every buffer of the map as NumPy arrays"""
    torch.cuda.synchronize()
    r = type("State", (), {})()
    for name in dev.NAMES:
        setattr(r, name, getattr(dev, name).cpu().numpy().copy())
    r.latent = r.latent.reshape(-1, 29)
    return r


def _same_map(st, pm, label, flag=None):
    """the map's persistent state against a restated TMap, and the merge / export scratch back at idle"""
    c = st.counters
    assert np.array_equal(st.indexer, pm.indexer) and np.array_equal(st.pos, pm.pos), label
    assert int(c[_lib.C_N_OCCUPIED]) == pm.n, label
    assert np.array_equal(TC.bits(st.obs), TC.bits(pm.obs)), label
    assert np.array_equal(TC.bits(st.latent), TC.bits(pm.latent)), label
    assert np.array_equal(st.dirty, pm.dirty), label
    assert not st.grid_tot.any() and not st.alloc_tot.any() and not st.alloc_bits.any() and not st.grid_bits.any() and not st.frame_count.any(), label
    if flag is not None:
        assert int(c[_lib.C_OVERFLOW]) == flag, label


# ---- tiled integrate, and the delta export / reset on the state it leaves --------------------------------------------------------------
def _check_lists(res, r, case, label, prev):
    """prev: the list buffer before the call (an export empties a list by its count: the entries stay)"""
    c, cap = res.counters, case.list_cap
    assert (int(c[_lib.C_HALO_L]), int(c[_lib.C_HALO_R])) == r.pending, (label, r.pending)
    assert int(c[_lib.C_ALLOC_KEPT]) == r.alloc_kept, label
    for side in (0, 1):
        lst = res.halo_list[side * cap:(side + 1) * cap]
        kept = lst[:r.kept[side]]
        assert np.array_equal(lst[r.kept[side]:], prev[side * cap:(side + 1) * cap][r.kept[side]:]), label      # nothing written past what the count says
        assert np.unique(kept).size == kept.size, f"{label}: a slot is in list {side} twice"
        if r.pending[side] <= cap:
            assert set(kept.tolist()) == r.lists[side], (label, side, sorted(set(kept.tolist()) ^ r.lists[side]))
        else:
            assert set(kept.tolist()) <= r.lists[side] and kept.size == cap, (label, side)


def _delta(dev, pm, case, max_records, sides, label, hold):
    """dif_export_halo_delta on dev against tiling_cases.export_halo_delta on pm; hold["flag"]: the overflow word before and after
    -> the two messages as NumPy arrays (None for a side without one)"""
    lib = _lib.load()
    bufs = [_buf((1 + max_records) * 32) if s else (None, None) for s in sides]
    g_note, note = _buf(8, -1)
    before = _snapshot(dev)
    _lib.check(lib.dif_export_halo_delta(ctypes.byref(dev.cmap), _lib.ptr(bufs[0][1]), _lib.ptr(bufs[1][1]), max_records, _lib.ptr(note),
                                         _lib.stream_ptr()), "dif_export_halo_delta")
    _dev_intact(dev, [(f"message {k}", b[0]) for k, b in enumerate(bufs) if b[0] is not None] + [("note", g_note)])
    want, flag, wnote = TC.export_halo_delta(pm, case.list_cap, max_records, sides)
    after = _snapshot(dev)
    c = after.counters
    assert (int(c[_lib.C_HALO_L]), int(c[_lib.C_HALO_R])) == (len(pm.lists[0]), len(pm.lists[1])), label      # emptied only where a message went
    assert int(c[_lib.C_HALO_TICKET]) == 0, label
    hold["flag"] = flag or hold["flag"]
    assert int(c[_lib.C_OVERFLOW]) == hold["flag"], label
    assert np.array_equal(note.cpu().numpy().astype(np.int64), wnote), (label, note.cpu().numpy(), wnote)
    for name in ("latent", "obs", "dirty", "indexer", "pos", "halo_list"):
        assert np.array_equal(getattr(after, name).view(np.uint8), getattr(before, name).view(np.uint8)), (label, name)
    out = []
    for side in (0, 1):
        if not sides[side]:
            out.append(None)
            continue
        msg = bufs[side][1].cpu().numpy().reshape(-1, 32)
        w = want[side]
        assert tuple(int(v) for v in msg[0, :3]) == w["header"], (label, side, msg[0, :3], w["header"])
        assert (msg[0, 3:].view(np.uint32) == FILL).all() and (msg[1 + w["n"]:].view(np.uint32) == FILL).all(), label
        rows = {r.tobytes() for r in msg[1:1 + w["n"]]}
        pool = {r.tobytes() for r in w["pool"]}
        assert len(rows) == w["n"], f"{label}: a record is in message {side} twice"
        assert rows == pool if w["exact"] and len(pool) == w["n"] else rows <= pool, (label, side)
        out.append(msg)
    return out


def _reset(dev, pm, sides, label):
    lib = _lib.load()
    hdrs = [_buf(32) if s else (None, None) for s in sides]
    for k, (g, v) in enumerate(hdrs):
        if v is not None:
            v[:3].copy_(torch.tensor([77 + k, 5, 1], dtype=torch.int32))
    g_note, note = _buf(8, -1)
    _lib.check(lib.dif_halo_lists_reset(ctypes.byref(dev.cmap), _lib.ptr(hdrs[0][1]), _lib.ptr(hdrs[1][1]), _lib.ptr(note), _lib.stream_ptr()),
               "dif_halo_lists_reset")
    _dev_intact(dev, [(f"header {k}", b[0]) for k, b in enumerate(hdrs) if b[0] is not None] + [("note", g_note)])
    want, wnote = TC.halo_lists_reset(pm, [(77 + k, 5, 1) if s else None for k, s in enumerate(sides)])
    c = dev.counters.cpu().numpy()
    assert (int(c[_lib.C_HALO_L]), int(c[_lib.C_HALO_R])) == (len(pm.lists[0]), len(pm.lists[1])), label
    assert np.array_equal(note.cpu().numpy().astype(np.int64), wnote), label
    for k, (g, v) in enumerate(hdrs):
        if v is not None:
            h = v.cpu().numpy()
            assert tuple(int(x) for x in h[:3]) == want[k] and (h[3:].view(np.uint32) == FILL).all(), (label, k)


def _integrate(dev, pm, case, frame, model, label, img=None, hold=None, call=None):
    """one frame through the GPU and the restatement, every check of the integrate envelope and the lists"""
    xyz, nrm = frame
    dev.counters[_lib.C_OVERFLOW] = 0                                       # (the flag is sticky: its reader clears it)
    if hold is not None:
        hold["flag"] = 0
    z_prev, w_prev = dev.state()
    prev = dev.halo_list.cpu().numpy().copy()
    r = TC.restate_tiled(pm, xyz, nrm, case.prune_min, own=case.own, halo=case.halo, list_cap=case.list_cap)
    res = dev.call(**call) if call else dev.call(xyz, nrm)
    IE._check_integer_state(res, r, pm, label, img=img)
    Si, _ = IE._check_sums(res, r, model, label)
    if r.M:
        IE._check_fusion(res, r, Si, z_prev, w_prev, label)
    pm.latent[:] = res.latent                                               # the restated map goes on from the GPU's latents (checked just now)
    _check_lists(res, r, case, label, prev)
    return res, r


@pytest.mark.parametrize("name", TC.INTEGRATE_CASES)
@pytest.mark.parametrize("pipe", PIPES)
def test_tiled_integrate(pipe, name, nets):
    """dif_integrate on a slab: pt_lin, mask, indexer, pos, counters, the pair list as a set, the exact per-slot sums, the fused latents and
    counts bit for bit; the two change lists as sets and their counts.  Then the delta export on what the call left (one side first — the other
    side's list and count survive and the next call delivers them), and dif_halo_lists_reset.
    alloc_overflow: the capacity cuts the allocation.  Before DIF_C_ALLOC_KEPT k_fuse took n_occupied (clamped) - ALLOC_NEW (not clamped) for
    the first new slot: 16 too low here, and the fused older slots of the right boundary layers above that line were missing from the list."""
    case = TC.integrate_case(name)
    model = nets("shipped", pipe)
    pm = case.pm.clone()
    dev = IE.Device(pm, model, case.prune_min, own=case.own, halo=case.halo, list_cap=case.list_cap)
    hold = {"flag": 0}
    for f, frame in enumerate(case.frames):
        label = f"{name}/{pipe} frame {f}"
        res, r = _integrate(dev, pm, case, frame, model, label, hold=hold)
        hold["flag"] = r.overflow
        assert r.M > 0 and r.dropped_pairs > 0, label
        if name == "alloc_overflow":
            assert r.overflow == 1 and int(res.counters[_lib.C_N_OCCUPIED]) == pm.capacity and int(res.counters[_lib.C_ALLOC_NEW]) == r.alloc_kept + TC.SHORT
        first = (True, False) if (f + len(name)) % 2 else (False, True)
        rows = 4096
        _delta(dev, pm, case, rows, first, f"{label} delta {first}", hold)
        _delta(dev, pm, case, rows, (not first[0], not first[1]), f"{label} delta, the other side", hold)
        _delta(dev, pm, case, rows, (True, True), f"{label} delta, nothing pending", hold)
        if name == "cap":
            assert hold["flag"] == 8 and r.pending[0] > case.list_cap
    # a list is dropped by the reset (one side, then both)
    xyz, nrm = case.frames[-1]
    res, r = _integrate(dev, pm, case, (xyz, nrm), model, f"{name}/{pipe} once more", hold=hold)
    assert sum(r.pending) > 0
    _reset(dev, pm, (False, True), f"{name}/{pipe} reset right")
    _reset(dev, pm, (True, True), f"{name}/{pipe} reset both")
    # fewer records than pending: flag 8, the count in the header
    res, r = _integrate(dev, pm, case, (xyz, nrm), model, f"{name}/{pipe} a third time", hold=hold)
    hold["flag"] = r.overflow
    if max(r.pending) > 2:
        _delta(dev, pm, case, 2, (True, True), f"{name}/{pipe} delta of 2 records", hold)
        assert hold["flag"] == 8


@pytest.mark.parametrize("hw", ((32, 48), (33, 47)))
@pytest.mark.parametrize("pipe", PIPES)
def test_tiled_frame(pipe, hw, nets):
    """dif_integrate_frame on a slab (32 x 48: 16 x 16 pixel tiles; 33 x 47: the flat walk), with at least one 256-point piece of the frame
    entirely outside slab + halo (chunk_any: k_prune_mark and k_focus_gather skip it), xyz_world given and NULL: the restatement's state, and
    the point path's bits."""
    case = TC.frame_case(*hw)
    culled, pieces = TC.culled_pieces(case)
    assert 1 <= culled < pieces
    model = nets("shipped", pipe)
    xyz, nrm = case.frames[0]
    pm = case.pm.clone()
    flat, _ = _integrate(IE.Device(pm, model, case.prune_min, own=case.own, halo=case.halo, list_cap=case.list_cap), pm, case, (xyz, nrm), model,
                         f"{case.label}/{pipe} points")
    for with_xyz in (True, False):
        label = f"{case.label}/{pipe} xyz_world {'given' if with_xyz else 'NULL'}"
        pm = case.pm.clone()
        dev = IE.Device(pm, model, case.prune_min, own=case.own, halo=case.halo, list_cap=case.list_cap)
        res, r = _integrate(dev, pm, case, (xyz, nrm), model, label, img=case.img, call=dict(frame=case, with_xyz=with_xyz))
        for k in ("latent", "obs"):
            assert np.array_equal(TC.bits(getattr(res, k)), TC.bits(getattr(flat, k))), (label, k)
        for k in ("dirty", "indexer", "pos", "mask", "pt_lin"):
            assert np.array_equal(getattr(res, k), getattr(flat, k)), (label, k)
        for side in (0, 1):
            cap = case.list_cap
            assert set(res.halo_list[side * cap:side * cap + r.kept[side]].tolist()) == set(flat.halo_list[side * cap:side * cap + r.kept[side]].tolist()), label


# ---- exports ---------------------------------------------------------------------------------------------------------------------------
def _export(dev, pm, x_lo, x_hi, raw, max_records, halo, label, flag_before=0):
    lib = _lib.load()
    rows = max_records + (1 if halo else 0)
    g_out, out = _buf(rows * 32)
    g_s, scratch = _buf(4096)
    before = _snapshot(dev)
    if halo:
        rc = lib.dif_export_halo(ctypes.byref(dev.cmap), _lib.ptr(out), max_records, x_lo, x_hi, _lib.ptr(scratch), _lib.stream_ptr())
    else:
        rc = lib.dif_export_records(ctypes.byref(dev.cmap), _lib.ptr(out), max_records, x_lo, x_hi, 1 if raw else 0, _lib.ptr(scratch), _lib.stream_ptr())
    assert rc == 0, label
    _dev_intact(dev, [("records", g_out), ("scratch", g_s)])
    want, count, flag = TC.export_records(pm, x_lo, x_hi, raw or halo, max_records)
    got = out.cpu().numpy().reshape(-1, 32)
    after = _snapshot(dev)
    assert int(after.counters[_lib.C_EXPORT_N]) == count and int(after.counters[_lib.C_OVERFLOW]) == (flag or flag_before), (label, count)
    if halo:
        assert int(got[0, 0]) == count and (got[0, 1:].view(np.uint32) == FILL).all(), label
        got = got[1:]
    wf, gf = want[:, 3:].copy().view(F32), got[:count, 3:].copy().view(F32)
    assert np.array_equal(got[:count, :3], want[:, :3]), label
    assert ((got[:count, 3:] == want[:, 3:]) | (np.isnan(wf) & np.isnan(gf))).all(), label
    assert (got[count:].view(np.uint32) == FILL).all(), f"{label}: rows past the count were written"
    for name in ("latent", "obs", "dirty", "indexer", "pos"):
        assert np.array_equal(getattr(after, name).view(np.uint8), getattr(before, name).view(np.uint8)), (label, name)
    return count, flag


def test_export_records_and_halo():
    """dif_export_records (payload z * w and raw) and dif_export_halo over every range of tiling_cases.EXPORT_RANGES (slots on both sides of
    each cut, x_lo < 0, x_hi > nx, empty and inverted ranges), max_records one below the count (flag 6, the count clamped, the first records
    in slot order), on a capacity of 1,024 (the single-workgroup scan) and of 8,192 (two passes); the refusals write nothing."""
    lib = _lib.load()
    for capacity, n in ((1024, 150), (8192, 150), (8192, 3000)):
        pm = TC.export_map(n=n, capacity=capacity)
        dev = IE.Device(pm, None, 0)
        for x_lo, x_hi in TC.EXPORT_RANGES:
            for raw in (False, True):
                count, flag = _export(dev, pm, x_lo, x_hi, raw, n + 7, False, f"records cap {capacity} n {n} [{x_lo},{x_hi}) raw {raw}")
                assert flag == 0
            count2, _ = _export(dev, pm, x_lo, x_hi, True, n + 7, True, f"halo cap {capacity} n {n} [{x_lo},{x_hi})")
            assert count2 == count
        count, _ = _export(dev, pm, 5, 11, False, 4096, False, "count")
        assert count > 10
        for halo in (False, True):
            got, flag = _export(dev, pm, 5, 11, False, count - 1, halo, f"one short, halo {halo}", flag_before=6 if halo else 0)
            assert got == count - 1 and flag == 6
        # refusals: nothing is written
        g_out, out = _buf(64 * 32)
        g_s, scratch = _buf(4096)
        before = _snapshot(dev)
        m, st = ctypes.byref(dev.cmap), _lib.stream_ptr()
        assert lib.dif_export_records(m, _lib.ptr(out), 0, 0, 16, 0, _lib.ptr(scratch), st) == -1
        assert lib.dif_export_records(m, _lib.ptr(out), -5, 0, 16, 0, _lib.ptr(scratch), st) == -1
        assert lib.dif_export_records(m, None, 64, 0, 16, 0, _lib.ptr(scratch), st) == -1
        assert lib.dif_export_records(m, _lib.ptr(out), 64, 0, 16, 0, None, st) == -1
        assert lib.dif_export_records(None, _lib.ptr(out), 64, 0, 16, 0, _lib.ptr(scratch), st) == -1
        assert lib.dif_export_halo(m, None, 63, 0, 16, _lib.ptr(scratch), st) == -1
        assert lib.dif_export_halo(m, _lib.ptr(out), 0, 0, 16, _lib.ptr(scratch), st) == -1
        assert lib.dif_export_halo(m, _lib.ptr(out), 63, 0, 16, None, st) == -1
        _dev_intact(dev, [("records", g_out), ("scratch", g_s)])
        after = _snapshot(dev)
        assert (out.cpu().numpy().view(np.uint32) == FILL).all() and (scratch.cpu().numpy().view(np.uint32) == FILL).all()
        for name in dev.NAMES:
            assert np.array_equal(getattr(after, name).view(np.uint8), getattr(before, name).view(np.uint8)), name


# ---- merges ----------------------------------------------------------------------------------------------------------------------------
def _merge(dev, sources, assign, how, note=False):
    """sources: [(rec, header or None)] -> after the call: the state, and the eight note words (dif_merge_halo2) or None"""
    lib = _lib.load()
    g_s, scratch = _buf(4096)
    held, extra = [], [("scratch", g_s)]
    m, st = ctypes.byref(dev.cmap), _lib.stream_ptr()
    msgs = []
    used = np.concatenate([dev.pm.pos[:dev.pm.n]] + [rec[:, 0].astype(np.int64) for rec, _ in sources])
    decoy_ids = np.setdiff1d(np.arange(TC.GRID ** 3), used)[-16:].reshape(2, 8)
    for k, (rec, hdr) in enumerate(sources):
        if how == "records":
            held.append(_upload(rec))
        else:
            msg = TC.message(rec, rec.shape[0], header=hdr)
            msg[0, 1:4] = (11, 22, 33)
            msgs.append(msg)
            # behind the message's rows: eight well-formed records of free voxels, which a count that is not held to max_records would merge
            decoys = np.zeros((8, 32), dtype=np.int32)
            decoys[:, 0], decoys[:, 1], decoys[:, 2], decoys[:, 3:] = decoy_ids[k], 1, TC.i32(np.full(8, 5.0, F32)), TC.i32(F32(0.25))[0]
            held.append(_upload(np.concatenate([msg, decoys])))
    g_note, d_note = _buf(8, -1)
    if how == "records":
        rc = lib.dif_merge_records(m, _lib.ptr(held[0][1]), sources[0][0].shape[0], 1 if assign else 0, _lib.ptr(scratch), st)
    elif how == "halo":
        rc = lib.dif_merge_halo(m, _lib.ptr(held[0][1]), sources[0][0].shape[0], _lib.ptr(scratch), st)
    else:
        a = held[0][1] if sources[0] is not None else None
        b = held[1][1] if len(held) > 1 else None
        rc = lib.dif_merge_halo2(m, _lib.ptr(a), sources[0][0].shape[0], _lib.ptr(b), sources[1][0].shape[0] if b is not None else 0, _lib.ptr(scratch),
                                 _lib.ptr(d_note) if note else None, st)
    assert rc == 0, how
    _dev_intact(dev, extra + [("note", g_note)])
    for (g, v), (rec, hdr) in zip(held, sources):
        assert _guards_intact(g)
    return _snapshot(dev), (d_note.cpu().numpy() if note else None), msgs


def _by_voxel(st):
    """a map's content by voxel id (slot numbers depend on the order of the calls)"""
    s = st.indexer
    have = s >= 0
    k = np.maximum(s, 0)
    return have, np.where(have, TC.bits(st.obs)[k], 0), np.where(have[:, None], TC.bits(st.latent)[k], 0), np.where(have, st.dirty[k], 0)


@pytest.mark.parametrize("name", TC.RECORD_SETS)
def test_merge(name):
    """dif_merge_records (additive and assign), dif_merge_halo and dif_merge_halo2 on every record set of tiling_cases: indexer, pos,
    n_occupied, ALLOC_NEW back at 0, counts, latents, dirty flags, flag 1, the note words and the bitmap totals back at idle against the
    restatement bit for bit; every slot no record names keeps its bits (the planted NaN payload, -0.0 and subnormal under a w_r = 0 record
    too); the additive result against the float64 weighted mean inside THE BAR."""
    rs = TC.record_set(name)
    single = len(rs.sources) == 1
    plans = []
    if single and rs.sources[0][1] is None:
        plans += [("records", False), ("records", True)]
    if single:
        hdr = rs.sources[0][1]
        src = [(rs.sources[0][0], rs.sources[0][0].shape[0] if hdr is None else hdr)]
        plans += [("halo", True, src), ("halo2", True, src)]
    else:
        plans += [("halo2", True, rs.sources)]
    for plan in plans:
        how, assign = plan[0], plan[1]
        sources = plan[2] if len(plan) > 2 else rs.sources
        label = f"{name}: {how}{' assign' if assign else ''}"
        pm = rs.pm.clone()
        dev = IE.Device(pm, None, 0)
        before = _snapshot(dev)
        st, note, msgs = _merge(dev, sources, assign, how, note=(how == "halo2"))
        flag, named = TC.merge(pm, [TC.Source(r, h if how != "records" else None) for r, h in sources], assign)
        _same_map(st, pm, label, flag=flag)
        assert int(st.counters[_lib.C_ALLOC_NEW]) == 0, label
        rest = np.ones(pm.capacity, dtype=bool)
        rest[named] = False
        assert np.array_equal(TC.bits(st.latent[rest]), TC.bits(before.latent[rest])) and np.array_equal(TC.bits(st.obs[rest]), TC.bits(before.obs[rest])), label
        assert np.array_equal(st.dirty[rest], before.dirty[rest]), label
        if how == "halo2":
            want = TC.merge_note([m[0] for m in msgs] + [None] * (2 - len(msgs)))
            assert np.array_equal(note, want), (label, note, want)
        if how == "records" and not assign:
            got = pm.clone()
            got.latent[:] = st.latent
            ratio, count = TC.bar_ratio(rs.pm, got, rs)
            print(f"  {label:28s} {count:6d} merged values  worst |z - mean64| / bar {ratio:.3f}")
            WORST["ratio"], WORST["values"] = max(WORST["ratio"], ratio), WORST["values"] + count
            assert ratio <= 1.0, f"{label}: over THE BAR, worst ratio {ratio:.3f}"
            if name == "mixed":
                assert 3 in named and np.array_equal(TC.bits(st.latent[3]), TC.bits(rs.pm.latent[3])) and np.isnan(st.latent[3, 0])
        if name == "overrun":
            assert flag == 1 and int(st.counters[_lib.C_N_OCCUPIED]) == pm.capacity
    if name == "two":
        # both messages in one pass against one message per call, in either order: the same map, voxel by voxel
        one = _by_voxel(_merge(IE.Device(rs.pm.clone(), None, 0), rs.sources, True, "halo2")[0])
        for order in ((0, 1), (1, 0)):
            dev = IE.Device(rs.pm.clone(), None, 0)
            for k in order:
                st = _merge(dev, [rs.sources[k]], True, "halo")[0]
            for a, b in zip(one, _by_voxel(st)):
                assert np.array_equal(a, b), order
    print(f"  so far: worst merge-bar ratio {WORST['ratio']:.3f} over {WORST['values']} values")


def test_merge_refusals_and_empty():
    lib = _lib.load()
    rs = TC.record_set("n2")
    dev = IE.Device(rs.pm.clone(), None, 0)
    g_s, scratch = _buf(4096)
    g_r, rec = _upload(rs.sources[0][0])
    before = _snapshot(dev)
    m, st = ctypes.byref(dev.cmap), _lib.stream_ptr()
    assert lib.dif_merge_records(m, _lib.ptr(rec), -1, 0, _lib.ptr(scratch), st) == -1
    assert lib.dif_merge_records(m, None, 2, 0, _lib.ptr(scratch), st) == -1
    assert lib.dif_merge_records(m, _lib.ptr(rec), 2, 0, None, st) == -1
    assert lib.dif_merge_halo(m, None, 2, _lib.ptr(scratch), st) == -1
    assert lib.dif_merge_halo(m, _lib.ptr(rec), 0, _lib.ptr(scratch), st) == -1
    assert lib.dif_merge_halo2(m, _lib.ptr(rec), 0, None, 0, _lib.ptr(scratch), None, st) == -1
    assert lib.dif_merge_records(m, _lib.ptr(rec), 0, 0, _lib.ptr(scratch), st) == 0          # no records: nothing to do
    assert lib.dif_merge_halo2(m, None, 0, None, 0, _lib.ptr(scratch), None, st) == 0
    _dev_intact(dev, [("scratch", g_s)])
    after = _snapshot(dev)
    for name in dev.NAMES:
        assert np.array_equal(getattr(after, name).view(np.uint8), getattr(before, name).view(np.uint8)), name


def test_delta_refusals():
    """dif_export_halo_delta refuses an untiled map, halo <= 0, a map without a list and max_records <= 0, and writes nothing"""
    lib = _lib.load()
    case = TC.integrate_case("cut_mid")
    g_m, msg = _buf(65 * 32)
    for own, halo, cap, rows in (((0, TC.GRID), 3, 64, 64), (None, 3, 64, 64), ((5, 11), 0, 64, 64), ((5, 11), -1, 64, 64), ((5, 11), 3, 0, 64),
                                 ((5, 11), 3, 64, 0), ((5, 11), 3, 64, -2), ((9, 9), 3, 64, 64)):
        dev = IE.Device(case.pm.clone(), None, 2, own=own, halo=halo, list_cap=cap)
        before = _snapshot(dev)
        rc = lib.dif_export_halo_delta(ctypes.byref(dev.cmap), _lib.ptr(msg), _lib.ptr(msg), rows, None, _lib.stream_ptr())
        assert rc == -1, (own, halo, cap, rows)
        _dev_intact(dev, [("message", g_m)])
        after = _snapshot(dev)
        assert (msg.cpu().numpy().view(np.uint32) == FILL).all()
        for name in dev.NAMES:
            assert np.array_equal(getattr(after, name).view(np.uint8), getattr(before, name).view(np.uint8)), name
    assert lib.dif_export_halo_delta(None, _lib.ptr(msg), _lib.ptr(msg), 64, None, _lib.stream_ptr()) == -1


# ---- the closed loop -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipe", PIPES)
def test_two_slabs_equal_the_full_map(pipe, nets):
    """A full 16^3 map and two slabs cut at x = 8 (halo 3) over three clouds of 2,000 points: integrate, delta export, hand-over by device copy,
    dif_merge_halo2.  The full map is checked against the restatement as in the integrate envelope; the owned voxels of both slabs equal it
    bit for bit after every frame (ids, counts, latents, dirty flags).  The small twin of test_spatial_tiling_matches_single_map_bit_for_bit."""
    lib = _lib.load()
    model = nets("shipped", pipe)
    G, cut, halo, cap, rows = TC.GRID, TC.CUT, 3, 3 * TC.PLANE, 3 * TC.PLANE
    full_pm = TC.TMap(np.zeros(0, dtype=np.int64), 4096)
    full = IE.Device(full_pm, model, 2)
    slabs = [IE.Device(TC.TMap(np.zeros(0, dtype=np.int64), 4096), model, 2, own=own, halo=halo, list_cap=cap) for own in ((0, cut), (cut, G))]
    g_s, scratch = _buf(4096)
    for f, (xyz, nrm) in enumerate(TC.loop_clouds()):
        label = f"loop/{pipe} frame {f}"
        z_prev, w_prev = full.state()
        r = IC.restate(full_pm, xyz, nrm, 2)
        res = full.call(xyz, nrm)
        IE._check_integer_state(res, r, full_pm, label)
        Si, _ = IE._check_sums(res, r, model, label)
        IE._check_fusion(res, r, Si, z_prev, w_prev, label)
        for dev in slabs:
            dev.call(xyz, nrm)
        msgs = []
        for k, dev in enumerate(slabs):                                    # slab 0 sends its right layers, slab 1 its left layers
            g_m, msg = _buf((1 + rows) * 32)
            _lib.check(lib.dif_export_halo_delta(ctypes.byref(dev.cmap), None if k == 0 else _lib.ptr(msg), _lib.ptr(msg) if k == 0 else None, rows, None,
                                                 _lib.stream_ptr()), "dif_export_halo_delta")
            _dev_intact(dev, [("message", g_m)])
            assert 0 < int(msg[0]) == int(msg[1]) <= cap and int(msg[2]) == 1, label
            msgs.append((g_m, msg))
        for k, dev in enumerate(slabs):
            g_in, got = _buf((1 + rows) * 32)
            got.copy_(msgs[1 - k][1])                                      # the hand-over: a device copy of the neighbour's message
            _lib.check(lib.dif_merge_halo2(ctypes.byref(dev.cmap), _lib.ptr(got), rows, None, 0, _lib.ptr(scratch), None, _lib.stream_ptr()), "dif_merge_halo2")
            _dev_intact(dev, [("message", g_in), ("scratch", g_s)])
        want = _by_voxel(_snapshot(full))
        x = np.arange(G ** 3) // TC.PLANE
        for k, dev in enumerate(slabs):
            st = _snapshot(dev)
            assert int(st.counters[_lib.C_OVERFLOW]) == 0, label
            owned = (x < cut) if k == 0 else (x >= cut)
            for what, a, b in zip(("allocated", "counts", "latents", "dirty flags"), want, _by_voxel(st)):
                assert np.array_equal(a[owned], b[owned]), f"{label}: the {what} of slab {k}'s owned voxels differ from the full map's"
            assert (want[1][owned] != 0).sum() > 50, label


def test_report():
    """(last in the file) the worst merge-bar ratio and the file's wall time"""
    print(f"\n  worst |z - mean64| / THE BAR over {WORST['values']} merged values: {WORST['ratio']:.3f};  the file took {time.perf_counter() - T0:.1f} s")
    assert WORST["ratio"] <= 1.0
