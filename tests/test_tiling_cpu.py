"""tests/tiling_cases.py on the CPU: the tiled restatements against the oracle, the cases against the paths they are named for, and the
float32 merge against THE BAR (no GPU)."""
import numpy as np
import pytest

from oracle import difusion_oracle as O
from tests import integrate_cases as IC
from tests import optim_cases as OC
from tests import tiling_cases as TC

F32 = np.float32
G = TC.GRID


def _oracle_of(pm, prune_min=0):
    """an OracleMap in pm's state (slot order, latents, counts, dirty set)"""
    _, net = IC.nets("shipped")
    hi = tuple(float(v) + pm.grid * pm.voxel_size for v in OC.BOUND_MIN)
    om = O.OracleMap(net, OC.BOUND_MIN, hi, pm.voxel_size, prune_min_vox_obs=prune_min, encoder_count_th=IC.TH)
    assert om.n_xyz == [pm.grid] * 3
    om.allocate_block(pm.pos[:pm.n].copy())
    om.latent_vecs[:pm.n], om.voxel_obs_count[:pm.n] = pm.latent[:pm.n], pm.obs[:pm.n]
    om.updated_vec_id = np.nonzero(pm.dirty[:pm.n])[0].astype(np.int64)
    return om


def _same_state(om, pm, label):
    n = pm.n
    assert om.n_occupied == n and np.array_equal(om.indexer, pm.indexer) and np.array_equal(om.latent_vecs_pos[:n], pm.pos[:n]), label
    assert np.array_equal(TC.bits(om.voxel_obs_count[:n]), TC.bits(pm.obs[:n])), label
    assert TC.same_bits(om.latent_vecs[:n], pm.latent[:n]), label
    assert np.array_equal(om.updated_vec_id, np.nonzero(pm.dirty[:n])[0]), label


def test_whole_grid_is_the_untiled_restatement():
    """own = the whole grid (with and without a halo and a list): every field of integrate_cases.restate, and no list entry"""
    cases = [IC.faces_case(257, 1), IC.runs_case(4), IC.corners_case(), IC.threshold_case(), IC.overflow_case(), IC.frame_case(24, 40)]
    for case in cases:
        for own, halo, cap in ((None, 0, 0), ((0, G), 3, 64), ((4, 4), 2, 64)):
            if case.pm.grid != G:
                continue
            a, b = case.pm.clone(), TC.TMap.of(case.pm)
            for xyz, nrm in case.frames:
                ra = IC.restate(a, xyz, nrm, case.prune_min)
                rb = TC.restate_tiled(b, xyz, nrm, case.prune_min, own=own, halo=halo, list_cap=cap)
                for k, v in vars(ra).items():
                    w = getattr(rb, k)
                    assert (TC.same_bits(v, w) if isinstance(v, np.ndarray) and v.dtype == F32 else np.array_equal(v, w)), (case.label, k)
                assert rb.pending == (0, 0) and rb.dropped_pairs == 0
                for k in ("indexer", "pos", "obs", "dirty"):
                    assert np.array_equal(getattr(a, k), getattr(b, k)), (case.label, k)


@pytest.mark.parametrize("name", [n for n in TC.INTEGRATE_CASES if n != "alloc_overflow"])        # (the oracle grows its buffers: no capacity to overrun)
def test_tiled_restatement_matches_the_oracle_on_owned_voxels(name):
    """OracleMap.integrate_keyframe on the points the slab keeps (the rule of test_parallel_gloo's _OracleSlabMap.integrate), from the
    restated state before every frame: allocation everywhere; ids, counts and dirty flags of the owned voxels; and the encode rows — the
    untiled restatement of the kept points (which test_ref64_cpu pins against the oracle) cut down to the pairs with an owned target."""
    case = TC.integrate_case(name)
    pm = case.pm.clone()
    lo, hi = case.own
    for f, (xyz, nrm) in enumerate(case.frames):
        label = f"{name} frame {f}"
        om, flat = _oracle_of(pm, case.prune_min), IC.IMap.clone(pm)
        r = TC.restate_tiled(pm, xyz, nrm, case.prune_min, own=case.own, halo=case.halo, list_cap=case.list_cap)
        ix = np.ceil((xyz[:, 0] - om.bound_min[0]) / F32(om.voxel_size)).astype(np.int64) - 1
        keep = (ix >= lo - case.halo) & (ix < hi + case.halo)
        assert np.array_equal(keep & (IC.voxel_ids(flat, xyz) >= 0), r.pt_lin >= 0), label
        keep &= IC.voxel_ids(flat, xyz) >= 0                            # (the oracle would index with a point outside the grid)
        omask = om.integrate_keyframe(xyz[keep], nrm[keep])
        mask = np.zeros(r.N, dtype=np.uint8)
        mask[keep] = omask
        assert np.array_equal(mask, r.mask), label
        assert om.n_occupied == pm.n and np.array_equal(om.indexer, pm.indexer) and np.array_equal(om.latent_vecs_pos[:pm.n], pm.pos[:pm.n]), label
        owned = (pm.pos[:pm.n] // TC.PLANE >= lo) & (pm.pos[:pm.n] // TC.PLANE < hi)
        assert np.array_equal(TC.bits(om.voxel_obs_count[:pm.n][owned]), TC.bits(pm.obs[:pm.n][owned])), label
        assert np.array_equal(np.isin(np.arange(pm.n), om.updated_vec_id)[owned], pm.dirty[:pm.n][owned] != 0), label
        assert not pm.dirty[:pm.n][~owned].any() or f > 0, label
        rf = IC.restate(flat, xyz[keep], nrm[keep], case.prune_min)
        orig = np.nonzero(keep)[0]
        tx = flat.pos[rf.slot] // TC.PLANE
        sel = (tx >= lo) & (tx < hi)
        assert sel.sum() == r.M > 0 and (~sel).sum() == r.dropped_pairs > 0, label
        assert np.array_equal(rf.o[sel], r.o) and np.array_equal(orig[rf.i[sel]], r.i) and np.array_equal(rf.slot[sel], r.slot), label
        assert TC.same_bits(rf.rows[sel], r.rows), label


def test_integrate_cases_reach_their_paths():
    out = {}
    for name in TC.INTEGRATE_CASES:
        case = TC.integrate_case(name)
        pm = case.pm.clone()
        rs = []
        for xyz, nrm in case.frames:
            valid = IC.voxel_ids(pm, xyz) >= 0
            r = TC.restate_tiled(pm, xyz, nrm, case.prune_min, own=case.own, halo=case.halo, list_cap=case.list_cap)
            r.culled = valid & (r.pt_lin < 0)
            r.cx = IC.voxel_ids(pm, xyz) // TC.PLANE
            rs.append(r)
            if name == "second_call":
                TC.export_halo_delta(pm, case.list_cap, 4096)          # the lists are handed over between the calls
        out[name] = (case, pm, rs)
    lo, hi = 5, 11
    case, pm, (r,) = out["cut_mid"]
    assert (r.cx[r.culled] < lo - 3).any() and (r.cx[r.culled] >= hi + 3).any()
    for x in (lo - 3, lo - 1, lo, hi - 1, hi, hi + 2):                  # first voxel in and out at every cut: points of it are kept
        assert ((r.cx == x) & (r.mask == 1)).any(), x
    for x in (lo - 4, hi + 3):
        assert (r.cx == x).any() and not ((r.cx == x) & (r.pt_lin >= 0)).any(), x
    px, tx = r.cx[r.i], pm.pos[r.slot] // TC.PLANE
    assert ((px < lo) & (tx == lo)).any() and ((px >= hi) & (tx == hi - 1)).any() and r.dropped_pairs > 0
    assert all(r.noted_new[s] and r.noted_old[s] for s in (0, 1)) and not (r.lists[0] & r.lists[1])
    assert max(r.pending) <= case.list_cap and r.overflow == 0
    case, pm, (r,) = out["thin"]
    assert r.lists[0] == r.lists[1] and len(r.lists[0]) > 4
    owned = (pm.pos[:pm.n] // TC.PLANE >= 7) & (pm.pos[:pm.n] // TC.PLANE < 9)
    assert set(np.nonzero(owned)[0][np.nonzero(owned)[0] >= r.n_before]) <= r.lists[0]
    case, pm, (r,) = out["edge_left"]
    assert not r.lists[0] and r.lists[1] and r.culled.any() and (r.cx[r.culled] >= 9).all()
    assert {int(x) for x in pm.pos[sorted(r.lists[1])] // TC.PLANE} == {3, 4, 5}
    case, pm, (r,) = out["edge_right"]
    assert r.lists[0] and not r.lists[1] and r.culled.any() and (r.cx[r.culled] < 7).all()
    assert {int(x) for x in pm.pos[sorted(r.lists[0])] // TC.PLANE} == {10, 11, 12}
    case, pm, (r,) = out["cap"]
    assert min(r.pending) > case.list_cap == 4 and r.kept == (4, 4)
    assert TC.export_halo_delta(pm, case.list_cap, 4096)[1] == 8        # flag 8
    case, pm, (r0, r1) = out["second_call"]
    for s in (0, 1):
        assert r1.noted_new[s] and r1.noted_old[s] and not (r1.noted_new[s] & r1.noted_old[s])
        assert r1.pending[s] == len(r1.lists[s])                        # no slot twice
        assert r1.noted_old[s] & r0.noted_new[s]                        # a slot the first call allocated is fused by the second
    fused_new = set(r1.uniq[r1.uniq >= r1.n_before])
    assert fused_new & (r1.noted_new[0] | r1.noted_new[1])              # allocated AND fused in one call: noted once
    case, pm, (r,) = out["alloc_overflow"]
    assert r.overflow == 1 and pm.n == pm.capacity and r.alloc_new - r.alloc_kept == TC.SHORT
    wrong_line = pm.capacity - r.alloc_new                               # n_occupied - ALLOC_NEW: what k_fuse once took for the first new slot
    missed = {s for s in (r.noted_old[0] | r.noted_old[1]) if s >= wrong_line}
    assert wrong_line == r.n_before - TC.SHORT and missed, "no fused older boundary slot above the misplaced line"
    for hw in ((32, 48), (33, 47)):
        case = TC.frame_case(*hw)
        culled, pieces = TC.culled_pieces(case)
        r = TC.restate_tiled(case.pm.clone(), *case.frames[0], case.prune_min, own=case.own, halo=case.halo, list_cap=case.list_cap)
        assert 1 <= culled < pieces and r.M > 100 and r.alloc_new > 5 and r.dropped_pairs > 0 and r.lists[0] and r.lists[1], (hw, culled, pieces, r.M)
    # the loop's clouds feed both slabs and both boundary layer sets
    pm = TC.TMap(np.zeros(0, dtype=np.int64), 4096)
    for xyz, nrm in TC.loop_clouds():
        r = TC.restate_tiled(pm, xyz, nrm, 2)
        assert r.M > 1000 and 1500 <= r.N <= 2500
    xs = pm.pos[:pm.n][pm.obs[:pm.n] > 0] // TC.PLANE
    assert (xs < TC.CUT - 3).any() and (xs >= TC.CUT + 3).any() and ((xs >= TC.CUT - 3) & (xs < TC.CUT)).any() and ((xs >= TC.CUT) & (xs < TC.CUT + 3)).any()


def test_export_restatements_match_the_oracle():
    pm = TC.export_map()
    om = _oracle_of(pm)
    rec, count, flag = TC.export_records(pm, 0, G, False, 4096)
    want = O.export_records(om)
    assert count == pm.n == want.shape[0] and flag == 0
    nan = np.isnan(rec[:, 3:].copy().view(F32)) & np.isnan(want[:, 3:].copy().view(F32))
    assert np.array_equal(rec[:, :3], want[:, :3]) and ((rec[:, 3:] == want[:, 3:]) | nan).all()
    plane_x = pm.pos[:pm.n] // TC.PLANE
    for x_lo, x_hi in TC.EXPORT_RANGES:
        n, body, flag = TC.export_halo_message(pm, x_lo, x_hi, 4096)
        a, b = max(x_lo, 0), min(x_hi, G)
        assert n == int(((plane_x >= a) & (plane_x < b)).sum()) and flag == 0
        if 0 <= x_lo and x_hi <= G:
            msg = O.export_halo_message(om, x_lo, x_hi, n + 3)
            assert msg[0, 0] == n and np.array_equal(msg[1:1 + n], body)
    assert TC.export_halo_message(pm, 8, 8, 10)[0] == 0 and TC.export_halo_message(pm, 9, 3, 10)[0] == 0
    # one record short: flag 6, the count clamped, the first records in slot order
    full, count, _ = TC.export_records(pm, 5, 11, False, 4096)
    cut, n_cut, flag = TC.export_records(pm, 5, 11, False, count - 1)
    assert flag == 6 and n_cut == count - 1 and np.array_equal(cut, full[:-1])


@pytest.mark.parametrize("name", ("mixed", "frac", "n65", "two", "n4097"))
def test_merge_restatements_match_the_oracle(name):
    """on the records the oracle accepts: ids inside the grid"""
    rs = TC.record_set(name)
    rec = np.concatenate([r for r, _ in rs.sources])
    rec = rec[(rec[:, 0] >= 0) & (rec[:, 0] < G ** 3)]
    pm, om = rs.pm.clone(), _oracle_of(rs.pm)
    flag, _ = TC.merge(pm, [TC.Source(rec)], assign=False)
    O.merge_records(om, rec)
    assert flag == 0
    _same_state(om, pm, name)
    pm, om = rs.pm.clone(), _oracle_of(rs.pm)
    TC.merge(pm, [TC.Source(rec, header=rec.shape[0])], assign=True)
    O.merge_halo_message(om, TC.message(rec, rec.shape[0] + 2))
    _same_state(om, pm, name + " (assign)")


def test_merge_edges_of_the_restatement():
    """what the oracle cannot take: out-of-range ids are skipped, the capacity cuts the allocation at the lowest ids (flag 1), a header is
    clamped to [0, rows], a w_r = 0 record allocates and leaves z alone"""
    rs = TC.record_set("mixed")
    pm = rs.pm.clone()
    z3 = pm.latent[3].copy()
    flag, s = TC.merge(pm, [TC.Source(*rs.sources[0])], assign=False)
    assert flag == 0 and 3 in s and np.array_equal(TC.bits(pm.latent[3]), TC.bits(z3)) and pm.indexer[G ** 3 - 1] >= 0
    assert (rs.w_r == 0).sum() > 3 and pm.n == rs.pm.n + 61
    rs = TC.record_set("overrun")
    pm = rs.pm.clone()
    flag, s = TC.merge(pm, [TC.Source(*rs.sources[0])], assign=False)
    new = np.unique([l for l in rs.sources[0][0][:, 0] if 0 <= l < G ** 3 and rs.pm.indexer[l] == -1])
    assert flag == 1 and pm.n == pm.capacity == 130 and (pm.indexer[new[:10]] >= 0).all() and (pm.indexer[new[10:]] == -1).all()
    for h, live in ((-3, 0), (0, 0), (TC.ROWS_HDR, TC.ROWS_HDR), (TC.ROWS_HDR + 5, TC.ROWS_HDR)):
        rs = TC.record_set(f"hdr{h}")
        assert TC.Source(*rs.sources[0]).live().shape[0] == live and rs.sources[0][0].shape[0] == TC.ROWS_HDR
    rs = TC.record_set("two")
    assert [r.shape[0] for r, _ in rs.sources] == [1, 70]
    for k in (1, 2, 63, 64, 65, 4097):
        assert TC.record_set(f"n{k}").sources[0][0].shape[0] == k


def test_delta_and_reset_restatements():
    case = TC.integrate_case("cut_mid")
    pm = case.pm.clone()
    r = TC.restate_tiled(pm, *case.frames[0], case.prune_min, own=case.own, halo=case.halo, list_cap=case.list_cap)
    (left, right), flag, note = TC.export_halo_delta(pm, case.list_cap, 4096, sides=(True, False))
    assert right is None and left["exact"] and left["header"] == (r.pending[0], r.pending[0], 1) and flag == 0
    assert list(note[:3]) == list(left["header"]) and (note[4:] == -1).all()
    assert not pm.lists[0] and len(pm.lists[1]) == r.pending[1]          # the side without a message keeps its list
    assert set(left["pool"][:, 0]) == {int(pm.pos[s]) for s in r.lists[0]}
    hdr, note = TC.halo_lists_reset(pm, (None, (77, 5, 1)))
    assert hdr == [None, (77, r.pending[1], 0)] and list(note[4:7]) == [77, r.pending[1], 0] and not pm.lists[1]
    (left, right), flag, _ = TC.export_halo_delta(pm, case.list_cap, 4096)
    assert left["n"] == right["n"] == 0 and flag == 0
    # records fewer than pending: flag 8
    pm.lists[0].extend([1, 2, 3])
    (left, _), flag, _ = TC.export_halo_delta(pm, case.list_cap, 2, sides=(True, False))
    assert flag == 8 and left["header"] == (2, 3, 1) and not left["exact"]


def test_float32_merge_stays_inside_the_bar():
    """The float32 restatement of the additive merge against the float64 weighted mean on every record set, under THE BAR of
    tiling_cases' docstring (C_INT = 3 + 2^-22 for integer weights, C_FRAC = 4 + 2^-20 otherwise): the reference passes on its own."""
    assert TC.C_INT == 3 + 2.0 ** -22 and TC.C_FRAC == 4 + 2.0 ** -20
    worst_all = 0.0
    for name in TC.RECORD_SETS:
        rs = TC.record_set(name)
        pm = rs.pm.clone()
        TC.merge(pm, [TC.Source(r, h) for r, h in rs.sources], assign=False)
        worst, count = TC.bar_ratio(rs.pm, pm, rs)
        print(f"  {name:8s} {count:7d} values  worst err/bar {worst:.3f}")
        assert worst <= 1.0, name
        worst_all = max(worst_all, worst)
    assert 0.1 < worst_all <= 1.0                                        # the bar is not slack by an order of magnitude
    # the bar does bite: one ulp more than the bar allows on a value is seen
    m, bar = TC.merge_bar(np.full((1, 29), 0.3, F32), [7.0], np.full((1, 29), -0.29, F32), [9.0])
    assert (bar < 4 * np.spacing(F32(0.3))).all() and (bar > 0).all()
