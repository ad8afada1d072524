"""The restatements of tests/extract_cases.py pinned on the CPU: the dirty list, batch and vbm on OracleMap.extract_prepare, the trilinear x2
on oracle.trilinear_upsample_align_corners and the golden `tri_up`, the log on oracle.mesh_cache_update at every limit the GPU tests run."""
import numpy as np
import pytest

from oracle import difusion_oracle as O
from tests import extract_cases as EC
from tests import integrate_cases as IC
from tests.conftest import GOLDEN

F32 = np.float32
MAX_STD = 0.15


def oracle_map(pm, net, dirty=None):
    """An OracleMap holding the planted map `pm` (its dirty flags, or the slots `dirty`, as updated_vec_id)"""
    G = pm.grid
    lo = np.asarray(pm.bound_min, dtype=np.float64)
    om = O.OracleMap(net, lo, lo + G * pm.voxel_size, pm.voxel_size)
    assert om.n_xyz == [G, G, G]
    n = pm.n
    om.n_occupied, om.indexer = n, pm.indexer.copy()
    om.latent_vecs, om.latent_vecs_pos, om.voxel_obs_count = pm.latent[:n].copy(), pm.pos[:n].copy(), pm.obs[:n].copy()
    om.voxel_optimized = np.zeros(n, dtype=bool)
    om.updated_vec_id = np.nonzero(pm.dirty[:n])[0] if dirty is None else np.asarray(dirty, dtype=np.int64)
    return om


def _check_prepare(pm, net, **kw):
    om = oracle_map(pm, net)
    a = om.extract_prepare(1, fast=False, no_cache=kw.get("no_cache", False))
    p = EC.prepare(pm, **kw)
    assert not pm.dirty.any() and p.overflow == 0 and p.deferred == 0
    assert np.array_equal(p.valid_blocks, a["valid_blocks"]) and p.K == a["valid_blocks"].size
    assert np.array_equal(p.occ_slot, a["occupied_vec_id"]) and p.B == a["occupied_vec_id"].size
    m = a["vec_batch_mapping"]
    assert np.array_equal(p.vbm[:m.size], m) and (p.vbm[m.size:] == -1).all()
    return p


@pytest.fixture(scope="module")
def case():
    return EC.planted(1024)


def test_the_planted_map_holds_what_it_is_for(case):
    pm, G = case.pm, EC.GRID
    n = pm.n
    assert 280 <= n <= 400 and {255, 256, 257, n - 1} <= set(case.dirty0.tolist())
    p = EC.prepare(pm.clone())
    dirty_lin = pm.pos[case.dirty0]
    # the dirty voxel at the threshold is listed and is not in the batch; a dirty voxel without any allocated neighbour; all eight corners
    at = EC._lin(EC.AT_TH)
    assert at in p.valid_blocks and at not in p.batch and pm.obs[pm.indexer[at]] == EC.IGNORE_TH
    assert (pm.indexer[np.setdiff1d(IC.neighbours7([EC._lin(EC.LONELY)], G), [EC._lin(EC.LONELY)])] == -1).all()
    assert set(EC._lin(v) for v in EC.CORNERS) <= set(dirty_lin.tolist())
    # counts at the threshold and at its successor among the neighbours of dirty voxels: the first outside the batch, the second inside
    nb = IC.neighbours7(dirty_lin, G)
    nb = nb[pm.indexer[nb] >= 0]
    w = pm.obs[pm.indexer[nb]]
    assert (w == EC.IGNORE_TH).sum() >= 3 and (w == EC.TH_NEXT).sum() >= 3
    assert not np.isin(nb[w == EC.IGNORE_TH], p.batch).any() and np.isin(nb[w == EC.TH_NEXT], p.batch).all()
    # what a neighbour without its clamp would pull in: allocated, confident, and outside the batch
    assert case.witnesses.size >= 6 and (pm.indexer[case.witnesses] >= 0).all() and not np.isin(case.witnesses, p.batch).any()
    # bits of one bitmap word, of two; neighbours shared by two dirty voxels
    words = dirty_lin // 32
    assert np.unique(words).size < words.size and {26, 27} <= set(words.tolist())
    each = np.concatenate([IC.neighbours7([v], G) for v in dirty_lin])
    assert np.unique(each).size < each.size
    assert case.clone.sum() >= n // 3 and np.unique(pm.latent[:n][case.clone], axis=0).shape[0] == 3


def test_prepare_against_the_oracle(case, oracle_net):
    p0 = _check_prepare(case.pm.clone(), oracle_net)
    assert p0.K == case.dirty0.size and p0.B > p0.K
    pm = case.pm.clone()
    pm.dirty[:] = 0
    EC.second_frame(case, pm)
    p1 = _check_prepare(pm, oracle_net)
    assert p1.K == case.dirty1.size and not np.isin(case.unconfident1, p1.occ_slot).any()
    pn = _check_prepare(case.pm.clone(), oracle_net, no_cache=True)
    assert pn.K == case.pm.n and pn.B == int((case.pm.obs[:case.pm.n] > EC.IGNORE_TH).sum())
    g = EC.grid64()
    p64 = _check_prepare(g.pm.clone(), oracle_net)
    assert set((p64.batch // 32 // 256).tolist()) >= {0, 1}              # two grid_tot blocks of the 64^3 bitmap


def test_prepare_limits_and_deferral(case):
    full = EC.prepare(case.pm.clone())
    K, B, n = full.K, full.B, case.pm.n
    p = EC.prepare(case.pm.clone(), max_voxels=K - 1)
    assert p.overflow in (2, 3) and p.K == K - 1 and np.array_equal(p.valid_blocks, full.valid_blocks[:K - 1])
    p = EC.prepare(case.pm.clone(), max_voxels=B - 1)
    assert p.overflow == 3 and p.K == K and p.B == B - 1 and np.array_equal(p.occ_slot, full.occ_slot[:B - 1])
    need = min(7 * K, n)
    pm = case.pm.clone()
    p = EC.prepare(pm, max_voxels=need - 1, block_totals=True)
    assert p.deferred == need and p.K == 0 and np.array_equal(pm.dirty, case.pm.dirty)
    p = EC.prepare(case.pm.clone(), max_voxels=need, block_totals=True)
    assert p.deferred == 0 and p.K == K and p.B == B


def test_tiled_prepare_follows_the_untiled_rule(case):
    """own_x = [4, 11): the dirty corners, faces and the row at x = 3 are halo voxels — not listed, their neighbourhoods in the batch"""
    own = (4, 11)
    whole = EC.prepare(case.pm.clone())
    pm = case.pm.clone()
    tiled = EC.prepare(pm, own=own)
    x = whole.valid_blocks // (EC.GRID * EC.GRID)
    inside = (x >= own[0]) & (x < own[1])
    assert 0 < inside.sum() < inside.size and not pm.dirty.any()
    assert np.array_equal(tiled.valid_blocks, whole.valid_blocks[inside])
    assert np.array_equal(tiled.batch, whole.batch) and np.array_equal(tiled.vbm, whole.vbm)


def test_fma32_rounds_once():
    """(2^23 + 1) * 1.5 = 12582913.5 is the midpoint of two float32; -+ 2^-60 puts the sum just below / above it.  float64 drops the dust and a
    second rounding then sees a tie (to even: 12582914 either way), which is what oracle._fma32 does; one rounding does not."""
    a, b, dust = F32(2.0 ** 23 + 1), F32(1.5), F32(2.0 ** -60)
    assert EC.fma32(a, b, -dust) == F32(12582913.0) and EC.fma32(a, b, dust) == F32(12582914.0)
    assert O._fma32(np.array([a]), np.array([b]), np.array([-dust]))[0] == F32(12582914.0)
    assert EC.fma32(-a, b, dust) == F32(-12582913.0) and EC.fma32(-a, b, -dust) == F32(-12582914.0)
    assert EC.fma32(a, b, F32(0)) == F32(12582914.0)                      # the tie itself: to even
    assert EC.fma32(F32(2.0 ** 23 + 2), b, F32(0.5)) == F32(12582916.0)  # 12582915.5: a tie again, to even, upward this time
    # wherever float64 adds exactly the two agree
    r = np.random.default_rng(1)
    x, y, z = (r.standard_normal(4096).astype(F32) for _ in range(3))
    exact = (x.astype(np.float64) * y + z) - z == x.astype(np.float64) * y
    assert exact.any() and np.array_equal(EC.fma32(x, y, z)[exact], O._fma32(x, y, z)[exact])


def test_upsample2_against_the_oracle_and_the_golden():
    g = np.load(GOLDEN / "networks.npz")
    low, want = g["tri_low"][:, 0], g["tri_up"][:, 0]
    assert np.array_equal(EC.upsample2(low, want.shape[-1]).view(np.uint32), np.ascontiguousarray(want).view(np.uint32))
    r = np.random.default_rng(3)
    for l in (1, 2, 3, 4, 8):
        x = (r.standard_normal((7, l, l, l)) * 0.3).astype(F32)
        assert np.array_equal(EC.upsample2(x, 2 * l).view(np.uint32), O.trilinear_upsample_align_corners(x, 2 * l).view(np.uint32)), l


# ---- the log -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def frames(case, oracle_net):
    """the untruncated canonical triangle lists of the two frames, by the oracle's decoder and the C marching cubes"""
    out = []
    pm = case.pm.clone()
    for f in range(2):
        if f == 1:
            EC.second_frame(case, pm)
        om = oracle_map(pm, oracle_net)
        tri, tid, tstd = om.extract_mesh(4, int(4e6), MAX_STD, fast=True)
        pm.dirty[:] = 0
        out.append((tri, tid, tstd))
    return out


def test_log_rule_at_every_limit(case, frames):
    pm = case.pm
    (tri0, tid0, std0), (tri1, tid1, std1) = frames
    v0, f0, c0 = EC.voxel_runs(tid0)
    v1, f1, c1 = EC.voxel_runs(tid1)
    assert tid0.size > 100 and v0.size >= 10 and tid1.size > 10
    # frame 1: batches replaced, and voxels that were meshed in frame 0 and yield nothing now (their stale batches are kept)
    again = pm.pos[case.dirty1]
    assert np.isin(v1, v0).any() and (np.isin(again, v0) & ~np.isin(again, v1)).any()
    n_whole = 0
    for frame, (tri, tid, tstd) in enumerate(frames):
        for mt, cc in EC.limit_cases(tid0.size, 0 if frame == 0 else tid0.size, tid.size, EC.voxel_runs(tid)):
            log = EC.Log(pm.capacity, cc if frame == 0 else max(cc, tid0.size))
            if frame == 1:
                EC.log_update(log, pm.indexer, tri0, tid0, std0, 10 ** 6)
            prev = log.live()
            prev_n, prev_s = log.tri_n.copy(), log.tri_start.copy()
            r = EC.log_update(log, pm.indexer, tri, tid, tstd, mt, out_capacity=7)
            n = r.n_new
            assert n == min(tid.size, mt, log.cc - log.kept) and (r.overflow == 5) == (log.kept + min(tid.size, mt) > log.cc)
            want = O.mesh_cache_update(prev if frame == 1 else None, tri[:n], tid[:n], tstd[:n])
            got = log.live()
            for a, b in zip(got, want):
                assert a.shape == b.shape and np.array_equal(a.view(np.uint32 if a.dtype == F32 else np.int64), b.view(np.uint32 if b.dtype == F32 else np.int64))
            # the bookkeeping names exactly the live batches
            for slot in np.nonzero(log.tri_n)[0]:
                s, k = log.tri_start[slot], log.tri_n[slot]
                assert log.alive[s:s + k].all() and (log.id[s:s + k] == pm.pos[slot]).all()
            assert log.tri_n.sum() == log.alive[:log.T].sum() == log.T - log.dead
            cut = pm.indexer[r.whole_cut]
            assert np.array_equal(log.tri_n[cut], prev_n[cut]) and np.array_equal(log.tri_start[cut], prev_s[cut])
            assert r.out[1].size == min(7, n) and r.pending[:3] == (1 if n else 0, log.kept, min(7, n))
            n_whole += int((prev_n[cut] > 0).sum()) if frame == 1 else 0
            if frame == 1 and (prev_n[cut] > 0).any():
                # what the kernels did before: the cut-off voxel's old batch died with it -> a hole the reference does not have
                old = EC.Log(pm.capacity, log.cc)
                EC.log_update(old, pm.indexer, tri0, tid0, std0, 10 ** 6)
                EC.log_update(old, pm.indexer, tri, tid, tstd, mt, cut_keeps=False)
                assert old.live()[1].size < got[1].size
    assert n_whole > 0, "no limit case cuts off a whole voxel that holds a batch of the first frame"
