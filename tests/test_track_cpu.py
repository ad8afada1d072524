"""CPU: the stage-by-stage restatement of the tracker's SDF term (tests/track_ref.py) without a GPU — against the oracle's one-piece
restatement and the reference's goldens, on crafted rows that sit on the robust kernels' thresholds, and the conditions the generators of
tests/track_cases.py promise to tests/test_gpu_track_envelope.py (asserted here, so that the GPU test cannot hide a gap in its inputs)."""
import numpy as np
import pytest

from oracle import difusion_oracle as O
from tests import mlp_cases as C
from tests import track_cases as K
from tests import track_ref as T
from tests.test_oracle_track import REL_TOL, close, kernel_of, n_cases, track_inputs

F = np.float32
SUM_SLACK = 1e-10          # as tests/test_gpu_photo.py; two float64 summation orders of M terms differ by at most M * 2^-53 * S (M < 9e5)


@pytest.mark.parametrize("name", ["track_small", "track_c2"])
def test_stages_reproduce_the_oracle_and_the_goldens(name, oracle_net):
    """dense_rows + the oracle's decoder + flat_terms + sums_of_flat on the oracle map of the fixture: the valid set and M of
    O.compute_sdf_hg exactly, its H / g / e to the summation order; and the reference's numbers at the bound tests/test_oracle_track.py states."""
    g, cfg, frames, obs = track_inputs(name)
    om = O.OracleMap(oracle_net, cfg.bound_min, cfg.bound_max, cfg.voxel_size)
    for xyz, nrm in frames:
        om.integrate_keyframe(xyz.numpy(), nrm.numpy())
    obs = obs.numpy()
    for i in range(n_cases(g)):
        dR, dt = O.twist_exp(g[f"case{i}_xi"])
        kernel, k = kernel_of(g, i), float(g[f"case{i}_k"])
        out, S, valid = T.compute_sdf_hg(om, obs, g["last_R"], g["last_t"], dR, dt, kernel, k)
        H, gg, e, M = O.compute_sdf_hg(om, obs, g["last_R"], g["last_t"], dR, dt, kernel, k)
        assert int(out[43]) == M == int(valid.sum())
        # (the kernel holds the upper triangle, H[r][c] = sum (J[r] w) J[c] for r <= c, and mirrors it; the oracle's einsum also forms the lower one
        # as sum (J[c] w) J[r], whose float32 factor J[c] w is rounded differently: 2 x 2^-24 per term.  The 28 sums the kernel holds:)
        Hu = np.triu(H) + np.triu(H, 1).T
        T.within(out[:43], np.concatenate([Hu.reshape(-1), gg, [e]]), S, SUM_SLACK, f"{name} case {i} vs the oracle")
        T.within(out[:36], H.reshape(-1), S[:36], 2.0 ** -23 + SUM_SLACK, f"{name} case {i} vs the oracle's lower triangle")
        assert np.array_equal(out[:36].reshape(6, 6), out[:36].reshape(6, 6).T)
        out2, S2, _ = T.compute_sdf_hg(om, obs, g["last_R"], g["last_t"], dR, dt, kernel, k, no_grad=True)
        assert out2[42] == out[42] and out2[43] == out[43] and not out2[:42].any()
        # the reference's own numbers
        assert abs(M - int(g[f"case{i}_M"])) <= 3
        close(out[:36].reshape(6, 6), g[f"case{i}_H"], f"{name} case {i} H")
        close(out[36:42], g[f"case{i}_g"], f"{name} case {i} g", rel=REL_TOL * np.abs(g[f"case{i}_H"]).max() / np.abs(g[f"case{i}_g"]).max())
        assert abs(out[42] - float(g[f"case{i}_e"])) < REL_TOL * max(1.0, abs(float(g[f"case{i}_e"])))


def test_crafted_rows_sit_on_the_thresholds():
    """std a power of two, sdf = +-k std and its float32 neighbours: s is exactly +-k, one step inside, one step outside.  At |s| == k Huber
    gives w = 1 (its branch is `>`) and Tukey w = 0 ((1 - 1)^2: `<=` and `<` agree there, the value is continuous); a step inside Huber still 1
    and Tukey a positive weight; a step outside Huber k / |s| < 1 and Tukey 0."""
    sdf, std, s_want = K.crafted_rows()
    assert len(sdf) == 36 and (np.log2(std) % 1 == 0).all()
    for kernel, k in T.KERNELS[1:]:
        s, w, wf, J = T.flat_terms(sdf, std, None, None, None, None, kernel, k)
        assert J is None and np.array_equal(s, s_want) and np.array_equal(wf, (s * w).astype(F))
        ab, kk = np.abs(s), F(k)
        on, inside, outside = ab == kk, ab == np.nextafter(kk, F(0)), ab == np.nextafter(kk, F(np.inf))
        assert on.sum() == inside.sum() == outside.sum() == 6            # (the other kernel's k gives the remaining 18 rows)
        if kernel == "huber":
            assert (w[on] == 1).all() and (w[inside] == 1).all() and (w[outside] < 1).all() and (w[outside] == kk / ab[outside]).all()
            assert (w[ab < kk] == 1).all() and (w[ab > kk] < 1).all()
        else:
            assert (w[on] == 0).all() and (w[outside] == 0).all() and (w[inside] > 0).all() and (w[inside] < 1e-12).all()
            assert (w[ab > kk] == 0).all() and (w[ab < np.nextafter(kk, F(0))] > 1e-3).all()
    s, w, wf, _ = T.flat_terms(sdf, std, None, None, None, None, None, 0.0)
    assert (w == 1).all() and np.array_equal(wf, s)
    # rows with std == 0 are skipped, whatever else they hold
    sdf2, std2 = np.concatenate([sdf, [F(np.nan), F(1)]]), np.concatenate([std, [F(0), F(-0.0)]])
    assert np.array_equal(T.flat_terms(sdf2, std2, None, None, None, None, "huber", 0.75)[0], T.flat_terms(sdf, std, None, None, None, None, "huber", 0.75)[0])


def test_sums_of_flat_on_a_case_worked_by_hand():
    s, w = np.array([2.0, -1.0], dtype=F), np.array([0.5, 1.0], dtype=F)
    J = np.array([[1, 2, 3, 4, 5, 6], [-1, 0, 1, 0, 2, 0]], dtype=F)
    out, S = T.sums_of_flat(s, w, (s * w).astype(F), J)
    assert out[43] == 2 and out[42] == (2 * 1 + 1 * 1) / 2 and out[0] == (0.5 + 1) / 2 and out[1] == out[6] == (1.0 + 0) / 2
    assert out[36] == (1 * 1 + (-1) * (-1)) / 2 and out[40] == (5 * 1 + 2 * (-1)) / 2 and S[40] == (5 + 2) / 2
    out, S = T.sums_of_flat(s[:0], w[:0], s[:0], J[:0])
    assert not out.any() and not S.any()


# ---- what the generators promise --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shipped_map():
    return K.track_map(O.OracleNetworks(C.weight_set("shipped")), 0, 0.3)


def test_the_cloud_holds_every_class(shipped_map):
    om, n, _, _, (at, above) = shipped_map
    xyz, kind, axis, plane = K.cloud()
    assert 1800 <= len(xyz) <= 2600 and all((kind == k).sum() >= 9 for k in range(8))
    assert (np.diff(kind) != 0).mean() > 0.5                                      # shuffled
    bad = xyz[kind == K.NONFINITE]
    for c in range(3):
        assert np.isnan(bad[:, c]).sum() == 1 and (bad[:, c] == np.inf).sum() == 1 and (bad[:, c] == -np.inf).sum() == 1
    for Tc in (K.IDENTITY, K.pose()):
        valid, rows = T.dense_rows(om, xyz, Tc)
        assert rows.shape == (int(valid.sum()), 32) and valid.sum() >= 1000
        assert not valid[kind == K.NONFINITE].any() and not valid[(kind == K.FAR) & (np.abs(xyz).max(axis=1) > 4)].any()
    valid, _ = T.dense_rows(om, xyz, K.IDENTITY)
    assert not valid[kind == K.UNALLOCATED].any() and valid[kind == K.INSIDE].mean() > 0.9
    # the count gate: points inside the voxels whose count is exactly the threshold (not valid) and its successor (valid)
    _, xn = T.posed_xn(om, xyz[kind == K.INSIDE], K.IDENTITY)
    slot = om.indexer[om._linearize_id(np.ceil(xn).astype(np.int64) - 1)]
    v = valid[kind == K.INSIDE]
    assert np.isin(slot, at).sum() >= 5 and not v[np.isin(slot, at)].any()
    assert np.isin(slot, above).sum() >= 5 and v[np.isin(slot, above)].all()
    assert (om.voxel_obs_count[at] == F(16)).all() and (om.voxel_obs_count[above] == np.nextafter(F(16), F(17))).all()
    # the outer faces: xn = 0 is outside, its successor inside; xn = n inside, its successor outside
    o = kind == K.OUTER
    _, xn = T.posed_xn(om, xyz[o], K.IDENTITY)
    xa = xn[np.arange(o.sum()), axis[o]]
    assert (xa == 0).sum() >= 6 and (xa == 8).sum() >= 6 and ((xa > 8) & (xa < 8.00001)).sum() >= 6 and ((xa > 0) & (xa < 1e-5)).sum() >= 6
    assert not valid[o][(xa <= 0) | (xa > 8)].any()


def test_the_face_sets_straddle_their_faces(shipped_map):
    """Posed set: >= 100 points on each side of the face and >= 100 exactly on it, all within one voxel.  Identity set: exact-on-face points
    on >= 6 of the 9 planes of every axis among the +-4 float32 neighbours of bound_min + j * voxel_size.  >= 50 face points have a valid voxel
    on one side only: there the mask flips with the verdict."""
    om = shipped_map[0]
    xyz, kind, axis, plane = K.cloud()
    Tc = K.pose()
    p = kind == K.FACE_POSED
    side, lo, hi = K.face_report(om, xyz[p], axis[p], plane[p], Tc)
    assert (side == -1).sum() >= 100 and (side == 0).sum() >= 100 and (side == 1).sum() >= 100 and not (side == 2).any()
    one_sided = int((lo != hi).sum())
    i = kind == K.FACE_ID
    side_i, lo_i, hi_i = K.face_report(om, xyz[i], axis[i], plane[i], K.IDENTITY)
    assert not (side_i == 2).any()
    for a in range(3):
        exact = set(plane[i][(side_i == 0) & (axis[i] == a)].tolist())
        assert len(exact) >= 6, (a, sorted(exact))
        assert (side_i[axis[i] == a] == -1).sum() >= 9 and (side_i[axis[i] == a] == 1).sum() >= 9
    one_sided += int((lo_i != hi_i).sum())
    assert one_sided >= 50, one_sided
    # the verdict decides the mask there: below or on the face the lower voxel, above it the upper one
    valid, _ = T.dense_rows(om, xyz, Tc)
    assert np.array_equal(valid[p], np.where(side <= 0, lo, hi))
    valid, _ = T.dense_rows(om, xyz, K.IDENTITY)
    assert np.array_equal(valid[i], np.where(side_i <= 0, lo_i, hi_i))


def test_float64_cannot_be_the_oracle_of_the_valid_set(shipped_map):
    """The same float32 pose entries applied in float64: on the posed face set the voxel differs from the float32 rule's for more than 100
    of the 768 points (a set with every point exactly on its face: 323 of 768).  Hence track_ref restates the float32 order, exactly."""
    om = shipped_map[0]
    xyz, kind, _, _ = K.cloud()
    R, t = K.pose()
    p = xyz[kind == K.FACE_POSED]
    cur = p.astype(np.float64) @ R.astype(F).astype(np.float64).T + t.astype(F).astype(np.float64)
    xn64 = (cur - om.bound_min.astype(np.float64)) / float(F(om.voxel_size))
    differ = int((np.ceil(xn64) != np.ceil(T.posed_xn(om, p, (R, t))[1])).any(axis=1).sum())
    print(f"  float64 pose vs the float32 rule: another voxel for {differ} of {len(p)} face points")
    assert len(p) == 768 and differ >= 100


@pytest.mark.parametrize("ws", C.WEIGHT_SETS)
def test_reference_rows_are_usable(ws):
    """Per weight set, latent scale and pose: at most 1 % of the valid rows are set aside by Bundle.grad_keep (a hidden pre-activation on its
    kink), and no valid row of the float64 reference or the float32 oracle has std == 0 (the kernel's mark of a row that is not valid)."""
    b = C.bundle(ws)
    xyz = K.cloud()[0]
    for scale in K.SCALES:
        om = K.track_map(b.oracle, C.WEIGHT_SETS.index(ws), scale)[0]
        for Tc in (K.IDENTITY, K.pose()):
            _, rows = T.dense_rows(om, xyz, Tc)
            keep = b.grad_keep(rows)
            assert (~keep).mean() <= 0.01, f"{ws} N(0,{scale:g}): {(~keep).mean():.2%} of the rows on a ReLU kink"
            assert (b.ref.decoder(rows)[1] >= 0.05).all() and (b.oracle.decoder(rows)[1] >= F(0.05)).all()


def test_split_pose_composes_to_the_pose():
    (lR, lt), (dR, dt) = K.split_pose()
    R, t = K.pose()
    assert np.abs(lR @ dR - R).max() < 1e-15 and np.abs(lR @ dt + lt - t).max() < 1e-15 and np.abs(lR @ lR.T - np.eye(3)).max() < 1e-14


def test_reduce_rows_hold_dead_rows_and_the_crafted_ones():
    nc = len(K.crafted_rows()[0])
    for N in (0, 1, 255, 513, 262401):
        sdf, std, grad, obs = K.reduce_rows(N)
        assert sdf.shape == std.shape == (N,) and grad.shape == obs.shape == (N, 3)
        dead = std == 0
        assert np.isnan(sdf[dead]).all() and np.isnan(grad[dead]).all() and not np.isnan(sdf[~dead]).any() and not np.isnan(grad[~dead]).any()
        if N >= 255:
            assert 0.15 < dead.mean() < 0.4 and np.array_equal(sdf[:nc], K.crafted_rows()[0]) and np.array_equal(sdf[N - nc:], K.crafted_rows()[0])


def test_new_symbols_are_declared_and_bound():
    from di_fusion_amd import _lib
    from tests.test_abi import header_symbols
    for s in ("dif_test_sdf_hg_views", "dif_test_sdf_hg_reduce"):
        assert s in header_symbols() and s in _lib.SIGNATURES
