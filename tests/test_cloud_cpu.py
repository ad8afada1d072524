"""Pins tests/cloud_cases.py, the reference the GPU envelope tests of the point-cloud ops are held to, on the CPU: the exhaustive search
against the oracle's two independent ones bit for bit, the float32 restatement of the normals against the oracle's, the float64 statement
on hand cases, and the properties that the constructed clouds (colliding cells, d2 == r^2 ties, cell faces, the accept limit) claim."""
import numpy as np
import pytest

from tests import cloud_cases as CC

F32, F64 = np.float32, np.float64


def _ulps(a, b):
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return np.abs(a.astype(F64) - b.astype(F64)) / np.spacing(np.maximum(np.abs(a), np.abs(b))).astype(F64)


def _special_clouds():
    pc_tie, r_tie = CC.tie_lattice()
    out = [("tie lattice", pc_tie, r_tie), ("collision", CC.collision_cloud()[0], CC.R_KNN), ("faces 0", CC.face_cloud((0, 0, 0)), CC.R_KNN),
           ("faces 2^15", CC.face_cloud((1 << 15, -(1 << 15), 1 << 15)), CC.R_KNN), ("clusters", CC.count_clusters()[0], CC.R_KNN)]
    out += [(f"limit {s:+d} stride {st}", CC.limit_cloud(s, st)[0], CC.R_KNN) for s, st in ((1, 3), (-1, 4))]
    out += [(f"degenerate {k}", v[0], v[2]) for k, v in CC.degenerate_clouds().items()]
    return out


@pytest.mark.parametrize("kind", CC.KINDS)
def test_knn_ref_equals_both_oracle_searches_on_the_sweep(kind):
    from oracle import difusion_oracle as O
    for name, pc, knn in CC.sweep(kind):
        oi, od = O.knn_bruteforce(pc, 32, CC.R_KNN)
        assert np.array_equal(knn[0], oi) and np.array_equal(knn[1], od), name
        ni, nd = O.knn_bruteforce_numpy(pc, 32, CC.R_KNN)
        assert np.array_equal(knn[0], ni) and np.array_equal(knn[1], nd), name
        for k, r in ((1, CC.R_KNN), (9, CC.R_KNN), (16, CC.R_OUT)):                 # a cut list is the list of the smaller k and radius
            ci, cd = CC.cut(knn, k, r)
            oi, od = O.knn_bruteforce(pc, k, r)
            assert np.array_equal(ci, oi) and np.array_equal(cd, od), (name, k, r)
        assert np.array_equal(CC.outlier_ref(pc, 16, CC.R_OUT, knn=knn), O.remove_radius_outlier(pc, 16, CC.R_OUT)), name


def test_knn_ref_equals_both_oracle_searches_on_the_special_clouds():
    """The oracle knows no accept limit: rows the product refuses are made NaN for it, which is how it states `nobody's neighbour`."""
    from oracle import difusion_oracle as O
    for name, pc, r in _special_clouds():
        acc = CC.accepted(pc, r, "knn")
        masked = pc.copy()
        masked[~acc, :3] = np.nan
        for k in (1, 8, 17, 32):
            idx, dist = CC.knn_ref(pc, k, r)
            oi, od = O.knn_bruteforce(masked, k, r)
            assert np.array_equal(idx, oi) and np.array_equal(dist, od), (name, k)
            ni, nd = O.knn_bruteforce_numpy(masked, k, r)
            assert np.array_equal(idx, ni) and np.array_equal(dist, nd), (name, k)
            assert (idx[~acc] == -1).all() and np.isinf(dist[~acc]).all()
            assert not np.isin(idx, np.nonzero(~acc)[0]).any()
    for n in (1, 2, 255, 257):
        pc = np.random.default_rng(n).uniform(-0.1, 0.1, (n, 3)).astype(F32)
        idx, dist = CC.knn_ref(pc, 32, 0.1)
        oi, od = O.knn_bruteforce(pc, 32, 0.1)
        assert np.array_equal(idx, oi) and np.array_equal(dist, od), n


def test_normals_ref32_equals_the_oracle():
    """NaN pattern identical, rows that go through the guard of the normalisation included (cross products whose squared length is below
    2^-100: exactly collinear neighbourhoods); values to 4 ulp on rows with a gap ratio of at least GAP_MIN (both take acos from the
    same libm; the oracle clips its argument first)."""
    from oracle import difusion_oracle as O
    worst, guarded = 0.0, 0
    for kind in CC.KINDS:
        for name, pc, knn in CC.sweep(kind)[:5]:
            for cam in ((0.0, 0.0, 0.0), (0.3, -0.2, 4.0)):
                ref = CC.normals_ref64(pc, 16, CC.R_KNN, cam, CC.cut(knn, 16, CC.R_KNN))
                want = O.estimate_normals(pc, 16, CC.R_KNN, cam)
                assert np.array_equal(np.isnan(ref["n32"]), np.isnan(want)), name
                guarded += int(((ref["len2"] < CC.LEN2_MIN) & (ref["cnt"] >= 5)).sum())
                ok = ref["gap"] >= CC.GAP_MIN
                if ok.any():
                    worst = max(worst, float(_ulps(ref["n32"][ok], want[ok]).max()))
    print(f"normals_ref32 against the oracle: {worst:.2f} ulp at worst; {guarded} rows went through the guard (all of kind `line`)")
    assert worst <= 4 and guarded > 0


def _rot(axis, angle):
    axis = np.asarray(axis, F64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def test_normals_ref64_on_hand_cases():
    g = np.random.default_rng(2)
    flat = np.concatenate([g.uniform(-0.2, 0.2, (400, 2)), np.full((400, 1), 0.5)], 1)
    cam = np.array([0.0, 0.0, 3.0])
    ref = CC.normals_ref64(flat.astype(F32), 16, 0.1, cam)
    ok = ~np.isnan(ref["n64"][:, 0])
    assert ok.mean() > 0.9 and np.abs(ref["n64"][ok] - np.array([0, 0, 1.0])).max() < 1e-12          # towards the camera: +z
    assert np.abs(CC.normals_ref64(flat.astype(F32), 16, 0.1, -cam)["n64"][ok] - np.array([0, 0, -1.0])).max() < 1e-12
    assert np.abs(ref["evals"][ok, 0]).max() < 1e-15 and (ref["gap"][ok] > 0.05).all()
    # a tilted plane gives its normal: float32 coordinates are off the plane by half an ulp of 0.5, the lever arm is the neighbourhood's
    # extent (> 0.02), so the angle is below 3e-8 / 0.02
    R = _rot([1.0, 2.0, -0.5], 0.7)
    tilt32 = (flat @ R.T).astype(F32)
    rt = CC.normals_ref64(tilt32, 16, 0.1, R @ cam)
    assert np.array_equal(np.isnan(rt["n64"][:, 0]), ~ok)
    assert np.abs(rt["n64"][ok] - R[:, 2]).max() < 2e-5
    # rotation and translation: a generic cloud whose coordinates stay exact under the motion (multiples of 2^-10, a signed permutation of
    # the axes, a shift by multiples of 2^-10) keeps its neighbour lists and turns its normals with it
    box = np.round(g.uniform(-0.2, 0.2, (500, 3)) * 1024) / 1024
    Pm = np.array([[0, 0, 1.0], [-1.0, 0, 0], [0, -1.0, 0]])
    shift = np.array([3.0, -1.5, 0.25])
    a = CC.normals_ref64(box.astype(F32), 16, 0.1, cam)
    b = CC.normals_ref64((box @ Pm.T + shift).astype(F32), 16, 0.1, Pm @ cam + shift)
    ok = ~np.isnan(a["n64"][:, 0]) & (a["gap"] > 1e-3)
    assert ok.sum() > 400 and np.array_equal(np.isnan(a["n64"]), np.isnan(b["n64"]))
    assert np.abs(a["n64"][ok] @ Pm.T - b["n64"][ok]).max() < 1e-9
    assert np.allclose(a["evals"][ok], b["evals"][ok], rtol=0, atol=1e-15)


def test_constructed_clouds_have_what_they_claim():
    # d2 == r^2 bit for bit, and the strict cut drops exactly those
    pc, r = CC.tie_lattice()
    idx, dist = CC.knn_ref(pc, 32, r)
    d = pc[:, None, :] - pc[None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    r2 = F32(r) * F32(r)
    assert (d2.view(np.int32) == r2.view(np.int32)).sum() >= 6 * 27
    centre = int(np.nonzero((pc == 0).all(1))[0][0])
    assert (d2[centre] < r2).sum() == 27 and (d2[centre] == r2).sum() == 6
    assert (idx[centre, :27] >= 0).all() and (idx[centre, 27:] == -1).all() and np.isinf(dist[centre, 27:]).all()
    assert CC.outlier_ref(pc, 27, r)[centre] and not CC.outlier_ref(pc, 28, r)[centre]
    # colliding cells
    pc, info = CC.collision_cloud()
    print("collision cloud:", info)
    assert len(pc) <= 2048 and info["T"] == 4096 and info["colliding"] >= 64 and info["empty_probes"] >= 1
    h = [CC.home_slot((8 * b[0], 8 * b[1], 8 * b[2]), info["T"])[0] >> 9 for b in info["blocks"]]
    assert len(set(h)) == 1 and len(info["blocks"]) == 3
    # home_slot: the cells of one block fill 512 different slots of one window; the second hash leaves the window for most cells
    slots = {CC.home_slot((x, y, z), 4096)[0] for x in range(8) for y in range(8) for z in range(8)}
    assert len(slots) == 512 and len({s >> 9 for s in slots}) == 1
    assert all(0 <= v < 8192 for c in ((0, 0, 0), (-5, 7, 123456), (CC.LIMIT, -CC.LIMIT, 1)) for v in CC.home_slot(c, 8192))
    # cell faces: planted values are there, both zeros included, and points sit exactly on computed edges
    c, _ = CC.cell_size(CC.R_KNN, 2)
    for cells in ((0, 0, 0), (1 << 15, -(1 << 15), 1 << 15)):
        f = CC.face_cloud(cells)
        assert CC.accepted(f, CC.R_KNN).all()
        for a in range(3):
            assert (f[:, a] == F32(cells[a] + 1) * c).any() and (f[:, a] == F32(cells[a]) * c).any()
    z = CC.face_cloud((0, 0, 0))
    assert (np.signbit(z) & (z == 0)).any() and (~np.signbit(z) & (z == 0)).any()
    # the accept limit: inside cluster accepted, outside cluster and the non-finite rows not, under both ops' cell sizes
    for s, st in ((1, 3), (-1, 4)):
        pc, first_bad = CC.limit_cloud(s, st)
        acc = CC.accepted(pc, CC.R_KNN, "knn")
        assert acc[:first_bad].all() and not acc[first_bad:].any() and len(pc) - first_bad == 32
        assert np.array_equal(acc, CC.accepted(pc, CC.R_OUT, "outlier"))
        _, cell = CC.cells_of(pc[200:first_bad], CC.R_KNN, 2)
        assert (np.abs(cell[:, 0]) >= CC.LIMIT - 3).all()
        assert st == 3 or np.isnan(pc[:, 3]).all()
    # 4, 5, 6 neighbours
    pc, cnt = CC.count_clusters()
    ref = CC.normals_ref64(pc, 16, CC.R_KNN, (0, 0, 0))
    assert np.array_equal(ref["cnt"], cnt) and np.array_equal(np.isnan(ref["n64"][:, 0]), cnt < 5) and set(cnt) == {4, 5, 6}
    assert np.array_equal(np.isnan(ref["n32"][:, 0]), cnt < 5)


def test_degenerate_neighbourhoods_of_the_restatement():
    """What the float32 closed form makes of them: all-NaN rows or unit vectors, nothing else."""
    for name, (pc, k, r) in CC.degenerate_clouds().items():
        ref = CC.normals_ref64(pc, k, r, (0.1, 0.2, 3.0))
        n = ref["n32"]
        nan = np.isnan(n)
        assert (nan.all(1) | ~nan.any(1)).all() and not np.isinf(n).any(), name
        fin = ~nan[:, 0]
        assert (np.abs(np.linalg.norm(n[fin].astype(F64), axis=1) - 1) <= CC.UNIT_ULPS * CC.ULP1).all(), name
        print(f"degenerate {name}: {int(fin.sum())} of {len(n)} rows finite in the restatement, {int((ref['cnt'] >= 5).sum())} with 5 neighbours")
    iso = CC.degenerate_clouds()["isotropic"]
    ref = CC.normals_ref64(*iso[:1], iso[1], iso[2], (0, 0, 0))
    centres = np.arange(0, 81, 9)
    assert (ref["cnt"][centres] == 8).all() and (ref["gap"][centres] < 1e-12).all()


def test_gap_threshold_and_e_ref():
    """The distribution of e_ref against the gap ratio on the non-degenerate kinds, every offset, printed per decade of the gap ratio and
    per offset (e_ref is the yardstick of the GPU bar: far from the origin the float32 mean and covariance lose digits and it grows from
    1e-6 to 1e-1).  Asserted: the share of rows under GAP_MIN is below 1 %, and the restatement has a finite normal on every row at or
    above GAP_MIN."""
    rows = below = 0
    table = {}
    for kind in CC.NON_DEGENERATE:
        for name, pc, knn in CC.sweep(kind):
            ref = CC.normals_ref64(pc, 16, CC.R_KNN, (0.0, 0.0, 0.0), CC.cut(knn, 16, CC.R_KNN))
            ok = ~np.isnan(ref["n64"][:, 0])
            rows += int(ok.sum())
            below += int((ref["gap"][ok] < CC.GAP_MIN).sum())
            judged = ok & (ref["gap"] >= CC.GAP_MIN)
            assert np.isfinite(ref["e_ref"][judged]).all(), name                      # on judged rows the restatement has a number
            dec = np.floor(np.log10(ref["gap"][judged])).astype(int)
            off = name.split()[1].lstrip("+-").rstrip("xyz")
            for d in np.unique(dec):
                e = ref["e_ref"][judged][dec == d]
                t = table.setdefault((off, int(d)), [0, 0.0])
                t[0] += len(e); t[1] = max(t[1], float(e.max()))
    print(f"rows with 5+ neighbours: {rows}; gap ratio below {CC.GAP_MIN}: {below} ({100.0 * below / rows:.3f} %)")
    for (off, d), (cnt, worst) in sorted(table.items()):
        print(f"  offset {off:>5} cells, gap ratio in [1e{d}, 1e{d + 1}): {cnt:6d} rows, worst e_ref {worst:.3g}")
    assert rows > 30000 and below <= 0.01 * rows
