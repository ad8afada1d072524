"""tests/frontend_cases.py pinned on the CPU: the float64 statement of the depth front end and of point_box_filter against answers that
can be written out by hand, the float32 restatement against the statement and against the oracle, the inputs' decision margins, the
constant K_FE of the GPU bar, and the box grid's input contract (tools/pbf_grid_check.cpp under the host sanitizers)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import frontend_cases as FC
from tests.conftest import GOLDEN, ROOT

F32, F64 = np.float32, np.float64


# ---- both statements, as (filter, unproject, normal_weight, eps): the hand cases hold for the float64 one to float64 rounding and for the
# float32 one to float32 rounding
IMPLS = {"float64": (FC.filter64, FC.unproject64, FC.normal_weight64, 2.0 ** -52), "float32": (FC.filter32, FC.unproject32, FC.normal_weight32, 2.0 ** -23)}


@pytest.fixture(params=list(IMPLS))
def impl(request):
    return IMPLS[request.param]


def test_l_squared_left_to_right_equals_precomputed():
    """The reference writes `(abs(i) + abs(j)) * MEAN_SIGMA_L * MEAN_SIGMA_L` (left to right), the kernel `k * (L * L)`: the same float32 for k = 0..4"""
    L = F32(1.2232)
    for k in range(5):
        assert (F32(k) * L) * L == F32(k) * (L * L), k


def test_threshold_value_is_below_the_double_constant():
    assert float(FC.TH32) < 1e-6 <= float(FC.UPPER) and float(np.nextafter(FC.TH32, F32(0))) < 1e-6
    assert bool(FC._lt(FC.TH32)) and not bool(FC._lt(FC.UPPER))


def test_plane_normal_is_the_planes_normal(impl):
    """A perspective image of the plane n . p = d: the four neighbours of a pixel lie on the plane, so the cross product of their
    differences is parallel to n exactly; the sign: cross(p(v+1) - p(v-1), p(u+1) - p(u-1)) points TOWARDS the camera (n_z < 0) on a
    surface that faces it."""
    _, unproject, normal_weight, eps = impl
    H, W = 12, 15
    K = FC.Intr(H, W)
    z = FC.plane_depth(H, W, K, FC.PLANE_N, 1.2 * FC.PLANE_N[2])
    if eps > 1e-10:
        z = z.astype(F32)
    nw = normal_weight(unproject(z, K))
    inner = np.zeros((H, W), bool); inner[1:-1, 1:-1] = True
    assert np.array_equal(nw["valid"], inner)
    err = np.abs(nw["normal"][inner].astype(F64) + FC.PLANE_N[None]).max()
    # a rounding of relative size eps in a depth of ~1.2 m moves a difference of 2 z / fx = 4.6e-3 m by 1.2 eps: ~300 eps on the direction, times the few operations behind it
    print(f"plane normal: worst error {err:.3g}")
    assert err < 4096 * eps
    assert (nw["normal"][inner][:, 2] < 0).all()


def test_constant_depth_is_a_fixed_point_of_the_filter(impl):
    filt, _, _, eps = impl
    for z in (0.5, 1.0, 3.75):
        d = np.full((9, 11), z, F32)
        out = filt(d)
        assert np.abs(out.astype(F64) - z).max() <= 64 * eps * z          # 25 products and sums, one division


def test_zero_and_negative_neighbours_carry_no_weight(impl):
    """A 2 mm centre (where sigma_z is small enough that a neighbour at 0 would weigh exp(-0.5 * 0.76) against it) among zeros, negatives
    and values below the threshold: the filtered centre is the centre."""
    filt, _, _, eps = impl
    d = np.zeros((5, 5), F32)
    d[0, :] = -1.0; d[1, :] = FC.TH32; d[3, :] = F32(1e-40); d[4, 2] = np.nextafter(FC.TH32, F32(0))
    d[2, 2] = 0.002
    assert float(filt(d)[2, 2]) == float(F32(0.002))
    d[2, 1] = 0.004                                     # one neighbour that counts: now the centre moves towards it
    out = float(filt(d)[2, 2])
    s = 1.0 / (F64(FC.C_A) + F64(FC.C_B) * (F64(F32(0.002)) - F64(FC.C_Z0)) ** 2 + F64(FC.C_C) / np.sqrt(F64(F32(0.002))) * 0.25)
    w = np.exp(-0.5 * (F64(FC.C_L) ** 2 + (F64(F32(0.004)) - F64(F32(0.002))) ** 2 * s * s))
    want = (F64(F32(0.002)) + w * F64(F32(0.004))) / (1.0 + w)
    assert 0.002 < out < 0.004 and abs(out - want) < 16 * eps * want
    d[2, 2] = FC.TH32                                   # a centre below the threshold is written as 0
    assert float(filt(d)[2, 2]) == 0.0


def test_a_depth_step_does_not_leak(impl):
    """Across a 1 m step the other side's weight is exp(-0.5 * (1 m * sigma_z)^2) = 0 (sigma_z > 300 / m): every filtered pixel stays
    inside the spread of its own side's window values."""
    filt, _, _, eps = impl
    g = np.random.default_rng(5)
    d = np.where(np.arange(14)[None, :] < 7, 1.0, 2.0) + g.uniform(0, 0.004, (11, 14))
    d = d.astype(F32)
    out = filt(d).astype(F64)
    for v in range(2, 9):
        for u in range(2, 12):
            win = d[v - 2:v + 3, u - 2:u + 3].astype(F64)
            own = win[np.abs(win - d[v, u]) < 0.5]
            assert own.min() - 8 * eps * 2 <= out[v, u] <= own.max() + 8 * eps * 2, (v, u)
    assert np.abs(out - d)[2:9, 2:12].max() > 1e-5      # and the filter did something


def test_weight_by_hand(impl):
    """theta = 0 (a mirrored point map, normal (0, 0, 1)): the angle term vanishes, weight = 1 / (0.0012f + 0.0019f (z - 0.4f)^2).  And a
    fronto-parallel image, where the normal is (0, 0, -1) and theta = pi."""
    _, unproject, normal_weight, eps = impl
    z, s = 1.0, 0.01
    v, u = np.meshgrid(np.arange(3.0), np.arange(3.0), indexing="ij")
    pc = np.stack([-u * s, v * s, np.full_like(u, z)], -1)
    nw = normal_weight(pc if eps < 1e-10 else pc.astype(F32))
    want = 1.0 / (F64(FC.C_A) + F64(FC.C_B) * (z - F64(FC.C_Z0)) ** 2)
    assert nw["valid"][1, 1] and nw["valid"].sum() == 1
    assert np.allclose(nw["normal"][1, 1], [0, 0, 1], atol=4 * eps)
    assert abs(float(nw["weight"][1, 1]) - want) < 16 * eps * want and abs(want - 530.785) < 0.01
    K = FC.Intr(3, 3)
    nw = normal_weight(unproject(np.full((3, 3), z, F64 if eps < 1e-10 else F32), K))
    td = np.pi / (F64(FC.C_HALF) * F64(FC.C_PI) - np.pi)
    want = 1.0 / (F64(FC.C_A) + F64(FC.C_B) * (z - F64(FC.C_Z0)) ** 2 + F64(FC.C_C) / 1.0 * td * td)
    assert np.allclose(nw["normal"][1, 1], [0, 0, -1], atol=4 * eps)
    assert abs(float(nw["weight"][1, 1]) - want) < 64 * eps * want          # acos near -1 is steep: sqrt(eps)-sized theta errors stay below this because n_z is exactly -1


@pytest.mark.parametrize("size", FC.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_border_rules(size, impl):
    """Every size of the list, on a noisy slanted wall without planted values: the filter changes the interior only (nothing at all below 5 x 5), a normal exists
    on 1..H-2 x 1..W-2 only (none below 3 x 3), the unprojected border is there."""
    filt, unproject, normal_weight, eps = impl
    H, W = size
    K = FC.Intr(H, W)
    d = FC.scene_depth("noisy", H, W, K, 3)
    out = filt(d)
    interior = np.zeros((H, W), bool); interior[2:H - 2, 2:W - 2] = True
    assert np.array_equal(out[~interior].astype(F64), d[~interior].astype(F64))
    assert interior.sum() == max(H - 4, 0) * max(W - 4, 0)
    if interior.any():
        assert (out[interior].astype(F64) != d[interior].astype(F64)).mean() > 0.5
    nw = normal_weight(unproject(out, K))
    stencil = np.zeros((H, W), bool); stencil[1:H - 1, 1:W - 1] = True
    assert np.array_equal(nw["valid"], stencil)
    assert (nw["weight"][~stencil] == -1).all() and (nw["weight"][stencil] > 0).all()


# ---- the restatement against the statement and the oracle -------------------------------------------------------------------------------
def _ids():
    return [(i, f) for i in range(len(FC.cases())) for f in (True, False)]


def test_restatement_decides_like_the_statement():
    """On every case: validity, the frame rule, the NaN pattern of the filtered depth, of the points and of the valid normals / weights equal
    the float64 statement's.  The values: the restatement's worst errors are what float32 costs (they are the e_ref of the GPU bar), and
    they stay within a generous multiple of one rounding."""
    worst = dict.fromkeys(FC.OUTPUTS, 0.0)
    n_valid = 0
    for i, filt in _ids():
        c = FC.cases()[i]
        st, rs = FC.results(i, filt)
        for k in ("valid", "use"):
            assert np.array_equal(st[k], rs[k]), (c.name, filt, k)
        for k in ("depth", "pc", "frame_depth", "frame_normal"):
            assert np.array_equal(np.isnan(st[k]), np.isnan(rs[k])), (c.name, filt, k)
        ok = st["valid"]
        assert np.array_equal(np.isnan(st["weight"][ok]), np.isnan(rs["weight"][ok])) and np.array_equal(np.isnan(st["normal"][ok]), np.isnan(rs["normal"][ok]))
        assert (rs["weight"][~ok] == -1).all()
        n_valid += int(ok.sum())
        e, m = FC.errors(rs, st)
        for o in FC.OUTPUTS:
            worst[o] = max(worst[o], e[o] / max(m[o], 1e-30) if o != "normal" else e[o])
    print("restatement vs float64, worst over the cases: depth %.3g (relative to the largest), normal %.3g, weight %.3g (relative)" % tuple(worst[o] for o in FC.OUTPUTS))
    assert n_valid > 10000
    # depth: a mean of <= 25 terms.  normal: one depth rounding (6e-8 z) against a neighbour distance of 2 z / fx: 1.6e-5 per rounding.
    # weight: carries the normal's error through theta / (c - theta), steep at grazing normals: a few 1e-3 relative at the steps
    assert worst["depth"] < 32 * 2.0 ** -24 and worst["normal"] < 1e-3 and worst["weight"] < 5e-2


def test_sign_and_scale_of_the_restatement_on_a_clean_plane():
    """The restatement on the unplanted tilted plane against the plane's own normal (not against the statement)."""
    for H, W in ((17, 17), (33, 19)):
        K = FC.Intr(H, W)
        rs = FC.restatement(FC.scene_depth("plane", H, W, K, 0), K, True)
        ok = rs["valid"]
        assert ok.sum() == (H - 2) * (W - 2)
        assert np.abs(rs["normal"][ok].astype(F64) + FC.PLANE_N[None]).max() < 2e-3


def test_restatement_against_the_oracle():
    """oracle.filter_depth / compute_normal_weight (NumPy float32, libm's expf / acosf, pairwise window sums) on the cases up to 33 x 19 and
    the noisy 48 x 64: masks and NaN patterns equal the restatement's; the value differences are reported (two float32 evaluations)."""
    from oracle import difusion_oracle as O
    worst = dict(depth=0.0, normal=0.0, weight=0.0)
    with np.errstate(all="ignore"):
        for i, filt in _ids():
            c = FC.cases()[i]
            if c.H * c.W > 700 and c.name != "noisy-48x64":
                continue
            _, rs = FC.results(i, filt)
            d = O.filter_depth(c.depth) if filt else c.depth
            assert np.array_equal(np.isnan(d), np.isnan(rs["depth"])), (c.name, filt)
            assert np.array_equal(d == 0, rs["depth"] == 0), (c.name, filt)
            fin = np.isfinite(d)
            worst["depth"] = max(worst["depth"], float(np.abs(d[fin] - rs["depth"][fin]).max(initial=0)))
            pc = O.unproject_depth(rs["depth"], *c.K.tuple())
            assert np.array_equal(pc.view(np.int32), rs["pc"].view(np.int32)) or np.array_equal(pc, rs["pc"], equal_nan=True)
            nw = O.compute_normal_weight(pc)
            valid = nw[..., 3] != -1
            assert np.array_equal(valid, rs["valid"]), (c.name, filt)
            assert np.array_equal(np.isnan(nw[..., 3]), np.isnan(rs["weight"])), (c.name, filt)
            ok = valid & np.isfinite(nw).all(-1)
            if ok.any():
                worst["normal"] = max(worst["normal"], float(np.abs(nw[ok][:, :3] - rs["normal"][ok]).max()))
                worst["weight"] = max(worst["weight"], float((np.abs(nw[ok][:, 3] - rs["weight"][ok]) / np.abs(rs["weight"][ok])).max()))
    print("oracle vs restatement: depth %.3g, normal %.3g, weight %.3g (relative)" % (worst["depth"], worst["normal"], worst["weight"]))
    assert worst["depth"] < 4e-6 and worst["normal"] < 1e-3 and worst["weight"] < 5e-2


def test_oracle_thresholds_compare_in_double():
    from oracle import difusion_oracle as O
    d = np.full((5, 5), 1.0, F32)
    d[2, 2] = FC.TH32
    assert O.filter_depth(d)[2, 2] == 0.0
    d[2, 2] = FC.UPPER
    assert O.filter_depth(d)[2, 2] != 0.0
    pc = FC.unproject32(np.full((3, 3), 1.0, F32), FC.Intr(3, 3))
    assert O.compute_normal_weight(pc)[1, 1, 3] > 0
    pc[1, 2, 2] = FC.TH32                                # a neighbour at float32(1e-6): below the double 1e-6 -> invalid
    assert O.compute_normal_weight(pc)[1, 1, 3] == -1
    pc[1, 2, 2] = FC.UPPER
    assert O.compute_normal_weight(pc)[1, 1, 3] > 0


def test_decision_margins():
    """No pixel outside the planted ones decides within 1e-3 of a threshold (frontend_cases.in_margin), in any case: float32 and float64
    take the same side everywhere.  The planted pixels inside the margin are decided on exact input values: the filtered depth there
    is the float32 input itself (or 0), bit for bit, in the float64 statement."""
    n_in = 0
    for i, filt in _ids():
        c = FC.cases()[i]
        st, _ = FC.results(i, filt)
        m = FC.in_margin(st)
        assert not (m & ~c.planted).any(), (c.name, filt, np.argwhere(m & ~c.planted)[:4])
        near = np.abs(st["depth"] - FC.TH) <= FC.MARGIN * FC.TH
        assert np.array_equal(st["depth"][near], c.depth[near].astype(F64)), (c.name, filt)
        n_in += int(m.sum())
    assert n_in > 100                                    # the plants are there
    # every planted value occurs in every scene at the largest size, on the seam block and on the rings
    for c in FC.cases():
        if (c.H, c.W) == (48, 64):
            seam = c.depth[13:19, 13:19][c.planted[13:19, 13:19]]
            assert c.planted[13:19, 13:19].sum() == 6 and c.planted[0, 0] and c.planted[-1, -1]
            vals = c.depth[c.planted]
            for pv in FC.PLANT_VALUES:
                assert ((vals.view(np.int32) == np.asarray(pv, F32).view(np.int32)) | (np.isnan(vals) & np.isnan(pv))).any(), pv
            assert len(seam) == 6


def k_table():
    """(case, filter, output, [e restatement, e numpy, e torch], ratio) for every case and output where all three errors are non-zero"""
    rows = []
    for i, filt in _ids():
        c = FC.cases()[i]
        st, rs = FC.results(i, filt)
        ev = [FC.errors(rs, st)[0]] + [FC.errors(FC.restatement(c.depth, c.K, filt, FC._Lib(kind), sequential=False), st)[0] for kind in ("numpy", "torch")]
        for o in FC.OUTPUTS:
            es = [e[o] for e in ev]
            if min(es) > 0:
                rows.append((c.name, filt, o, es, max(es) / min(es)))
    return rows


def test_k_fe():
    """K_FE is twice the largest ratio between the errors of three honest float32 evaluations of the same cases (the restatement: kernel
    order, exp / acos / sqrt rounded once; NumPy float32 with its libm and its own window sums; torch CPU float32 likewise), per case and
    output: re-measured here.  10 % of slack upwards (the ratios move with the libm build); a K_FE more than twice the measurement no
    longer describes it."""
    rows = k_table()
    for o in FC.OUTPUTS:
        r = max((r for r in rows if r[2] == o), key=lambda r: r[4])
        print(f"  {o}: {r[4]:.2f} at {r[0]} filter={r[1]}  errors {['%.3g' % e for e in r[3]]}")
    worst = max(r[4] for r in rows)
    print(f"largest ratio {worst:.2f} over {len(rows)} (case, filter, output) triples; K_FE = {FC.K_FE}")
    assert FC.K_FE / 4.0 <= worst <= 1.1 * FC.K_FE / 2.0, worst


# ---- point_box_filter -------------------------------------------------------------------------------------------------------------------
def test_box_filter_against_the_references_own():
    """tests/golden/box_filter.npz is what the reference's point_box_filter returned: same boxes in the same order; the float64 means within
    the golden's own float32 rounding (it is a float32 scatter_mean: a sum of up to n terms and a division), the fixed-point restatement
    within the derived bound of the float64 means."""
    from di_fusion_amd import synthetic as syn
    g = np.load(GOLDEN / "box_filter.npz")
    xyz, nrm = syn.frame_points(syn.default_room(), 3, syn.Intrinsic().scaled(0.5))
    xyz, nrm = xyz.numpy(), nrm.numpy()
    assert len(xyz) == int(g["n"])
    for vs in (0.02, 0.05):
        wp, wn = g[f"vs{int(vs * 100)}_points"], g[f"vs{int(vs * 100)}_normals"]
        mp, mn, cnt = FC.box_filter64(xyz, nrm, vs)
        assert mp.shape == wp.shape
        assert (np.abs(mp - wp) <= (cnt[:, None] + 1) * FC.spacing32(mp) + 2.0 ** -149).all()
        assert (np.abs(mn - wn) <= (cnt[:, None] + 1) * FC.spacing32(np.maximum(np.abs(mn), 1.0 / 64)) + 2.0 ** -149).all()      # cancelling sums: ulps of the terms, not of the mean
        fp, fn = FC.box_filter32(xyz, nrm, vs)
        assert (np.abs(fp - mp) <= FC.box_mean_bound(mp)).all() and (np.abs(fn - mn) <= FC.box_mean_bound(mn)).all()
        print(f"vs {vs}: {len(mp)} boxes; restatement vs float64 {np.abs(fp - mp).max():.3g} (bound at the largest coordinate {FC.box_mean_bound(np.abs(mp).max()):.3g})")


def test_box_filter_hand_cases():
    p = np.array([[1.5, -2.5, 0.25]], F32); n = np.array([[0.0, 0.6, 0.8]], F32)
    for f in (FC.box_filter64, FC.box_filter32):
        out = f(p, n, 0.02)
        assert np.array_equal(np.asarray(out[0], F64), p.astype(F64)) and np.allclose(out[1], n, atol=2.0 ** -24)      # one point: itself
    # all points in one box (within a third of a voxel of its centre): one mean
    g = np.random.default_rng(2)
    p = (np.array([[0.31, -0.47, 1.13]]) + g.uniform(-0.006, 0.006, (40, 3))).astype(F32)
    n = np.tile(np.array([[1.0, 0.0, 0.0]], F32), (40, 1))
    mp, mn, cnt = FC.box_filter64(p, n, 0.02)
    assert len(mp) <= 8 and cnt.sum() == 40
    one = (np.array([[0.31, -0.47, 1.13]]) + g.uniform(-0.003, 0.003, (40, 3)) + 0.01).astype(F32)
    lin, _ = FC.box_ids(one, 1.0)
    assert len(set(lin.tolist())) == 1
    mp, mn, cnt = FC.box_filter64(one, n, 1.0)
    assert mp.shape == (1, 3) and cnt[0] == 40 and np.allclose(mp[0], one.astype(F64).mean(0), atol=1e-15) and np.array_equal(mn, [[1.0, 0.0, 0.0]])
    # cells 31 and 32: the last bit of bitmap word 0 and the first of word 1
    p, n = FC.box_cloud_cells_31_32(0.05)
    lin, grid = FC.box_ids(p, 0.05)
    assert lin.tolist() == [0, 31, 31, 32, 40] and grid[0] >= 49
    mp, _, cnt = FC.box_filter64(p, n, 0.05)
    assert cnt.tolist() == [1, 2, 1, 1] and mp[1, 0] == (float(p[1, 0]) + float(p[2, 0])) / 2
    fp, _ = FC.box_filter32(p, n, 0.05)
    assert (np.abs(fp - mp) <= FC.box_mean_bound(mp)).all()
    # negative coordinates: the grid starts half a voxel below the smallest; order follows x fastest, then y, then z
    # (binary fractions, so that the float32 grid arithmetic is exact and the ids can be written down)
    p = np.array([[-1.0, -1.0, -1.0], [-0.875, -1.0, -1.0], [-1.0, -0.875, -1.0], [-1.0, -1.0, -0.875], [-0.999, -1.0, -1.0]], F32)
    lin, grid = FC.box_ids(p, 0.125)
    assert grid.tolist() == [18, 18, 18] and lin.tolist() == [0, 1, 18, 324, 0]
    mp, _, cnt = FC.box_filter64(p, np.zeros_like(p), 0.125)
    assert cnt.tolist() == [2, 1, 1, 1] and np.allclose(mp[0], [-0.9995, -1.0, -1.0], atol=1e-7)


def test_box_cloud_sizes():
    for n in (1, 63, 64, 65, 257):
        p, _ = FC.box_cloud(n, n)
        lin, grid = FC.box_ids(p, 0.05)
        assert len(p) == n and len(set(lin.tolist())) <= 200 and int(np.prod(grid)) <= 131072      # fits the single-workgroup scan (4,096 bitmap words)


# ---- the box grid's input contract -------------------------------------------------------------------------------------------------------
def test_pbf_grid_under_the_host_sanitizers(tmp_path):
    """tools/pbf_grid_check.cpp (its own main; host code only) built with AddressSanitizer, UBSan and float-cast-overflow: NaN / +-Inf
    bounds, an extent of 1e12, voxel_size down to 1e-6 and ordinary clouds through csrc/pbf_grid.hip.h: the verdicts, and every accepted
    cell id in [0, cells).  Skipped where there is no host compiler (or no sanitizer runtime to link)."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "pbf_grid_check"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fsanitize=float-cast-overflow", "-fno-sanitize-recover=all",
           "-I", str(ROOT / "di_fusion_amd" / "csrc"), str(ROOT / "tools" / "pbf_grid_check.cpp"), "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and ("asan" in b.stderr.lower() or "ubsan" in b.stderr.lower() or "sanitize" in b.stderr.lower()):
        pytest.skip("the host compiler cannot link the sanitizer runtimes: " + b.stderr.strip().splitlines()[-1])
    assert b.returncode == 0, b.stderr
    # (leak checking needs ptrace, which a sandboxed runner may not grant; the program's point is the arithmetic, not its two vectors)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    print(r.stdout.strip())
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failures" in r.stdout


if __name__ == "__main__":                               # the table of profiles/frontend_envelope_k.md
    rows = k_table()
    print(f"largest ratio {max(r[4] for r in rows):.2f}; K_FE = {FC.K_FE}")
    for r in sorted(rows, key=lambda r: -r[4])[:12]:
        print(f"| {r[0]} | {'on' if r[1] else 'off'} | {r[2]} | " + " | ".join("%.3g" % e for e in r[3]) + f" | {r[4]:.2f} |")
    print("e_ref per case (filter on / off): depth, normal, weight")
    for i, c in enumerate(FC.cases()):
        es = [FC.errors(FC.results(i, f)[1], FC.results(i, f)[0])[0] for f in (True, False)]
        print(f"| {c.name} | " + " | ".join("%.3g / %.3g" % (es[0][o], es[1][o]) for o in FC.OUTPUTS) + " |")
