"""The depth front end (k_depth_frontend, k_normal_weight, k_unproject), point_box_filter and groupby_sum against the float64 statement and
the float32 restatement of tests/frontend_cases.py, on its cases: four scenes with planted NaN / 0 / -1 / threshold / subnormal / Inf
values on the tile seam, the corners and the outer rings, at fourteen sizes from 1 x 1 to 48 x 64, filter on and off.

THE BAR, per case and output (filtered depth, normal, weight):   e_gpu <= K_FE * e_ref + U ulp
  e_ref  the restatement's worst error against the float64 statement over the case, e_gpu the kernel's;
  K_FE   frontend_cases.K_FE, measured on the CPU (test_frontend_cpu.py::test_k_fe, profiles/frontend_envelope_k.md);
  U      1 for the filtered depth (expf: 1 ulp in the HIP math API's table), 0 for the rest.
Every test prints e_gpu / e_ref.  Decisions (validity, NaN patterns, the -1 weights, the frame pair's NaN pattern) must equal the float64
statement's on every pixel: the cases keep every unplanted pixel out of the thresholds' margins and decide the planted ones on exact
inputs (test_frontend_cpu.py::test_decision_margins).  The normal of an invalid pixel is not written by the reference nor by the kernel:
those slots are checked to keep a sentinel (test_output_subsets), not compared.
"""
import functools

import numpy as np
import pytest
import torch

from tests import frontend_cases as FC

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F32, F64 = np.float32, np.float64
SENTINEL = -7.25


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _same(x, y):
    """the same bits, or NaN on both sides (which operand's NaN payload survives is the compiler's choice)"""
    x, y = np.ascontiguousarray(x, F32), np.ascontiguousarray(y, F32)
    return x.shape == y.shape and bool(((x.view(np.int32) == y.view(np.int32)) | (np.isnan(x) & np.isnan(y))).all())


@functools.lru_cache(maxsize=None)
def _gpu(i, filt):
    """the fused kernel's five outputs on case i, as the dict frontend_cases.errors takes"""
    from di_fusion_amd.system import ext
    c = FC.cases()[i]
    d, pc, nw, fd, fn = (x.cpu().numpy() for x in ext.depth_frontend(_t(c.depth), *c.K.tuple(), filter=filt, want_frame=True))
    return dict(depth=d, pc=pc, normal=nw[..., :3], weight=nw[..., 3], valid=nw[..., 3] != -1, frame_depth=fd, frame_normal=fn)


def _ids():
    return [(i, f) for i in range(len(FC.cases())) for f in (True, False)]


def _check_bars(got, st, rs, name, fails, ratios):
    e_gpu, m = FC.errors(got, st)
    e_ref, _ = FC.errors(rs, st)
    for o in FC.OUTPUTS:
        bar = FC.bar(e_ref[o], m[o], o)
        if e_ref[o] > 0:
            ratios[o] = max(ratios[o], e_gpu[o] / e_ref[o])
        if not e_gpu[o] <= bar:
            fails.append(f"{name} {o}: e_gpu {e_gpu[o]:.3g} > bar {bar:.3g} (e_ref {e_ref[o]:.3g})")
    return e_gpu, e_ref


def test_fused_frontend_against_the_statement():
    """dif_depth_frontend, all outputs, every case: decisions equal the float64 statement's, values within the bar, points and the frame
    pair bit for bit what the restatement makes of the kernel's own filtered depth."""
    fails, ratios, n_valid = [], dict.fromkeys(FC.OUTPUTS, 0.0), 0
    for i, filt in _ids():
        c = FC.cases()[i]
        name = f"{c.name} filter={'on' if filt else 'off'}"
        st, rs = FC.results(i, filt)
        got = _gpu(i, filt)
        # decisions
        if not np.array_equal(got["valid"], st["valid"]):
            fails.append(f"{name}: validity differs at {np.argwhere(got['valid'] != st['valid'])[:4].tolist()}")
            continue
        for k in ("depth", "pc", "weight", "frame_depth", "frame_normal"):
            if not np.array_equal(np.isnan(got[k]), np.isnan(st[k])):
                fails.append(f"{name}: NaN pattern of {k} differs at {np.argwhere(np.isnan(got[k]) != np.isnan(st[k]))[:4].tolist()}")
        ok = st["valid"]
        n_valid += int(ok.sum())
        if not np.array_equal(np.isnan(got["normal"][ok]), np.isnan(st["normal"][ok])):
            fails.append(f"{name}: NaN pattern of the valid normals differs")
        if not (got["weight"][~ok] == -1).all():
            fails.append(f"{name}: an invalid pixel's weight is not -1")
        # values that involve no device function: bit for bit
        if not filt and not _same(got["depth"], c.depth):
            fails.append(f"{name}: the unfiltered depth is not the input")
        border = np.ones((c.H, c.W), bool); border[2:c.H - 2, 2:c.W - 2] = False
        if not _same(got["depth"][border], c.depth[border]):
            fails.append(f"{name}: write_border does not carry the raw border")
        if not _same(got["pc"], FC.unproject32(got["depth"], c.K)):
            fails.append(f"{name}: points are not the back-projection of the kernel's depth")
        if not filt and not (_same(got["pc"], rs["pc"]) and _same(got["normal"][ok], rs["normal"][ok])):
            fails.append(f"{name}: points / normals differ from the restatement's bits (no expf, acosf only behind the weight)")
        use = st["use"]
        if not (_same(got["frame_depth"][use], got["depth"][use]) and _same(got["frame_normal"][use], got["normal"][use])):
            fails.append(f"{name}: the frame pair does not carry the depth / normal")
        e_gpu, e_ref = _check_bars(got, st, rs, name, fails, ratios)
        print(f"{name}: e_gpu / e_ref  " + "  ".join(f"{o} {e_gpu[o]:.3g} / {e_ref[o]:.3g}" for o in FC.OUTPUTS))
    print("largest e_gpu / e_ref: " + ", ".join(f"{o} {ratios[o]:.2f}" for o in FC.OUTPUTS) + f"; K_FE = {FC.K_FE}; {n_valid} valid pixels")
    assert n_valid > 10000
    assert not fails, "\n".join(fails)


def test_flat_ops_against_the_statement():
    """The three flat ops of the reference's API.  dif_unproject: the restatement's bits.  dif_filter_depth: writes the interior only (a
    sentinel buffer; nothing at all when H or W is below 5), the interior holds the fused kernel's bits.  dif_compute_normal_weight on the
    restatement's points: decisions equal the statement's, values within the bar."""
    from di_fusion_amd.system import ext
    fails, ratios = [], dict.fromkeys(FC.OUTPUTS, 0.0)
    for i, c in enumerate(FC.cases()):
        st_off, rs_off = FC.results(i, False)
        if not _same(ext.unproject_depth(_t(c.depth), *c.K.tuple()).cpu().numpy(), rs_off["pc"]):
            fails.append(f"{c.name}: k_unproject differs from the restatement")
        out = torch.full((c.H, c.W), SENTINEL, device=DEV)
        ext.filter_depth(_t(c.depth), out)
        out = out.cpu().numpy()
        interior = np.zeros((c.H, c.W), bool); interior[2:c.H - 2, 2:c.W - 2] = True
        if not (out[~interior] == F32(SENTINEL)).all():
            fails.append(f"{c.name}: dif_filter_depth wrote outside the interior")
        if not _same(out[interior], _gpu(i, True)["depth"][interior]):
            fails.append(f"{c.name}: dif_filter_depth differs from the fused kernel")
        for filt in (True, False):
            st, rs = FC.results(i, filt)
            nw = ext.compute_normal_weight(_t(rs["pc"])).cpu().numpy()
            got = dict(depth=rs["depth"], normal=nw[..., :3], weight=nw[..., 3], valid=nw[..., 3] != -1)
            if not np.array_equal(got["valid"], st["valid"]) or not np.array_equal(np.isnan(got["weight"]), np.isnan(st["weight"])):
                fails.append(f"{c.name} filter={filt}: k_normal_weight decides differently")
                continue
            if not _same(got["normal"][st["valid"]], rs["normal"][st["valid"]]):
                fails.append(f"{c.name} filter={filt}: k_normal_weight's normals differ from the restatement's bits")
            _check_bars(got, st, rs, f"{c.name} filter={filt} (flat)", fails, ratios)
    print("k_normal_weight, largest e_gpu / e_ref: " + ", ".join(f"{o} {ratios[o]:.2f}" for o in FC.OUTPUTS))
    assert not fails, "\n".join(fails)


def test_output_subsets():
    """dif_depth_frontend through the C ABI with each of {depth_out}, {pc}, {normal_weight}, {frame pair} alone: the bits of the all-outputs
    call (sentinel-filled buffers, so what is not written is compared too: the normal slots of invalid pixels stay untouched); a lone
    frame_depth is DIF_EINVAL."""
    from di_fusion_amd import _lib
    lib = _lib.load()
    names = {c.name: i for i, c in enumerate(FC.cases())}
    for nm in ("sphere-22x22", "noisy-5x5", "plane-33x19", "near-3x3", "noisy-48x64"):
        c = FC.cases()[names[nm]]
        d = _t(c.depth)
        shapes = dict(depth=(c.H, c.W), pc=(c.H, c.W, 3), nw=(c.H, c.W, 4), fd=(c.H, c.W), fn=(c.H, c.W, 3))

        def run(want, filt):
            bufs = {k: torch.full(s, SENTINEL, device=DEV) for k, s in shapes.items()}
            rc = lib.dif_depth_frontend(_lib.ptr(d), c.H, c.W, *c.K.tuple(), 1 if filt else 0, *[_lib.ptr(bufs[k] if k in want else None) for k in shapes],
                                        _lib.stream_ptr())
            torch.cuda.synchronize()
            return rc, {k: bufs[k].cpu().numpy() for k in want}
        for filt in (True, False):
            rc, full = run(tuple(shapes), filt)
            assert rc == 0
            invalid = full["nw"][..., 3] == -1
            assert (full["nw"][invalid][:, :3] == F32(SENTINEL)).all(), nm
            assert _same(full["nw"][..., 3], _gpu(names[nm], filt)["weight"])
            for want in (("depth",), ("pc",), ("nw",), ("fd", "fn")):
                rc, part = run(want, filt)
                assert rc == 0
                for k in want:
                    assert _same(part[k], full[k]), (nm, filt, want, k)
        assert run(("fd",), True)[0] == -1 and run(("fn",), True)[0] == -1          # DIF_EINVAL


# ---- point_box_filter -------------------------------------------------------------------------------------------------------------------
SINGLE_WG_CELLS = 131072          # 4,096 bitmap words: launch_scan takes its single-workgroup path; the default 2^27 takes the two-pass one
VS = 0.05


def _box(p, n, **kw):
    from di_fusion_amd.system import ext
    fp, fn = ext.point_box_filter(_t(p), _t(n), VS, **kw)
    return fp.cpu().numpy(), fn.cpu().numpy()


def _box_clouds():
    clouds = [(f"N={n}", *FC.box_cloud(n, 100 + n, VS)) for n in (1, 63, 64, 65, 257)]
    clouds.append(("cells 31|32", *FC.box_cloud_cells_31_32(VS)))
    return clouds


def test_point_box_filter_against_the_statement():
    """Boxes: count and order equal the restatement's.  Means: within 2^-25 + 2^-23 |mean64| (1 + 2^-24) of the float64 mean (each point's
    rounding to the 2^-24 fixed point, one rounding of the sum to float32, one float32 division).  A permuted cloud and the other scan
    path (max_cells = 131072: single workgroup; default: two passes) give identical bits."""
    g = np.random.default_rng(9)
    for name, p, n in _box_clouds():
        mp, mn, cnt = FC.box_filter64(p, n, VS)
        rp, rn = FC.box_filter32(p, n, VS)
        assert len(mp) <= 200
        outs = {}
        for path, kw in (("single", dict(max_cells=SINGLE_WG_CELLS)), ("two-pass", {})):
            fp, fn = _box(p, n, **kw)
            assert fp.shape == rp.shape == mp.shape and fn.shape == rn.shape, (name, path, fp.shape, mp.shape)
            ep, en = np.abs(fp - mp), np.abs(fn - mn)
            print(f"{name} {path}: {len(mp)} boxes; worst error / bound: points {(ep / FC.box_mean_bound(mp)).max():.2f}, normals {(en / FC.box_mean_bound(mn)).max():.2f}; "
                  f"{int((fp.view(np.int32) != rp.view(np.int32)).sum() + (fn.view(np.int32) != rn.view(np.int32)).sum())} values differ from the restatement's bits")
            assert (ep <= FC.box_mean_bound(mp)).all() and (en <= FC.box_mean_bound(mn)).all(), (name, path)
            perm = g.permutation(len(p))
            qp, qn = _box(p[perm], n[perm], **kw)
            assert _same(qp, fp) and _same(qn, fn), (name, path, "input order")
            outs[path] = (fp, fn)
        assert _same(outs["single"][0], outs["two-pass"][0]) and _same(outs["single"][1], outs["two-pass"][1]), name
    e = np.zeros((0, 3), F32)
    for kw in (dict(max_cells=SINGLE_WG_CELLS), {}):
        fp, fn = _box(e, e, **kw)
        assert fp.shape == (0, 3) and fn.shape == (0, 3)


@pytest.mark.parametrize("max_cells", [SINGLE_WG_CELLS, None], ids=["single", "two-pass"])
def test_point_box_filter_refuses_what_the_grid_cannot_hold(max_cells):
    """A cloud with one NaN row, one with a point at 1e12 and one beyond max_cells each raise (told apart in the message), write nothing,
    and the next ordinary call returns the right bits: the refusal leaves the scratch bitmap clean."""
    kw = {} if max_cells is None else dict(max_cells=max_cells)
    p, n = FC.box_cloud(257, 7, VS)
    want = _box(p, n, **kw)
    mp, mn, _ = FC.box_filter64(p, n, VS)
    assert (np.abs(want[0] - mp) <= FC.box_mean_bound(mp)).all()
    bad_nan, bad_far, wide = p.copy(), p.copy(), p.copy()
    bad_nan[100] = np.nan
    bad_far[200, 1] = 1e12
    wide[5, 0] = 10000.0                                   # 200,000 boxes on x at 5 cm, times 43 x 43: beyond 2^27 cells, not beyond int
    for bad, what in ((bad_nan, "NaN or infinite"), (bad_far, "max_cells"), (wide, "max_cells")):
        with pytest.raises(RuntimeError, match=what):
            _box(bad, n, **kw)
        got = _box(p, n, **kw)
        assert _same(got[0], want[0]) and _same(got[1], want[1]), what


# ---- groupby_sum -------------------------------------------------------------------------------------------------------------------------
def test_groupby_sum_ignores_indices_out_of_range():
    """Indices < 0 and >= C are skipped in sums and counts; counts exact; every sum within count * ulp of the float64 sum, the ulp taken
    at the group's sum of magnitudes (each of the `count` atomic adds rounds a partial sum no larger than that).  Lw = 1, N = 1 included."""
    from di_fusion_amd.system import ext
    g = np.random.default_rng(4)
    for N, L, C in ((1, 1, 3), (1, 29, 1), (257, 1, 5), (1000, 29, 37), (65, 3, 2)):
        vals = g.standard_normal((N, L)).astype(F32)
        idx = g.integers(-3, C + 3, N).astype(np.int64)
        if N == 1:
            idx[:] = C - 1
        else:
            k = np.arange(0, N, 7)
            idx[k] = np.where(k % 2 == 0, -1 - k, C + k)          # one row in seven is out of range for certain: -1, C, and far beyond both
        s, cnt = ext.groupby_sum(_t(vals), _t(idx), C)
        s, cnt = s.cpu().numpy(), cnt.cpu().numpy()
        keep = (idx >= 0) & (idx < C)
        want_c = np.bincount(idx[keep], minlength=C)
        want_s, mag = np.zeros((C, L)), np.zeros((C, L))
        np.add.at(want_s, idx[keep], vals[keep].astype(F64)); np.add.at(mag, idx[keep], np.abs(vals[keep]).astype(F64))
        assert np.array_equal(cnt, want_c), (N, L, C)
        assert (np.abs(s - want_s) <= want_c[:, None] * FC.spacing32(mag)).all(), (N, L, C)
        assert N == 1 or (~keep).sum() > N // 8
    # every index out of range: nothing is written
    vals = np.ones((10, 4), F32)
    s, cnt = ext.groupby_sum(_t(vals), _t(np.array([-1, 5, 6, -9, 5, 7, 2 ** 40, -2 ** 40, 5, -1], np.int64)), 5)
    assert not s.any() and not cnt.any()
