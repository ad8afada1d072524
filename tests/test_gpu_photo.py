"""GPU: the tracker's photometric term (csrc/kernels_photo.hip.h; reference ext/imgproc/photometric.cu, tracker.py:41-56, 131-172) — the image
operators bit for bit against the numpy restatement (tests/photo_ref.py) and the reference's torch pyramid, the fused `dif_rgb_hg` against
"flat operator, then float64 sums on the host" and against what the REFERENCE's `SDFTracker.compute_rgb_Hg` returned
(tests/golden/photo_*.npz), and through `gauss_newton` / `track_camera` with the configuration the reference ships.

What the fixtures pin and what they do not: see tests/test_photo_cpu.py — the Python half of the term is the reference's own code, its two CUDA
kernels were stood in for by the restatement, which is pinned on them only by reading."""
import ctypes
import json
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from di_fusion_amd import _lib
from di_fusion_amd import synthetic as syn
from di_fusion_amd.system import ext
from di_fusion_amd.system.map import DenseIndexedMap
from di_fusion_amd.system.tracker import Pose, SDFTracker, photo_warp, rgb_hg
from tests import photo_ref as P
from tests.conftest import GOLDEN
from tests.test_photo_cpu import INTR, fixture_frames, kernel_of, within

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CALIB = SimpleNamespace(fx=INTR[0], fy=INTR[1], cx=INTR[2], cy=INTR[3])
# double accumulation of N <= 307,200 terms in any order errs by at most (N - 1) 2^-53 S = 3.4e-11 S
SUM_SLACK = 1e-10


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    """Equal as bit patterns, any NaN equal to any NaN."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb])


def to_np(pyr):
    return tuple([x.cpu().numpy() for x in lst] for lst in pyr)


def gpu_pyramids(g, noise):
    return [ext.photo_pyramid(rgb, depth) for rgb, depth in fixture_frames(g, noise, DEV)]


def tracker_args(iters=(), rgb=None, **rgb_extra):
    return SimpleNamespace(sdf=dict(robust_kernel="huber", robust_k=5.0, subsample=0.5), rgb=dict(rgb or P.SHIPPED_RGB, **rgb_extra),
                           iter_config=list(iters))


def test_pyramid_and_gradient_bits():
    """All nine arrays of both frames of photo_c2 bit-identical to the reference's (torch CPU resizes + the restated Sobel); the fused front
    end's gradients are `ext.gradient_xy` of its own intensities; `_make_image_pyramid` gives the same lists.  At 481 x 641 every level against
    torch's CPU resize of the level above within 3 x 2^-24 (tests/test_photo_cpu.py: the bound's derivation)."""
    g = np.load(GOLDEN / "photo_c2.npz")
    for tag, (rgb, depth) in zip(("prev", "cur"), fixture_frames(g, True, DEV)):
        Is, Ds, Gs = ext.photo_pyramid(rgb, depth)
        for l in range(3):
            assert Is[l].shape == (480 >> l, 640 >> l) and Gs[l].shape == (480 >> l, 640 >> l, 2)
            for name, lst in zip("IDG", (Is, Ds, Gs)):
                assert P.sha(lst[l].cpu().numpy()) == str(g[f"{tag}_{name}{l}_sha"]), f"{tag} {name}{l}"
            assert same_bits(ext.gradient_xy(Is[l]).cpu().numpy(), Gs[l].cpu().numpy())
        t = SDFTracker(None, tracker_args())
        I2, D2, G2 = t._make_image_pyramid(Is[0].clone(), depth)          # (torch.mean on the GPU is not the CPU's ((r + g) + b) / 3)
        assert I2[0].data_ptr() != Is[0].data_ptr()
        for l in range(3):
            assert same_bits(I2[l].cpu().numpy(), Is[l].cpu().numpy()) and same_bits(D2[l].cpu().numpy(), Ds[l].cpu().numpy())
            assert same_bits(G2[l].cpu().numpy(), Gs[l].cpu().numpy())
    rng = np.random.default_rng(4)
    H, W = 481, 641
    rgb = torch.from_numpy(rng.random((H, W, 3), dtype=np.float32))
    depth = torch.from_numpy(0.5 + 4.5 * rng.random((H, W), dtype=np.float32))
    depth[rng.random((H, W)) < 0.1] = float("nan")
    Is, Ds, Gs = ext.photo_pyramid(rgb.to(DEV), depth.to(DEV))
    assert np.array_equal(Is[0].cpu().numpy(), torch.mean(rgb, dim=-1).numpy()) and same_bits(Ds[0].cpu().numpy(), depth.numpy())
    worst = 0.0
    for l in (1, 2):
        h, w = Is[l - 1].size(0) // 2, Is[l - 1].size(1) // 2
        ti = torch.nn.functional.interpolate(Is[l - 1].cpu()[None, None], (h, w), mode="bilinear")[0, 0].numpy()
        td = torch.nn.functional.interpolate(Ds[l - 1].cpu()[None, None], (h, w), mode="nearest")[0, 0].numpy()
        assert Is[l].shape == (h, w) and same_bits(Ds[l].cpu().numpy(), td)
        worst = max(worst, float(np.abs(Is[l].cpu().numpy() - ti).max()))
        assert same_bits(Is[l].cpu().numpy(), P.resize_bilinear(Is[l - 1].cpu().numpy(), h, w))           # the restatement: bitwise at any size
    for l in range(3):
        assert same_bits(ext.gradient_xy(Is[l]).cpu().numpy(), Gs[l].cpu().numpy())
        assert same_bits(Gs[l].cpu().numpy(), P.gradient_xy(Is[l].cpu().numpy()))
    print(f"  481 x 641: bilinear levels within {worst / 2.0 ** -24:.2f} x 2^-24 of torch's CPU resize")
    assert worst <= 3 * 2.0 ** -24


def check_flat_and_fused(owner, prev, cur, level, calib, pose, rgb_args, kernels, what, level_scale=1.0):
    """One (level, pose): the flat operator against the restatement (masks identical, f and J bit-identical), then for every robust kernel the
    fused call against the float64 sums of the flat operator's outputs on the host (M equal, every entry within SUM_SLACK x S; two calls the
    same bits; the `no_grad` energy the full call's, bitwise).  Returns {kernel: (44 numbers of the fused call, S)}."""
    pn, cn = to_np(prev), to_np(cur)
    intr, krkinv, kt = photo_warp(calib, pose, level_scale)
    f, J = ext.rgb_odometry(prev[0][level], prev[1][level], cur[0][level], cur[1][level], cur[2][level], intr, krkinv, kt,
                            rgb_args["min_grad_scale"], rgb_args["max_depth_delta"], True)
    (f1,) = ext.rgb_odometry(prev[0][level], prev[1][level], cur[0][level], cur[1][level], cur[2][level], intr, krkinv, kt,
                             rgb_args["min_grad_scale"], rgb_args["max_depth_delta"], False)
    f, J, f1 = f.cpu().numpy(), J.cpu().numpy(), f1.cpu().numpy()
    fr, Jr = P.rgb_odometry(pn[0][level], pn[1][level], cn[0][level], cn[1][level], cn[2][level], intr, krkinv, kt, rgb_args["min_grad_scale"],
                            rgb_args["max_depth_delta"], True)
    assert np.array_equal(np.isnan(f), np.isnan(fr)), f"{what}: valid masks differ in {(np.isnan(f) != np.isnan(fr)).sum()} pixels"
    assert same_bits(f, fr) and same_bits(f1, f), f"{what}: f"
    assert same_bits(J, Jr), f"{what}: J differs in {(bits(J) != bits(Jr)).sum() - 0} words"
    res = {}
    for kernel, k in kernels:
        host, S, mask = P.sums_of_flat(f, J, rgb_args["weight"], kernel, k)
        kw = dict(weight=rgb_args["weight"], robust_kernel=kernel, robust_k=k, min_grad_scale=rgb_args["min_grad_scale"],
                  max_depth_delta=rgb_args["max_depth_delta"], level_scale=level_scale)
        H, gg, e, M = rgb_hg(owner, prev[0][level], prev[1][level], cur[0][level], cur[1][level], cur[2][level], calib, pose, **kw)
        assert M == int(host[43]), f"{what} {kernel}: M {M} vs {int(host[43])}"
        x = np.concatenate([H.reshape(36), gg, [e]])
        within(x, host[:43], 0.0, S, SUM_SLACK, f"{what} {kernel}: fused vs flat + host sums")
        assert np.array_equal(H, H.T)
        H2, g2, e2, M2 = rgb_hg(owner, prev[0][level], prev[1][level], cur[0][level], cur[1][level], cur[2][level], calib, pose, **kw)
        assert np.array_equal(H, H2) and np.array_equal(gg, g2) and e == e2 and M == M2
        H3, g3, e3, M3 = rgb_hg(owner, prev[0][level], prev[1][level], cur[0][level], cur[1][level], cur[2][level], calib, pose, no_grad=True, **kw)
        assert H3 is None and g3 is None and e3 == e and M3 == M
        res[kernel] = (np.concatenate([x, [M]]), S)
    return res


@pytest.mark.parametrize("name", ["photo_c2", "photo_c2_cut"])
def test_flat_operator_fused_term_and_the_references_numbers(name):
    """Every case of the fixture (levels 0-2 x five poses x three robust kernels).  Against the reference's numbers, entry by entry and in
    absolute terms: |x_gpu - x_ref| <= d_ref + 1e-10 S with d_ref = |x_ref - x_64| as the fixture's generator measured it between the
    reference's float32 torch sums and the float64 restatement on the same valid set (the triangle inequality, no margin)."""
    g = np.load(GOLDEN / f"{name}.npz")
    prev, cur = gpu_pyramids(g, True)
    rgb_args = json.loads(str(g["rgb_args"]))
    owner = SimpleNamespace()
    n = 0
    worst = 0.0
    while n < int(g["n_cases"]):
        level, pose = int(g[f"case{n}_level"]), Pose(g[f"case{n}_R"], g[f"case{n}_t"])
        group = [m for m in range(n, int(g["n_cases"])) if int(g[f"case{m}_level"]) == level and str(g[f"case{m}_pose"]) == str(g[f"case{n}_pose"])]
        kernels = [(kernel_of(g, f"case{m}"), float(g[f"case{m}_k"])) for m in group]
        res = check_flat_and_fused(owner, prev, cur, level, CALIB, pose, rgb_args, kernels, f"{name} level {level} {g[f'case{n}_pose']}")
        for m, (kernel, _) in zip(group, kernels):
            x, S = res[kernel]
            assert int(x[43]) == int(g[f"case{m}_M"])
            assert np.allclose(S, g[f"case{m}_S"], rtol=1e-9, atol=0.0)
            within(x[:43], g[f"case{m}_x"], g[f"case{m}_d_ref"], g[f"case{m}_S"], SUM_SLACK, f"{name} case {m} vs the reference")
            worst = max(worst, float(np.abs(x[:42] - g[f"case{m}_x"][:42]).max() / np.abs(g[f"case{m}_x"][:42]).max()))
        n = group[-1] + 1
    print(f"  {name}: H, g vs the reference's tracker within {worst:.1e} of the largest entry")


def test_crafted_inputs():
    """NaN / 0 / inf in either depth image, warp targets on the image's edges and one pixel outside, |warped - d0| exactly at max_depth_delta and
    one ulp beyond, gradients just below and above min_grad_scale: the flat operator, the fused call and the restatement agree, and the pixels
    crafted for a verdict get it."""
    H, W = 24, 32
    rng = np.random.default_rng(11)
    F = np.float32
    prev_I, cur_I = rng.random((H, W), dtype=F), rng.random((H, W), dtype=F)
    cur_D = np.full((H, W), 2.0, dtype=F)
    prev_D = np.full((H, W), 2.0, dtype=F)
    cur_G = np.stack([np.full((H, W), 0.25, dtype=F), np.full((H, W), -0.5, dtype=F)], axis=-1)
    # the warp: K R K^-1 = identity, K t = (-2, 2, 0) at depth 2: (u, v) -> (u - 1, v + 1), warped depth = the depth
    krkinv, kt = np.eye(3).flatten().tolist(), [-2.0, 2.0, 0.0]
    max_dd, min_grad = 0.5, 0.01
    cur_D[3, 5], cur_D[3, 6], cur_D[3, 7], cur_D[3, 8] = np.nan, 0.0, np.inf, -np.inf          # the current depth: NaN, 0 (quotients -inf and +inf), inf
    # the previous depth at the targets of row 6 (targets: row 7, column u - 1)
    at = lambda u, val: prev_D.__setitem__((7, u - 1), val)   # noqa: E731
    at(5, np.nan); at(6, 0.0); at(7, np.inf); at(8, -1.0)
    at(10, F(2.5)); at(11, np.nextafter(F(2.5), F(3))); at(12, F(1.5)); at(13, np.nextafter(F(1.5), F(0)))
    # the previous depth must be > 0 even where it is within max_depth_delta of the warped depth: at depth 0.25 (u, v) -> (u - 8, v + 8)
    cur_D[6, 20], cur_D[6, 22] = 0.25, 0.25
    prev_D[14, 12], prev_D[14, 14] = 0.0, 0.5
    # gradients around min_grad_scale (row 9): 0.1^2 rounds above float32(0.01), 0.0999^2 is below; NaN gradient
    cur_G[9, 5] = (F(0.1), 0.0); cur_G[9, 6] = (F(0.0999), 0.0); cur_G[9, 7] = (np.nan, 0.0); cur_G[9, 8] = (0.0, F(-0.1)); cur_G[9, 9] = (0.0, 0.0)
    intr = [30.0, 28.0, 15.5, 11.5]
    fr, Jr = P.rgb_odometry(prev_I, prev_D, cur_I, cur_D, cur_G, intr, krkinv, kt, min_grad, max_dd, True)
    valid = ~np.isnan(fr)
    # the verdicts
    assert not valid[:, 0].any() and valid[0:H - 1, 1].all()            # column 0 -> target column -1: outside; column 1 -> 0: the edge
    assert not valid[H - 1, :].any() and valid[H - 2, 1:].sum() >= W - 6    # row H - 1 -> target row H: outside; row H - 2 -> H - 1: the edge
    assert not valid[3, 5:9].any()
    assert not valid[6, 5:9].any()
    assert valid[6, 10] and not valid[6, 11] and valid[6, 12] and not valid[6, 13]
    assert not valid[6, 20] and valid[6, 22]
    assert valid[9, 5] and not valid[9, 6] and not valid[9, 7] and valid[9, 8] and not valid[9, 9]
    t = lambda a: torch.from_numpy(a).to(DEV)   # noqa: E731
    tp = (t(prev_I), t(prev_D), t(cur_I), t(cur_D), t(cur_G))
    f, J = ext.rgb_odometry(*tp, intr, krkinv, kt, min_grad, max_dd, True)
    f, J = f.cpu().numpy(), J.cpu().numpy()
    assert np.array_equal(np.isnan(f), ~valid) and same_bits(f, fr) and same_bits(J, Jr)
    lib = _lib.load()
    ws = torch.zeros((int(lib.dif_rgb_hg_workspace_bytes()) + 256,), dtype=torch.uint8, device=DEV)
    base = ws.data_ptr() + (-ws.data_ptr()) % 256
    out = torch.zeros((44,), dtype=torch.float64, device=DEV)
    for kernel, k in ((0, 0.0), (1, 0.3), (2, 0.6)):
        a = ext.photo_args(intr, krkinv, kt, min_grad, max_dd, 500.0, kernel, k, False)
        assert lib.dif_rgb_hg(*[_lib.ptr(x) for x in tp], H, W, ctypes.byref(a), ctypes.c_void_p(base), ws.numel() - 256, _lib.ptr(out), None, 1,
                              _lib.stream_ptr()) == 0
        torch.cuda.synchronize()
        x = out.cpu().numpy()
        host, S, _ = P.sums_of_flat(f, J, 500.0, [None, "huber", "tukey"][kernel], k)
        assert int(x[43]) == int(valid.sum()) == int(host[43])
        within(x[:43], host[:43], 0.0, S, SUM_SLACK, f"crafted, kernel {kernel}")


def test_compute_rgb_hg_poses_and_errors():
    g = np.load(GOLDEN / "photo_c2.npz")
    prev, cur = gpu_pyramids(g, True)
    t = SDFTracker(None, tracker_args())
    t.last_intensity, t.last_depth = prev[0], prev[1]
    p = Pose(g["case6_R"], g["case6_t"])
    want = t.compute_rgb_Hg(1, p, *cur, CALIB)
    assert want[0].shape == (6, 6) and want[1].shape == (6,) and isinstance(want[2], float)
    x_ref = g["case21_x"]                                             # level 1, twist0, no robust kernel
    assert np.abs(want[0].reshape(36) - x_ref[:36]).max() < 1e-5 * np.abs(x_ref[:36]).max()
    iso = SimpleNamespace(q=SimpleNamespace(rotation_matrix=p.R.copy()), t=p.t.copy())
    for pose in (iso, p.matrix):
        got = t.compute_rgb_Hg(1, pose, *cur, CALIB)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]
    H0, g0, e0 = t.compute_rgb_Hg(1, p, *cur, CALIB, no_grad=True)
    assert H0 is None and g0 is None and e0 == want[2]
    # level_calib: the intrinsics of the level
    t2 = SDFTracker(None, tracker_args(level_calib=True))
    t2.last_intensity, t2.last_depth = prev[0], prev[1]
    scaled = t2.compute_rgb_Hg(1, p, *cur, CALIB)
    direct = rgb_hg(t2, prev[0][1], prev[1][1], cur[0][1], cur[1][1], cur[2][1], SimpleNamespace(fx=INTR[0] / 2, fy=INTR[1] / 2, cx=INTR[2] / 2, cy=INTR[3] / 2),
                    p, weight=500.0, max_depth_delta=0.2)
    assert np.array_equal(scaled[0], direct[0]) and scaled[2] == direct[2] and not np.array_equal(scaled[0], want[0])
    assert np.array_equal(t2.compute_rgb_Hg(0, p, *cur, CALIB)[0], t.compute_rgb_Hg(0, p, *cur, CALIB)[0])
    # no valid pixel: M = 0, the term raises like the reference's 1. / 0
    t.last_depth = [torch.full_like(d, float("nan")) for d in prev[1]]
    H, gg, e, M = rgb_hg(t, prev[0][2], t.last_depth[2], cur[0][2], cur[1][2], cur[2][2], CALIB, p, weight=500.0, max_depth_delta=0.2)
    assert M == 0 and e == 0.0 and not H.any() and not gg.any()
    with pytest.raises(ZeroDivisionError):
        t.compute_rgb_Hg(2, p, *cur, CALIB)
    t.last_depth = prev[1]
    with pytest.raises(RuntimeError):
        rgb_hg(t, prev[0][2].cpu(), prev[1][2], cur[0][2], cur[1][2], cur[2][2], CALIB, p)
    with pytest.raises(RuntimeError):
        ext.gradient_xy(cur[0][2].cpu())
    with pytest.raises(RuntimeError):
        ext.rgb_odometry(prev[0][2], prev[1][2], cur[0][2], cur[1][2].cpu(), cur[2][2], INTR, [1, 0, 0, 0, 1, 0, 0, 0, 1], [0, 0, 0], 0.0, 0.2, True)
    with pytest.raises(NotImplementedError):
        rgb_hg(t, prev[0][2], prev[1][2], cur[0][2], cur[1][2], cur[2][2], CALIB, p, robust_kernel="cauchy")
    # an rgb configuration without colour is a clear error; without a previous frame too
    t3 = SDFTracker(None, tracker_args(P.SHIPPED_ITERS))
    with pytest.raises(ValueError, match="rgb_data"):
        t3.track_camera(None, cur[1][0], CALIB, set_pose=Pose())
    with pytest.raises(RuntimeError, match="previous frame"):
        t3.compute_rgb_Hg(0, p, *cur, CALIB)


def test_c_abi_refuses_what_it_cannot_run():
    """`dif_rgb_hg` through ctypes: a workspace that is too small or not 256-byte aligned, an unknown robust kernel, a missing result or image
    pointer, an image under 3 x 3 are DIF_EINVAL (-1), and nothing is launched."""
    lib = _lib.load()
    need = int(lib.dif_rgb_hg_workspace_bytes())
    assert need > 0 and need % 256 == 0
    H, W = 12, 16
    ws = torch.zeros((need + 512,), dtype=torch.uint8, device=DEV)
    base = ws.data_ptr() + (-ws.data_ptr()) % 256
    out = torch.zeros((44,), dtype=torch.float64, device=DEV)
    img = torch.full((H, W), 0.5, dtype=torch.float32, device=DEV)
    dep = torch.full((H, W), 2.0, dtype=torch.float32, device=DEV)
    grad = torch.full((H, W, 2), 0.25, dtype=torch.float32, device=DEV)
    a = ext.photo_args([20.0, 20.0, 7.5, 5.5], [1, 0, 0, 0, 1, 0, 0, 0, 1], [0, 0, 0], 0.0, 0.2, 1.0, 0, 0.0, False)

    def call(ws_ptr, ws_bytes, out_ptr=_lib.ptr(out), h=H, w=W, first=_lib.ptr(img)):
        return int(lib.dif_rgb_hg(first, _lib.ptr(dep), _lib.ptr(img), _lib.ptr(dep), _lib.ptr(grad), h, w, ctypes.byref(a), ctypes.c_void_p(ws_ptr),
                                  ws_bytes, out_ptr, None, 1, _lib.stream_ptr()))

    assert call(base, need) == 0
    torch.cuda.synchronize()
    assert int(out[43].item()) == H * W and out[42].item() == 0.0          # the identity warp of a constant image: every pixel, no residual
    out.fill_(-7.0)
    assert call(base, need - 1) == -1
    assert call(base + 64, need) == -1
    assert call(0, need) == -1
    assert call(base, need, None) == -1
    assert call(base, need, first=None) == -1
    assert call(base, need, h=2) == -1 and call(base, need, w=2) == -1
    a.robust_kernel = 3
    assert call(base, need) == -1
    a.robust_kernel = 0
    f = torch.empty((H, W), dtype=torch.float32, device=DEV)
    assert int(lib.dif_rgb_odometry(_lib.ptr(img), _lib.ptr(dep), _lib.ptr(img), _lib.ptr(dep), _lib.ptr(grad), H, W, ctypes.byref(a), None, None,
                                    _lib.stream_ptr())) == -1
    assert int(lib.dif_gradient_xy(_lib.ptr(img), H, W, None, _lib.stream_ptr())) == -1
    assert int(lib.dif_photo_pyramid(None, _lib.ptr(dep), H, W, None, _lib.stream_ptr())) == -1
    torch.cuda.synchronize()
    assert (out == -7.0).all()                                            # nothing ran
    assert int(lib.dif_rgb_odometry(_lib.ptr(img), _lib.ptr(dep), _lib.ptr(img), _lib.ptr(dep), _lib.ptr(grad), H, W, ctypes.byref(a), _lib.ptr(f), None,
                                    _lib.stream_ptr())) == 0
    torch.cuda.synchronize()
    assert (f == 0.0).all()


def track_setup(model, g):
    """The map and the cloud of track_c2 and the noise-free pyramids of frames 1 and 2, checked against photo_track_c2's hashes."""
    scene, cfg = syn.config_c2()
    m = DenseIndexedMap(model, cfg.namespace(), 29, DEV, initial_capacity=1024)
    for f in range(int(g["n_map_frames"])):
        xyz, nrm = syn.frame_points(scene, f, syn.Intrinsic())
        assert P.sha(xyz.numpy()) == str(g[f"f{f}_xyz_sha"])
        m.integrate_keyframe(xyz.to(DEV), nrm.to(DEV))
    assert int(m.n_occupied) == int(g["n_occupied"])
    obs, _, _ = syn.frame_cloud_camera(scene, 2, syn.Intrinsic().scaled(0.5))
    assert P.sha(obs.numpy()) == str(g["obs_sha"])
    prev, cur = gpu_pyramids(g, False)
    return m, obs.to(DEV), prev, cur


def test_gauss_newton_vs_the_references_loop(gpu_model):
    """`SDFTracker.gauss_newton` over the SHIPPED iter_config and rgb block against the reference's run (photo_track_c2): the same number and
    kind of evaluations, the same accept / reject decisions, every evaluated pose within 2e-5 and energy within 2e-3 relative, and the
    returned pose (the bars of tests/test_gpu_track.py for the SDF-only loop)."""
    g = np.load(GOLDEN / "photo_track_c2.npz")
    m, obs, prev, cur = track_setup(gpu_model, g)
    t = SDFTracker(m, tracker_args(json.loads(str(g["iter_config"])), json.loads(str(g["rgb_args"]))))
    t.all_pd_pose = [Pose(g["last_R"], g["last_t"])]
    t.last_intensity, t.last_depth = prev[0], prev[1]
    calls = []
    sdf0, rgb0 = t.compute_sdf_Hg, t.compute_rgb_Hg

    def rec_sdf(n_iter, last_pose, delta, obs_xyz, no_grad=False):
        r = sdf0(n_iter, last_pose, delta, obs_xyz, no_grad)
        calls.append(("sdf", delta, r))
        return r

    def rec_rgb(level, delta, Is, Ds, Gs, calib, no_grad=False):
        r = rgb0(level, delta, Is, Ds, Gs, calib, no_grad)
        calls.append((str(level), delta, r))
        return r

    t.compute_sdf_Hg, t.compute_rgb_Hg = rec_sdf, rec_rgb
    final = t.gauss_newton(t.all_pd_pose[-1], *cur, obs, CALIB)
    print("  terms: " + " ".join(c[0] for c in calls))
    assert len(calls) == int(g["gn_n_calls"])
    for j, (term, delta, (H, gg, e)) in enumerate(calls):
        assert term == str(g[f"gn{j}_term"]) and (H is None) == bool(g[f"gn{j}_no_grad"]), f"evaluation {j}"
        assert np.abs(delta.R - g[f"gn{j}_delta_R"]).max() < 2e-5 and np.abs(delta.t - g[f"gn{j}_delta_t"]).max() < 2e-5, f"evaluation {j}"
        assert abs(e - float(g[f"gn{j}_e"])) < 2e-3 * max(1.0, float(g[f"gn{j}_e"])), f"evaluation {j}"
    assert np.abs(final.R - g["gn_final_R"]).max() < 2e-5 and np.abs(final.t - g["gn_final_t"]).max() < 2e-5
    print(f"  {len(calls)} evaluations, final pose {np.linalg.norm(final.t - g['gt_t']) * 1000:.2f} mm from the true one")


def pose_error(pose, R, t):
    return float(np.linalg.norm(pose.t - t)), float(np.degrees(np.arccos(np.clip((np.trace(pose.R.T @ R) - 1) / 2, -1, 1))))


def test_track_camera_with_the_shipped_configuration(gpu_model):
    """`track_camera(rgb, depth, calib)` end to end on three noise-free frames of the C2 stream with the tracking block the reference ships:
    frames 0 and 1 with their poses given, frame 2 tracked — with the reference's calib at every level (the default), with `level_calib`,
    and with the SDF term alone.  The bar is the project's own for this scene: 1 cm / 0.05 degrees from the true pose."""
    scene, cfg = syn.config_c2()
    intr = syn.Intrinsic()
    errs = {}
    for name, args in (("reference calib", tracker_args(P.SHIPPED_ITERS)), ("level_calib", tracker_args(P.SHIPPED_ITERS, level_calib=True)),
                       ("sdf only", tracker_args([{"n": 10, "type": [["sdf"]]}]))):
        m = DenseIndexedMap(gpu_model, cfg.namespace(), 29, DEV, initial_capacity=1024)
        t = SDFTracker(m, args)
        for f in range(3):
            R, tt = syn.orbit_pose(f)
            rgb, depth = syn.render_rgbd(scene, R, tt, intr, DEV)
            pose = t.track_camera(rgb, depth, CALIB, set_pose=Pose(R, tt) if f < 2 else None)
            if name != "sdf only":
                assert len(t.last_intensity) == 3 and t.last_intensity[2].shape == (120, 160) and t.last_depth[0].shape == (480, 640)
            assert t.last_colored_pcd is None
            if f < 2:
                xyz, n_w = syn.frame_points(scene, f, intr, DEV)
                m.integrate_keyframe(xyz, n_w)
        errs[name] = pose_error(pose, R, tt)
    print("  tracked frame 2: " + "; ".join(f"{k}: {e[0] * 1000:.2f} mm / {e[1]:.4f} degrees" for k, e in errs.items()))
    for k, (et, er) in errs.items():
        assert et < 0.01 and er < 0.05, k
