"""Times the tracker's photometric term (reference tracker.py:131-172) on frames 1 and 2 of the C2 room stream at 640 x 480: one evaluation at
pyramid levels 0 / 1 / 2, with and without derivatives — the one-launch `dif_rgb_hg` against the reference's op sequence (the flat operator
`rgb_odometry`, then mask / negate / einsum / sums as torch ops, H / g / energy to the host) —, the SDF term `dif_sdf_hg` on the tracker's
320 x 240 cloud of the same frame against the same map beside it, the per-frame pyramid front end, and one whole `track_camera` call with the
shipped configuration.  Host wall clock: every evaluation ends with its numbers on the host, like an iteration of the loop.
Usage: python tools/bench_photo.py"""
import json
import sys
import time
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from di_fusion_amd import synthetic as syn                      # noqa: E402
from di_fusion_amd.network import utility as net_util            # noqa: E402
from di_fusion_amd.system import ext                             # noqa: E402
from di_fusion_amd.system.map import DenseIndexedMap             # noqa: E402
from di_fusion_amd.system.tracker import Pose, SDFTracker, photo_warp, rgb_hg, sdf_hg      # noqa: E402

RGB = dict(weight=500.0, robust_kernel=None, robust_k=0.01, min_grad_scale=0.0, max_depth_delta=0.2)      # configs/fusion-lr-kt.yaml:51-56
ITERS = [{"n": 10, "type": [["rgb", 2]]}, {"n": 10, "type": [["sdf"], ["rgb", 1]]}, {"n": 50, "type": [["sdf"], ["rgb", 0]]}]


def wall(fn, reps=200):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def device_ms(fn, reps=100):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def reference_evaluation(prev, cur, level, calib, delta, no_grad=False):
    """tracker.py:131-172 as the reference writes it (no robust kernel), on the flat operator of this library."""
    intr, krkinv, kt = photo_warp(calib, delta)
    o = ext.rgb_odometry(prev[0][level], prev[1][level], cur[0][level], cur[1][level], cur[2][level], intr, krkinv, kt, RGB["min_grad_scale"],
                         RGB["max_depth_delta"], not no_grad)
    f_map = o[0]
    mask = ~torch.isnan(f_map)
    f_map = f_map[mask]
    scale = 1. / f_map.size(0) * RGB["weight"]
    e = (f_map * f_map).sum().item() * scale
    if no_grad:
        return None, None, float(e)
    J = -o[1][mask]
    H = torch.einsum("na,nb->nab", J, J).sum(0) * scale
    g = (J * f_map.unsqueeze(1)).sum(0) * scale
    return H.cpu().numpy().astype(float), g.cpu().numpy().astype(float), float(e)


def main():
    dev = torch.device("cuda:0")
    scene, cfg = syn.config_c2()
    intr = syn.Intrinsic()
    calib = SimpleNamespace(fx=intr.fx, fy=intr.fy, cx=intr.cx, cy=intr.cy)
    model = net_util.networks_from_arrays(net_util.load_weights_npz())
    m = DenseIndexedMap(model, cfg.namespace(), 29, dev, initial_capacity=1024)
    frames = []
    for f in range(3):
        R, t = syn.orbit_pose(f)
        frames.append(syn.render_rgbd(scene, R, t, intr, dev, noise_seed=1234 + f))
        if f < 2:
            m.integrate_keyframe(*syn.frame_points(scene, f, intr, dev))
    prev, cur = ext.photo_pyramid(*frames[1]), ext.photo_pyramid(*frames[2])
    last, delta = Pose(*syn.orbit_pose(1)), Pose()
    owner = SimpleNamespace()
    kw = dict(weight=RGB["weight"], max_depth_delta=RGB["max_depth_delta"])
    out = {"device": torch.cuda.get_device_name(0), "clock": "host wall clock per call in ms, the numbers on the host at the end of each (200 calls)"}
    for level in range(3):
        args = (owner, prev[0][level], prev[1][level], cur[0][level], cur[1][level], cur[2][level], calib, delta)
        H, g, e, M = rgb_hg(*args, **kw)
        Hr, gr, er = reference_evaluation(prev, cur, level, calib, delta)
        assert np.abs(H - Hr).max() < 1e-4 * np.abs(Hr).max() and abs(e - er) < 1e-5 * max(1.0, er)
        h, w = cur[0][level].shape
        out[f"rgb level {level} ({w}x{h})"] = {
            "pixels": h * w, "valid_pixels": M,
            "rgb_hg_ms": round(wall(lambda: rgb_hg(*args, **kw)), 4),
            "rgb_hg_no_grad_ms": round(wall(lambda: rgb_hg(*args, no_grad=True, **kw)), 4),
            "reference_op_sequence_ms": round(wall(lambda: reference_evaluation(prev, cur, level, calib, delta), 50), 4),
            "reference_op_sequence_no_grad_ms": round(wall(lambda: reference_evaluation(prev, cur, level, calib, delta, True), 50), 4)}
    obs, _, _ = syn.frame_cloud_camera(scene, 2, intr.scaled(0.5), device=dev)
    _, _, _, M = sdf_hg(m, obs, last, delta, "huber", 5.0)
    out["sdf term (320x240 cloud)"] = {"points": int(obs.size(0)), "valid_points": M,
                                       "sdf_hg_ms": round(wall(lambda: sdf_hg(m, obs, last, delta, "huber", 5.0)), 4),
                                       "sdf_hg_no_grad_ms": round(wall(lambda: sdf_hg(m, obs, last, delta, "huber", 5.0, no_grad=True)), 4)}
    rgb, depth = frames[2]

    def torch_pyramid():
        Is, Ds = [torch.mean(rgb, dim=-1)], [depth]
        for _ in range(2):
            hw = (Is[-1].size(0) // 2, Is[-1].size(1) // 2)
            Is.append(torch.nn.functional.interpolate(Is[-1][None, None], hw, mode="bilinear")[0, 0])
            Ds.append(torch.nn.functional.interpolate(Ds[-1][None, None], hw, mode="nearest")[0, 0])
        return Is, Ds, [ext.gradient_xy(i) for i in Is]

    out["pyramid front end (640x480)"] = {"photo_pyramid_device_ms": round(device_ms(lambda: ext.photo_pyramid(rgb, depth)), 4),
                                          "photo_pyramid_wall_ms": round(wall(lambda: ext.photo_pyramid(rgb, depth)), 4),
                                          "torch_ops_and_gradient_xy_device_ms": round(device_ms(torch_pyramid), 4)}
    # one tracked frame, the shipped configuration (pyramid, cloud preparation, the loop)
    t = SDFTracker(m, SimpleNamespace(sdf=dict(robust_kernel="huber", robust_k=5.0, subsample=0.5), rgb=dict(RGB), iter_config=ITERS))
    for f in range(2):
        t.track_camera(*frames[f], calib, set_pose=Pose(*syn.orbit_pose(f)))
    n_eval = [0]
    sdf0, rgb0 = t.compute_sdf_Hg, t.compute_rgb_Hg
    t.compute_sdf_Hg = lambda *a, **k: (n_eval.__setitem__(0, n_eval[0] + 1), sdf0(*a, **k))[1]
    t.compute_rgb_Hg = lambda *a, **k: (n_eval.__setitem__(0, n_eval[0] + 1), rgb0(*a, **k))[1]

    def previous_frame():
        t.all_pd_pose = t.all_pd_pose[:2]
        t.last_intensity, t.last_depth = prev[0], prev[1]

    def tracked():
        previous_frame()
        return t.track_camera(*frames[2], calib)

    def loop_alone():
        previous_frame()
        return t.gauss_newton(t.all_pd_pose[1], *cur, t.last_processed_pc[0], calib)

    pose = tracked()
    per_frame = n_eval[0]
    gn = wall(loop_alone, 20)
    out["track_camera frame 2, shipped config"] = {
        "term_evaluations": per_frame, "track_camera_ms": round(wall(tracked, 20), 3), "gauss_newton_alone_ms": round(gn, 3),
        "off_true_pose_mm": round(float(np.linalg.norm(pose.t - syn.orbit_pose(2)[1])) * 1e3, 2)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
