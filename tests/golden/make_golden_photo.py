#!/usr/bin/env python3
"""Generate the fixtures of the tracker's photometric term by IMPORTING the reference's `SDFTracker` on the CPU:
photo_c2.npz, photo_c2_cut.npz, photo_track_c2.npz.

Runs only where the reference is available (see make_golden.py, whose stubs and `_import_reference_tracker()` are used as they are).  The
reference's two CUDA image kernels cannot run here: `rgb_odometry` and `gradient_xy` inside the reference's tracker module are bound to the
numpy restatement of tests/photo_ref.py.  Everything else is the reference's own code on CPU tensors: `_make_image_pyramid`
(torch.nn.functional.interpolate), `compute_rgb_Hg` (mask, sign flip, robust weights, weight / M, the unscaled K), `gauss_newton`.
So these fixtures pin the Python half of the term on the reference; the CUDA half is pinned by reading its 75 lines against the restatement.

Inputs are stored by SHA-256 (the tests regenerate them from di_fusion_amd.synthetic), outputs in full.

Usage:  python tests/golden/make_golden_photo.py [photo_c2] [photo_c2_cut] [photo_track_c2]
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent.parent))

import make_golden as mg                        # noqa: E402  (stubs + the reference on sys.path)
from di_fusion_amd import synthetic as syn      # noqa: E402
from tests import photo_ref as P                # noqa: E402

ref_tracker, Isometry, Quaternion = mg._import_reference_tracker()


def _rgb_odometry(prev_I, prev_D, cur_I, cur_D, cur_G, intr, krkinv, kt, min_grad_scale, max_depth_delta, compute_J):
    f, J = P.rgb_odometry(prev_I.numpy(), prev_D.numpy(), cur_I.numpy(), cur_D.numpy(), cur_G.numpy(), intr, krkinv, kt, min_grad_scale,
                          max_depth_delta, compute_J)
    return [torch.from_numpy(f), torch.from_numpy(J)] if compute_J else [torch.from_numpy(f)]


ref_tracker.rgb_odometry = _rgb_odometry
ref_tracker.gradient_xy = lambda I: torch.from_numpy(P.gradient_xy(I.numpy()))


class Calib:
    """dataset.production.FrameIntrinsic, as far as the tracker reads it."""

    def __init__(self, intr):
        self.fx, self.fy, self.cx, self.cy = intr.fx, intr.fy, intr.cx, intr.cy

    def to_K(self):
        return np.array([[self.fx, 0.0, self.cx], [0.0, self.fy, self.cy], [0.0, 0.0, 1.0]])


def tracker(map_, rgb, iters, sdf=None):
    a = argparse.Namespace(sdf=sdf or dict(robust_kernel="huber", robust_k=5.0, subsample=0.5), rgb=dict(rgb), iter_config=iters)
    return ref_tracker.SDFTracker(map_, a)


def frame_pyramid(t, out, tag, scene, f, depth_cut, noise):
    """The reference's pyramid of frame f of the C2 orbit; the hashes of the inputs and of the nine arrays go to `out`."""
    R, tt = syn.orbit_pose(f)
    rgb, depth = syn.render_rgbd(scene, R, tt, syn.Intrinsic(), depth_cut=depth_cut, noise_seed=(1234 + f) if noise else None)
    out[f"{tag}_rgb_sha"], out[f"{tag}_depth_sha"] = np.array(P.sha(rgb.numpy())), np.array(P.sha(depth.numpy()))
    Is, Ds, Gs = t._make_image_pyramid(torch.mean(rgb, dim=-1), depth)
    for l in range(3):
        out[f"{tag}_I{l}_sha"], out[f"{tag}_D{l}_sha"], out[f"{tag}_G{l}_sha"] = (np.array(P.sha(x[l].contiguous().numpy())) for x in (Is, Ds, Gs))
    return Is, Ds, Gs


def as_np(pyr):
    return tuple([x.contiguous().numpy() for x in lst] for lst in pyr)


def photo_fixture(name, depth_cut):
    scene, _ = syn.config_c2()
    intr = syn.Intrinsic()
    calib = Calib(intr)
    out = dict(depth_cut=np.array(depth_cut, dtype=np.float64), frames=np.array([1, 2]), rgb_args=np.array(json.dumps(P.SHIPPED_RGB)))
    t = tracker(None, P.SHIPPED_RGB, [])
    prev = frame_pyramid(t, out, "prev", scene, 1, depth_cut, True)
    cur = frame_pyramid(t, out, "cur", scene, 2, depth_cut, True)
    t.last_intensity, t.last_depth = prev[0], prev[1]
    out["nan_depth_share"] = np.float64(torch.isnan(cur[1][0]).float().mean())
    (R1, t1), (R2, t2) = syn.orbit_pose(1), syn.orbit_pose(2)
    true_delta = Isometry(q=Quaternion(matrix=R1.T @ R2), t=R1.T @ (t2 - t1))
    rng = np.random.default_rng(20)
    poses = [("identity", Isometry()), ("true", true_delta)]
    for j in range(3):
        xi = np.concatenate([rng.uniform(-0.03, 0.03, 3) / np.sqrt(3), rng.uniform(-1.5, 1.5, 3) / np.sqrt(3) * np.pi / 180])
        out[f"twist{j}"] = xi
        poses.append((f"twist{j}", Isometry.from_twist(xi)))
    n = 0
    worst = 0.0
    for level in range(3):
        for pname, delta in poses:
            for kernel, k in P.KERNELS:
                t.rgb_args.robust_kernel, t.rgb_args.robust_k = kernel, k
                H, g, e = t.compute_rgb_Hg(level, delta, cur[0], cur[1], cur[2], calib, False)
                _, _, e2 = t.compute_rgb_Hg(level, delta, cur[0], cur[1], cur[2], calib, True)
                assert e2 == e
                R, tt = delta.q.rotation_matrix, delta.t
                x64, S, mask = P.compute_rgb_hg(as_np(prev), as_np(cur), level, [intr.fx, intr.fy, intr.cx, intr.cy], R, tt,
                                                dict(P.SHIPPED_RGB, robust_kernel=kernel, robust_k=k))
                x_ref = np.concatenate([H.reshape(36), g, [e]])
                c = f"case{n}"
                out[f"{c}_level"], out[f"{c}_pose"], out[f"{c}_kernel"], out[f"{c}_k"] = np.int64(level), np.array(pname), np.array(str(kernel)), np.float64(k)
                out[f"{c}_R"], out[f"{c}_t"] = np.array(R, dtype=np.float64), np.array(tt, dtype=np.float64)
                out[f"{c}_x"], out[f"{c}_M"], out[f"{c}_mask_sha"] = x_ref, np.int64(mask.sum()), np.array(P.sha(mask))
                out[f"{c}_d_ref"], out[f"{c}_S"] = np.abs(x_ref - x64[:43]), S
                krkinv, kt = P.warp_of([intr.fx, intr.fy, intr.cx, intr.cy], R, tt)
                out[f"{c}_krkinv"], out[f"{c}_kt"] = krkinv, kt
                rel = np.abs(x_ref - x64[:43])[:42].max() / np.abs(x_ref[:42]).max()
                worst = max(worst, rel)
                print(f"{name} {c}: level {level} {pname:9s} {str(kernel):5s} M {int(mask.sum()):6d} ({mask.mean():.3f}) e {e:.6f} cond(H) {np.linalg.cond(H):.2e} "
                      f"ref vs float64: {rel:.1e} of the largest entry, e {abs(e - x64[42]) / max(abs(e), 1e-30):.1e}")
                n += 1
    out["n_cases"] = np.int64(n)
    np.savez_compressed(HERE / f"{name}.npz", **out)
    print(f"{name}: {n} cases, worst {worst:.2e}; saved ({(HERE / f'{name}.npz').stat().st_size / 1e6:.2f} MB)")


def photo_track_fixture():
    """The map and the cloud of track_c2 (tests/test_oracle_track.py:TRACK), the noise-free RGB-D frames 1 (last) and 2 (current), and the
    reference's `gauss_newton` over the shipped iter_config with the shipped rgb block, from the last frame's pose (tracker.py:121-124)."""
    model, _ = mg.load_reference_model()
    scene, cfg = syn.config_c2()
    intr = syn.Intrinsic()
    m = mg.ref_map.DenseIndexedMap(model, cfg.namespace(), 29, torch.device("cpu"))
    out = dict(n_map_frames=np.int64(2), iter_config=np.array(json.dumps(P.SHIPPED_ITERS)), rgb_args=np.array(json.dumps(P.SHIPPED_RGB)))
    for f in range(2):
        xyz, nrm = syn.frame_points(scene, f, intr)
        out[f"f{f}_xyz_sha"] = np.array(P.sha(xyz.numpy()))
        m.integrate_keyframe(xyz, nrm)
    out["n_occupied"] = np.int64(int(m.n_occupied))
    obs, R_gt, t_gt = syn.frame_cloud_camera(scene, 2, intr.scaled(0.5))
    out["obs_sha"], out["obs_n"] = np.array(P.sha(obs.numpy())), np.int64(obs.size(0))
    R_last, t_last = syn.orbit_pose(1)
    out["last_R"], out["last_t"], out["gt_R"], out["gt_t"] = R_last, t_last, R_gt, t_gt
    last_pose = Isometry(q=Quaternion(matrix=R_last), t=t_last)
    t = tracker(m, P.SHIPPED_RGB, P.SHIPPED_ITERS)
    t.all_pd_pose = [last_pose]
    prev = frame_pyramid(t, out, "prev", scene, 1, (0.5, 5.0), False)
    cur = frame_pyramid(t, out, "cur", scene, 2, (0.5, 5.0), False)
    t.last_intensity, t.last_depth = prev[0], prev[1]
    calls = []
    sdf0, rgb0 = t.compute_sdf_Hg, t.compute_rgb_Hg

    def rec_sdf(n_iter, last_pose_, delta, obs_xyz, no_grad=False):
        r = sdf0(n_iter, last_pose_, delta, obs_xyz, no_grad)
        calls.append(("sdf", n_iter, delta.q.rotation_matrix.copy(), delta.t.copy(), r))
        return r

    def rec_rgb(level, delta, Is, Ds, Gs, calib, no_grad=False):
        r = rgb0(level, delta, Is, Ds, Gs, calib, no_grad)
        j = len(calls)
        calls.append((str(level), -1 if no_grad else 0, delta.q.rotation_matrix.copy(), delta.t.copy(), r))
        x64, S, mask = P.compute_rgb_hg(as_np(prev), as_np(cur), level, [intr.fx, intr.fy, intr.cx, intr.cy], delta.q.rotation_matrix, delta.t,
                                        P.SHIPPED_RGB, no_grad)
        x_ref = np.concatenate([np.zeros(42) if no_grad else np.concatenate([r[0].reshape(36), r[1]]), [r[2]]])
        d = np.abs(x_ref - x64[:43])
        if no_grad:
            d[:42] = 0.0
        out[f"gn{j}_M"], out[f"gn{j}_mask_sha"], out[f"gn{j}_d_ref"], out[f"gn{j}_S"] = np.int64(mask.sum()), np.array(P.sha(mask)), d, S
        return r

    t.compute_sdf_Hg, t.compute_rgb_Hg = rec_sdf, rec_rgb
    final = t.gauss_newton(last_pose, cur[0], cur[1], cur[2], obs.clone(), Calib(intr))
    out["gn_n_calls"] = np.int64(len(calls))
    for j, (term, it, dR, dt, (H, g, e)) in enumerate(calls):
        out[f"gn{j}_term"], out[f"gn{j}_no_grad"], out[f"gn{j}_delta_R"], out[f"gn{j}_delta_t"], out[f"gn{j}_e"] = \
            np.array(term), np.int64(1 if H is None else 0), dR, dt, np.float64(e)
        if term == "sdf":
            out[f"gn{j}_iter"] = np.int64(it)
        if H is not None:
            out[f"gn{j}_H"], out[f"gn{j}_g"] = H, g
        print(f"photo_track_c2 call {j}: {term:3s} no_grad {H is None} e {e:.12f}")
    out["gn_final_R"], out["gn_final_t"] = final.q.rotation_matrix.copy(), final.t.copy()
    err_t = np.linalg.norm(final.t - t_gt)
    err_R = np.degrees(np.arccos(np.clip((np.trace(final.q.rotation_matrix.T @ R_gt) - 1) / 2, -1, 1)))
    print(f"photo_track_c2: {len(calls)} calls, final pose off the true one by {err_t * 1000:.2f} mm / {err_R:.4f} deg")
    np.savez_compressed(HERE / "photo_track_c2.npz", **out)
    print(f"photo_track_c2: saved ({(HERE / 'photo_track_c2.npz').stat().st_size / 1e6:.2f} MB)")


if __name__ == "__main__":
    which = sys.argv[1:] or ["photo_c2", "photo_c2_cut", "photo_track_c2"]
    if "photo_c2" in which:
        photo_fixture("photo_c2", (0.5, 5.0))
    if "photo_c2_cut" in which:
        photo_fixture("photo_c2_cut", (0.5, 3.0))
    if "photo_track_c2" in which:
        photo_track_fixture()
