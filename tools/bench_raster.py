"""Times `dif_mesh_render` (depth, normal, std and triangle images of an indexed mesh from a camera pose) with HIP events: the welded mesh of the
C3 bench stream after `--frames` frames at 640x480 from the stream's own poses (the micro-triangle regime: a lattice cell of 1.25 cm seen from
a metre or two), and one synthetic close-up in which large triangles dominate (a coarse icosphere filling the image: every triangle goes
through the cooperative path).  Beside them `dif_mesh_weld` on the same soup, for scale.  Per launch: the kernels of one call as the torch
profiler sees them (mean over the repetitions); where it sees none, run this under `rocprofv3 --kernel-trace --stats` with `--only`.
For the stream's views the rendered depth is also held against the input depth frame of the same pose (median and 95th percentile of the
absolute difference over the pixels valid in both).
Usage: python tools/bench_raster.py [--warmup 3] [--reps 20] [--frames 20] [--only c3|closeup] [--md profiles/mesh_render.md]"""
import argparse
import ctypes
import json
import re
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from di_fusion_amd import _lib, synthetic as syn                 # noqa: E402
from di_fusion_amd.network import utility as net_util            # noqa: E402
from di_fusion_amd.system import mesh as M                       # noqa: E402
from tests import raster_ref as R                                # noqa: E402

DEV = torch.device("cuda:0")


def timed(call, warmup, reps):
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return dict(median=round(statistics.median(ms), 4), min=round(min(ms), 4), max=round(max(ms), 4))


def per_launch(call, reps, kernels=r"k_raster_\w+"):
    """mean device microseconds per kernel of one call, by kernel name (those that match `kernels`, and the memsets); None if the profiler
    cannot start or records no kernel of the library"""
    from torch.profiler import ProfilerActivity, profile
    try:
        prof = profile(activities=[ProfilerActivity.CUDA])
        prof.__enter__()
    except RuntimeError as e:               # (a profiler that cannot start is no reason to lose the totals; anything after this is a bug and raises)
        print(f"per-launch times unavailable: {e!r}", file=sys.stderr)
        return None
    try:
        for _ in range(reps):
            call()
        torch.cuda.synchronize()
    finally:
        prof.__exit__(None, None, None)
    out = {}
    for e in prof.key_averages():
        m = re.search(kernels, e.key)
        name = m.group(0) if m else ("memset" if re.search(r"memset|fill", e.key, flags=re.I) else None)
        total = e.device_time_total if hasattr(e, "device_time_total") else e.cuda_time_total
        if name and total:
            out[name] = round(out.get(name, 0.0) + total / reps, 2)
    return out if any(k != "memset" for k in out) else None


class Renderer:
    """the entry point with every buffer allocated once"""

    def __init__(self, mesh: M.IndexedMesh, H, W):
        self.lib = _lib.load()
        self.mesh, self.H, self.W = mesh, H, W
        self.V, self.K = int(mesh.vertices.shape[0]), int(mesh.triangles.shape[0])
        self.ws_bytes = int(self.lib.dif_mesh_render_workspace_bytes(self.V, self.K, H, W))
        self.ws = torch.empty((self.ws_bytes,), dtype=torch.uint8, device=DEV)
        f32 = dict(dtype=torch.float32, device=DEV)
        self.depth, self.normal, self.std = torch.empty((H, W), **f32), torch.empty((H, W, 3), **f32), torch.empty((H, W), **f32)
        self.triangle = torch.empty((H, W), dtype=torch.int32, device=DEV)
        self.counts = torch.empty((_lib.RASTER_COUNT,), dtype=torch.int32, device=DEV)

    def call(self, args):
        m, P = self.mesh, _lib.ptr
        _lib.check(self.lib.dif_mesh_render(P(m.vertices), P(m.normals), P(m.vertex_std), P(m.triangles), self.V, self.K, ctypes.byref(args), P(self.ws),
                                            self.ws_bytes, P(self.depth), P(self.normal), P(self.std), P(self.triangle), P(self.counts),
                                            _lib.stream_ptr()), "dif_mesh_render")


def measure(name, mesh, pose, intr, warmup, reps, input_depth=None):
    H, W = intr.height, intr.width
    r = Renderer(mesh, H, W)
    args = M.raster_args(pose, intr, H, W)
    t = timed(lambda: r.call(args), warmup, reps)
    c = dict(zip(M.RENDER_COUNT_NAMES, r.counts.cpu().tolist()))
    assert c["status"] == 0, c
    row = dict(name=name, vertices=r.V, triangles=r.K, image=f"{W}x{H}", warmup=warmup, reps=reps, ms_median=t["median"], ms_min=t["min"], ms_max=t["max"],
               counts=c, large_share=round(c["large"] / max(c["drawn"], 1), 4), pixels_hit_share=round(c["pixels_hit"] / (H * W), 4),
               workspace_bytes=r.ws_bytes, per_launch_us=per_launch(lambda: r.call(args), reps))
    if input_depth is not None:
        both = torch.isfinite(r.depth) & torch.isfinite(input_depth)
        diff = (r.depth - input_depth)[both].abs()
        row.update(pixels_valid_in_both=int(both.sum()), depth_diff_median_m=round(float(diff.median()), 5), depth_diff_p95_m=round(float(diff.quantile(0.95)), 5))
    return row


def weld_ms(soup, warmup, reps):
    """`dif_mesh_weld` on the same soup (the launch chain alone, as tools/bench_weld.py times it)"""
    tri, std, ids, bm, vs, res, n_xyz = soup
    T = int(tri.shape[0])
    lib = _lib.load()
    args = M.weld_args(bm, vs, res, n_xyz)
    ws_bytes = int(lib.dif_mesh_weld_workspace_bytes(T))
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=DEV)
    f32 = dict(dtype=torch.float32, device=DEV)
    out = [torch.empty((3 * T, 3), **f32), torch.empty((3 * T, 3), **f32), torch.empty((3 * T,), **f32), torch.empty((T, 3), dtype=torch.int32, device=DEV),
           torch.empty((T,), dtype=torch.int64, device=DEV), torch.empty((_lib.WELD_COUNT,), dtype=torch.int32, device=DEV)]
    P = _lib.ptr
    return timed(lambda: _lib.check(lib.dif_mesh_weld(P(tri), P(std), P(ids), T, ctypes.byref(args), P(ws), ws_bytes, *(P(o) for o in out), _lib.stream_ptr()),
                                    "dif_mesh_weld"), warmup, reps)


def c3_scene(model, frames):
    """the C3 bench stream after `frames` frames -> (stream, intrinsics, the soup of its mesh cache as `weld_ms` takes it, the welded mesh)"""
    from di_fusion_amd.stream import FusionStream
    scene, cfg = syn.config_c3()
    intr = syn.Intrinsic()
    st = FusionStream(model, scene, cfg, intr, DEV, frames, deg_per_frame=0.5)
    for i in range(frames):
        st.step(i)
    st.flush()
    m = st.map
    tri, tid, tstd = (t.clone() for t in m.mesh_cache_tensors())
    soup = (tri, tstd, tid, list(m._cmap.bound_min), float(m._cmap.voxel_size), st.resolution, m.n_xyz)
    return st, intr, soup, M.weld(*soup)


def c3_pose(i):
    Rm, t = syn.orbit_pose(i, 0.3, 0.5)
    pose = np.eye(4)
    pose[:3, :3], pose[:3, 3] = Rm, t
    return pose


def c3_rows(model, frames, warmup, reps):
    st, intr, soup, mesh = c3_scene(model, frames)
    w = weld_ms(soup, warmup, reps)
    rows = []
    for i in sorted({0, frames // 2, frames - 1}):
        row = measure(f"C3 bench stream after {frames} frames, pose of frame {i}", mesh, c3_pose(i), intr, warmup, reps, input_depth=st.depth[i].reshape(intr.height, intr.width))
        row.update(weld_ms_median=w["median"], soup_triangles=int(soup[0].shape[0]))
        rows.append(row)
    return rows


def closeup_row(warmup, reps):
    """An icosphere of 1,280 triangles, radius 0.45, from 0.75 m: it fills the 640x480 image, a triangle spans some 50 pixels."""
    v, n, s, t = R.icosphere(3, 0.45)
    mesh = M.IndexedMesh(*(torch.from_numpy(a).to(DEV) for a in (v, n, s, t)), torch.arange(t.shape[0], dtype=torch.int64, device=DEV), {})
    pose = np.eye(4)
    pose[:3, 3] = (0.0, 0.0, -0.75)
    return measure("close-up: icosphere of 1,280 triangles, r 0.45 from 0.75 m", mesh, pose, syn.Intrinsic(), warmup, reps)


def write_md(path, rows, a):
    with open(path, "w") as f:
        f.write("# `dif_mesh_render`: depth, normal, std and triangle images of an indexed mesh\n\n"
                f"`python tools/bench_raster.py --warmup {a.warmup} --reps {a.reps} --frames {a.frames} --md {path}` on one MI355X.\n\n"
                f"Per view: {a.warmup} warm-up calls, then {a.reps} calls each between its own pair of HIP events (the whole chain: the memset of the counts, "
                "project + z-buffer reset, triangles, large triangles, resolve); median, min and max.  Per launch: mean device time per kernel of one call "
                "as the torch profiler records it over the same number of calls.  `weld` = `dif_mesh_weld` on the soup the mesh came from, same method.  "
                "`large` = share of the drawn triangles whose pixel box exceeds RASTER_THREAD_PIXELS "
                f"({_lib.RASTER_THREAD_PIXELS}) and is walked by a workgroup.  Depth difference: rendered depth against the stream's input depth frame of the "
                "same pose, over the pixels valid in both.\n\n"
                "| view | vertices | triangles | median ms | min | max | pixels hit | drawn | clipped | degenerate | offscreen | large | weld ms | depth diff median / p95 (m) |\n"
                "|---|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|\n")
        for r in rows:
            c = r["counts"]
            dd = f"{r['depth_diff_median_m']} / {r['depth_diff_p95_m']}" if "depth_diff_median_m" in r else "-"
            f.write(f"| {r['name']} | {r['vertices']} | {r['triangles']} | {r['ms_median']} | {r['ms_min']} | {r['ms_max']} | {c['pixels_hit']} ({100 * r['pixels_hit_share']:.1f} %) | "
                    f"{c['drawn']} | {c['clipped']} | {c['degenerate']} | {c['offscreen']} | {c['large']} ({100 * r['large_share']:.2f} %) | {r.get('weld_ms_median', '-')} | {dd} |\n")
        f.write("\nPer launch (microseconds):\n\n| view | " + " | ".join(KERNELS) + " |\n|---|" + "---:|" * len(KERNELS) + "\n")
        for r in rows:
            p = r["per_launch_us"] or {}
            f.write(f"| {r['name']} | " + " | ".join(str(p.get(k, "-")) for k in KERNELS) + " |\n")


KERNELS = ("memset", "k_raster_project", "k_raster_triangles", "k_raster_large", "k_raster_resolve")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--only", choices=["c3", "closeup"], default=None)
    ap.add_argument("--md", default=None, help="also write the tables as markdown")
    a = ap.parse_args()
    rows = []
    if a.only in (None, "c3"):
        rows += c3_rows(net_util.networks_from_arrays(net_util.load_weights_npz()), a.frames, a.warmup, a.reps)
    if a.only in (None, "closeup"):
        rows.append(closeup_row(a.warmup, a.reps))
    for r in rows:
        print(json.dumps(r))
    if a.md:
        write_md(a.md, rows, a)


if __name__ == "__main__":
    main()
