"""Times `dif_mesh_weld` (indexed mesh from the triangle soup: weld by lattice edge + vertex normals) with HIP events at three sizes: the sphere
map of the tests, the mesh cache of the C3 bench stream after 20 frames, and a tiled lattice sheet of 10^6 triangles.  Beside each: the host
time of the numpy restatement (tests/weld_ref.py) on the same soup, and the algorithmic traffic (soup read once, mesh written once).
Usage: python tools/bench_weld.py [--warmup 3] [--reps 20] [--frames 20] [--md profiles/mesh_weld.md]"""
import argparse
import ctypes
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from di_fusion_amd import _lib, synthetic as syn                 # noqa: E402
from di_fusion_amd.network import utility as net_util            # noqa: E402
from di_fusion_amd.system import mesh as M                       # noqa: E402
from di_fusion_amd.system.map import DenseIndexedMap             # noqa: E402
from tests import weld_ref as W                                  # noqa: E402

DEV = torch.device("cuda:0")


def sphere_soup(model):
    b = W.SPHERE_BOUND
    cfg = syn.MapConfig((-b, -b, -b), (b, b, b), W.SPHERE_VOXEL)
    m = DenseIndexedMap(model, cfg.namespace(), 29, DEV, initial_capacity=1024)
    xyz, nrm = W.sphere_cloud()
    m.integrate_keyframe(torch.from_numpy(xyz).to(DEV), torch.from_numpy(nrm).to(DEV))
    m.extract_mesh_arrays(W.SPHERE_RES, int(4e6), fast=True, max_std=2000.0, to_host=False)
    tri, tid, tstd = (t.clone() for t in m.mesh_cache_tensors())
    return tri, tstd, tid, list(m._cmap.bound_min), float(m._cmap.voxel_size), W.SPHERE_RES, m.n_xyz


def c3_soup(model, frames):
    from di_fusion_amd.stream import FusionStream
    scene, cfg = syn.config_c3()
    st = FusionStream(model, scene, cfg, syn.Intrinsic(), DEV, frames, deg_per_frame=0.5)
    for i in range(frames):
        st.step(i)
    st.flush()
    m = st.map
    tri, tid, tstd = (t.clone() for t in m.mesh_cache_tensors())
    return tri, tstd, tid, list(m._cmap.bound_min), float(m._cmap.voxel_size), st.resolution, m.n_xyz


def sheet(T):
    bm, vs, r = (-3.2, -3.2, -3.2), 0.05, 4
    tri, std, ids = W.sheet_soup(T, r=r, voxel_size=vs, bound_min=bm, width=1000)
    return torch.from_numpy(tri).to(DEV), torch.from_numpy(std).to(DEV), torch.from_numpy(ids).to(DEV), list(bm), vs, r, None


def measure(name, soup, warmup, reps):
    tri, std, ids, bm, vs, r, n_xyz = soup
    T = int(tri.shape[0])
    lib = _lib.load()
    args = M.weld_args(bm, vs, r, n_xyz)
    ws_bytes = int(lib.dif_mesh_weld_workspace_bytes(T))
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=DEV)
    out_v = torch.empty((3 * T, 3), dtype=torch.float32, device=DEV)
    out_n = torch.empty((3 * T, 3), dtype=torch.float32, device=DEV)
    out_s = torch.empty((3 * T,), dtype=torch.float32, device=DEV)
    out_t = torch.empty((T, 3), dtype=torch.int32, device=DEV)
    out_i = torch.empty((T,), dtype=torch.int64, device=DEV)
    counts = torch.empty((_lib.WELD_COUNT,), dtype=torch.int32, device=DEV)

    def call():
        _lib.check(lib.dif_mesh_weld(_lib.ptr(tri), _lib.ptr(std), _lib.ptr(ids), T, ctypes.byref(args), _lib.ptr(ws), ws_bytes, _lib.ptr(out_v),
                                     _lib.ptr(out_n), _lib.ptr(out_s), _lib.ptr(out_t), _lib.ptr(out_i), _lib.ptr(counts), _lib.stream_ptr()),
                   "dif_mesh_weld")

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
    c = counts.cpu().tolist()
    V, K = c[_lib.WELD_VERTICES], c[_lib.WELD_KEPT]
    t0 = time.perf_counter()
    ref = W.weld(tri.cpu().numpy(), std.cpu().numpy(), ids.cpu().numpy(), bm, vs, r)
    host_s = time.perf_counter() - t0
    assert ref["counts"].tolist() == c[:5], (ref["counts"].tolist(), c)
    assert np.array_equal(ref["triangles"], out_t[:K].cpu().numpy())
    traffic = T * (36 + 12 + 8) + V * (12 + 12 + 4) + K * (12 + 8)
    med = statistics.median(ms)
    return dict(name=name, triangles=T, vertices=V, kept=K, dropped=c[_lib.WELD_DROPPED], unkeyed=c[_lib.WELD_UNKEYED], warmup=warmup, reps=reps,
                ms_median=round(med, 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4), traffic_bytes=traffic,
                gb_per_s=round(traffic / med / 1e6, 1), workspace_bytes=ws_bytes, host_numpy_ms=round(host_s * 1e3, 1),
                speedup_over_host=round(host_s * 1e3 / med, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--md", default=None, help="also write the table as markdown")
    a = ap.parse_args()
    model = net_util.networks_from_arrays(net_util.load_weights_npz())
    rows = [measure("sphere map (r 0.45, voxel 0.1, resolution 4)", sphere_soup(model), a.warmup, a.reps),
            measure(f"C3 bench stream, cache after {a.frames} frames", c3_soup(model, a.frames), a.warmup, a.reps),
            measure("lattice sheet, 10^6 triangles", sheet(1000000), a.warmup, a.reps)]
    for r in rows:
        print(json.dumps(r))
    if a.md:
        with open(a.md, "w") as f:
            f.write("# `dif_mesh_weld`: indexed mesh from the triangle soup\n\n"
                    f"`python tools/bench_weld.py --warmup {a.warmup} --reps {a.reps} --frames {a.frames} --md profiles/mesh_weld.md` on one MI355X.\n\n"
                    f"Per size: {a.warmup} warm-up calls, then {a.reps} calls each between its own pair of HIP events (the whole launch chain: two memsets, "
                    "insert, vertex scan, corner map, triangle scan with the normal sums, normalise); median, min and max of those.  Traffic = the "
                    "algorithmic minimum: the soup read once (56 B per triangle), the mesh written once (28 B per vertex, 20 B per kept triangle); the "
                    "class table and the per-corner scratch (`workspace`) are on top of that and are what the time really goes to.  Host = the numpy "
                    "restatement `tests/weld_ref.py::weld` on the same soup, one run, same counts and triangle indices asserted.\n\n"
                    "| soup | triangles | vertices | kept | dropped | unkeyed | median ms | min | max | GB/s | workspace MB | host numpy ms | speed-up |\n"
                    "|---|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|\n")
            for r in rows:
                f.write(f"| {r['name']} | {r['triangles']} | {r['vertices']} | {r['kept']} | {r['dropped']} | {r['unkeyed']} | {r['ms_median']} | {r['ms_min']} | "
                        f"{r['ms_max']} | {r['gb_per_s']} | {r['workspace_bytes'] / 2**20:.1f} | {r['host_numpy_ms']} | {r['speedup_over_host']}x |\n")


if __name__ == "__main__":
    main()
