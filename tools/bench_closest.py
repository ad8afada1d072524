"""Times `dif_mesh_locator_build` and `dif_mesh_closest` with HIP events on the mesh cache of the C3 bench stream after 20 frames (the mesh of
profiles/mesh_weld.md), beside the weld of the same mesh in the same run: the build; the query for (i) the mesh's own vertices and (ii) the
points of the stream's last depth frame (in image order, NaN where the depth is invalid); the same two queries with every triangle on the
large list (`max_cells=-1`: the all-pairs search, the floor the grid has to beat); and `simplify(cell)` at 2 / 4 / 8 lattice steps measured
both ways with `distance_to` (on the grid `DenseIndexedMap.indexed_mesh(simplify_cell=...)` uses, as tools/bench_simplify.py).  `--check`
compares a sample of the queries with the numpy restatement (tests/closest_ref.py), and the grid answers with the all-pairs answers in full.
Per-launch times: run this under `rocprofv3 --kernel-trace --stats`.
Usage: python tools/bench_closest.py [--warmup 2] [--reps 10] [--frames 20] [--max-distance-cells 4] [--check] [--md profiles/mesh_closest.md]"""
import argparse
import ctypes
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from di_fusion_amd import _lib, synthetic as syn                 # noqa: E402
from di_fusion_amd.network import utility as net_util            # noqa: E402
from di_fusion_amd.system import mesh as M                       # noqa: E402
from tests import closest_ref as R                               # noqa: E402
from tools.bench_components import timed, welded                 # noqa: E402

DEV = torch.device("cuda:0")
STEPS = (2, 4, 8)
OUT_NAMES = ("d2", "triangle", "point", "barycentric")
NOTES = "## What the numbers say"        # write_md keeps the file from this heading on


def c3_stream(model, frames):
    """The C3 bench stream after `frames` eager frames: its soup (as tools/bench_weld.py:c3_soup) and the world points of the last depth frame."""
    from di_fusion_amd.stream import FusionStream
    scene, cfg = syn.config_c3()
    st = FusionStream(model, scene, cfg, syn.Intrinsic(), DEV, frames, deg_per_frame=0.5)
    for i in range(frames):
        st.step(i)
    st.flush()
    m = st.map
    tri, tid, tstd = (t.clone() for t in m.mesh_cache_tensors())
    return (tri, tstd, tid, list(m._cmap.bound_min), float(m._cmap.voxel_size), st.resolution, m.n_xyz), st.xyz.clone()


def build_ms(mesh: M.IndexedMesh, loc: M.MeshLocator, warmup, reps):
    """The bare launch chain of the build into the locator's own workspace (same cell, same capacity)."""
    lib = _lib.load()
    V, K = int(mesh.vertices.shape[0]), int(mesh.triangles.shape[0])
    counts = torch.empty((_lib.LOCATOR_COUNT,), dtype=torch.int32, device=DEV)
    P = _lib.ptr
    return timed(lambda: _lib.check(lib.dif_mesh_locator_build(P(mesh.vertices), P(mesh.triangles), V, K, ctypes.byref(loc.args), P(loc.workspace), loc.workspace.numel(),
                                                               P(counts), _lib.stream_ptr()), "dif_mesh_locator_build"), warmup, reps)


def query_ms(loc: M.MeshLocator, points, r, warmup, reps):
    """The bare query launch into preallocated outputs, no read-back."""
    lib = _lib.load()
    N = int(points.shape[0])
    f32 = dict(dtype=torch.float32, device=DEV)
    d2, tri, pt, bc = torch.empty((N,), **f32), torch.empty((N,), dtype=torch.int32, device=DEV), torch.empty((N, 3), **f32), torch.empty((N, 3), **f32)
    counts = torch.empty((_lib.CLOSEST_COUNT,), dtype=torch.int32, device=DEV)
    P = _lib.ptr
    return timed(lambda: _lib.check(lib.dif_mesh_closest(ctypes.byref(loc.args), loc.n_triangles, P(loc.workspace), loc.workspace.numel(), P(points), N,
                                                         int(points.shape[1]), r, P(d2), P(tri), P(pt), P(bc), P(counts), _lib.stream_ptr()), "dif_mesh_closest"), warmup, reps)


def same(a: M.MeshClosest, b: M.MeshClosest):
    return a.counts == b.counts and all(torch.equal(getattr(a, k).view(torch.int32), getattr(b, k).view(torch.int32)) for k in OUT_NAMES)


def distance_row(a: M.IndexedMesh, b: M.IndexedMesh, r):
    d = a.distance_to(b, r)
    return {k: (round(d[k], 6) if isinstance(d[k], float) else d[k]) for k in ("mean", "rms", "max", "median", "found", "far")}


def measure(name, mesh: M.IndexedMesh, weld_ms, frame_points, bound_min, lattice_step, a):
    V, K = int(mesh.vertices.shape[0]), int(mesh.triangles.shape[0])
    loc = mesh.locator()
    cell = loc.counts["cell"]
    r = float(np.float32(a.max_distance_cells * cell))
    floor_loc = M.locator(mesh.vertices, mesh.triangles, cell, max_cells=-1)
    row = dict(name=name, vertices=V, triangles=K, warmup=a.warmup, reps=a.reps, weld_ms=weld_ms, cell=cell, max_distance=r, build_counts=loc.counts,
               workspace_mb=round(loc.workspace.numel() / 2 ** 20, 1), build_ms=build_ms(mesh, loc, a.warmup, a.reps), queries=[], simplify=[], checked=bool(a.check))
    for what, pts in (("own vertices", mesh.vertices), ("depth frame", frame_points)):
        grid = loc.closest(pts, r)
        q = dict(points=what, n=int(pts.shape[0]), counts=grid.counts, grid_ms=query_ms(loc, pts, r, a.warmup, a.reps),
                 all_pairs_ms=query_ms(floor_loc, pts, r, 1, max(2, a.reps // 4)))
        found = torch.isfinite(grid.d2)
        q["median_distance"] = round(float(torch.sqrt(grid.d2[found]).median()), 6) if bool(found.any()) else None
        if a.check:
            assert same(grid, floor_loc.closest(pts, r)), what                    # the grid against the all-pairs search, in full
            pick = torch.arange(0, int(pts.shape[0]), max(1, int(pts.shape[0]) // 64), device=DEV)[:64]
            h = mesh.cpu()
            want = R.closest(h.vertices.numpy(), h.triangles.numpy(), pts[pick].cpu().numpy(), r, cell)
            for k in OUT_NAMES:
                assert getattr(grid, k)[pick].cpu().numpy().tobytes() == want[k].tobytes(), (what, k)
        row["queries"].append(q)
    step = np.float32(lattice_step)
    origin = [float(x) for x in np.asarray(bound_min, dtype=np.float32) - step / np.float32(2)]      # the grid of `indexed_mesh(simplify_cell=...)`
    for n in STEPS:
        c = float(np.float32(n) * step)
        small = mesh.simplify(c, origin)
        rr = float(np.float32(2.0 * c))
        row["simplify"].append(dict(lattice_steps=n, cell=c, vertices=int(small.vertices.shape[0]), triangles=int(small.triangles.shape[0]), max_distance=rr,
                                    simplified_to_full=distance_row(small, mesh, rr), full_to_simplified=distance_row(mesh, small, rr)))
    return row


def write_md(path, rows, a):
    def cell(t):
        return "-" if t is None else f"{t['median']} ({t['min']} - {t['max']})"
    notes = ""
    if Path(path).exists():                                                     # the hand-written reading of the numbers stays with the file
        old = Path(path).read_text()
        notes = old[old.index(NOTES):] if NOTES in old else ""
    with open(path, "w") as f:
        f.write("# Closest point on an indexed mesh\n\n"
                f"`python tools/bench_closest.py --warmup {a.warmup} --reps {a.reps} --frames {a.frames} --max-distance-cells {a.max_distance_cells}"
                f"{' --check' if a.check else ''} --md profiles/mesh_closest.md` on one MI355X.\n\n"
                f"Per call: {a.warmup} warm-up calls, then {a.reps} calls each between its own pair of HIP events (the bare launch chain into preallocated "
                "outputs, no read-back; the all-pairs search: 1 warm-up and a quarter of the calls); median (min - max) in ms.  weld = `mesh.weld` on the soup the "
                "mesh came from, WITH its allocations and the read-back of its counts.  The cell is the default one (twice the mean longest box side of the "
                "triangles); max_distance is that many cells.  all pairs = the same query with every triangle on the large list (`max_cells=-1`).\n\n")
        for r in rows:
            c = r["build_counts"]
            f.write(f"## {r['name']}\n\n{r['vertices']} vertices, {r['triangles']} triangles.  weld {cell(r['weld_ms'])} ms.  Cell {r['cell']:.6f}, max_distance "
                    f"{r['max_distance']:.6f}.  Locator: {c['indexed']} indexed, {c['large']} large, {c['degenerate']} degenerate, {c['skipped']} skipped, "
                    f"{c['pairs']} pairs in {c['cells']} cells, workspace {r['workspace_mb']} MiB; build {cell(r['build_ms'])} ms.\n\n"
                    "| query points | N | found | far | bad | median distance | grid, ms | all pairs, ms |\n|---|---:|---:|---:|---:|---:|---:|---:|\n")
            for q in r["queries"]:
                k = q["counts"]
                f.write(f"| {q['points']} | {q['n']} | {k['found']} | {k['far']} | {k['bad_point']} | {q['median_distance']} | {cell(q['grid_ms'])} | "
                        f"{cell(q['all_pairs_ms'])} |\n")
            f.write("\n`simplify(cell)` measured with `distance_to` (vertices of the first against the surface of the second, max_distance = two cells; "
                    "metres):\n\n| cell (lattice steps) | vertices | triangles | direction | mean | rms | median | max | far |\n|---:|---:|---:|---|---:|---:|---:|---:|---:|\n")
            for s in r["simplify"]:
                for name, key in (("simplified -> full", "simplified_to_full"), ("full -> simplified", "full_to_simplified")):
                    d = s[key]
                    f.write(f"| {s['cell']:.5f} ({s['lattice_steps']}) | {s['vertices']} | {s['triangles']} | {name} | {d['mean']} | {d['rms']} | {d['median']} | "
                            f"{d['max']} | {d['far']} |\n")
            f.write("\n")
        if a.check:
            f.write("Checked (`--check`): every grid answer equals the all-pairs answer bit for bit, and 64 queries of each set equal the numpy restatement.\n")
        if notes:
            f.write("\n" + notes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--max-distance-cells", type=float, default=4.0)
    ap.add_argument("--check", action="store_true", help="compare with the all-pairs search (in full) and the numpy restatement (a sample)")
    ap.add_argument("--md", default=None, help="also write the tables as markdown")
    a = ap.parse_args()
    model = net_util.networks_from_arrays(net_util.load_weights_npz())
    soup, frame_points = c3_stream(model, a.frames)
    mesh, t = welded(soup, a.warmup, a.reps)
    rows = [measure(f"C3 bench stream, cache after {a.frames} frames", mesh, t, frame_points, soup[3], soup[4] / soup[5], a)]
    for r in rows:
        print(json.dumps(r))
    if a.md:
        write_md(a.md, rows, a)


if __name__ == "__main__":
    main()
