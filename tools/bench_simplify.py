"""Times `dif_mesh_simplify` with HIP events beside `dif_mesh_weld` and `dif_mesh_components` on the same mesh, at the sizes of
profiles/mesh_weld.md — the mesh cache of the C3 bench stream after 20 frames and a lattice sheet of 10^6 triangles — at cells of 2, 4 and 8
lattice steps on the grid `DenseIndexedMap.indexed_mesh(simplify_cell=...)` uses (origin = bound_min - half a lattice step), with the
reduction and the edge census before and after.  `--check` compares every result with the numpy restatement (tests/simplify_ref.py).
Per-launch times: run this under `rocprofv3 --kernel-trace --stats`, one mesh per run (`--only`).
Usage: python tools/bench_simplify.py [--warmup 3] [--reps 20] [--frames 20] [--only c3|sheet] [--check] [--md profiles/mesh_simplify.md]"""
import argparse
import ctypes
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from di_fusion_amd import _lib                                   # noqa: E402
from di_fusion_amd.network import utility as net_util            # noqa: E402
from di_fusion_amd.system import mesh as M                       # noqa: E402
from tests import simplify_ref as S                              # noqa: E402
from tools import bench_weld                                     # noqa: E402
from tools.bench_components import timed, welded                 # noqa: E402

DEV = torch.device("cuda:0")
STEPS = (2, 4, 8)


def census(mesh: M.IndexedMesh):
    t = mesh.topology()
    return dict(components=t.count, edges=int(t.n_edges.sum()), boundary_edges=int(t.n_boundary.sum()), max_edge_use=t.max_edge_use)


def components_ms(mesh: M.IndexedMesh, warmup, reps):
    lib = _lib.load()
    V, K = int(mesh.vertices.shape[0]), int(mesh.triangles.shape[0])
    i32 = dict(dtype=torch.int32, device=DEV)
    ws = torch.empty((int(lib.dif_mesh_components_workspace_bytes(V, K)),), dtype=torch.uint8, device=DEV)
    vc, tc, nv, nt, counts = torch.empty((V,), **i32), torch.empty((K,), **i32), torch.empty((V,), **i32), torch.empty((V,), **i32), torch.zeros((8,), **i32)
    P = _lib.ptr
    return timed(lambda: _lib.check(lib.dif_mesh_components(P(mesh.triangles), K, V, P(ws), ws.numel(), P(vc), P(tc), P(nv), P(nt), P(counts), _lib.stream_ptr()),
                                    "dif_mesh_components"), warmup, reps)


def measure(name, mesh: M.IndexedMesh, weld_ms, bound_min, lattice_step, warmup, reps, check):
    lib = _lib.load()
    V, K = int(mesh.vertices.shape[0]), int(mesh.triangles.shape[0])
    step = np.float32(lattice_step)
    origin = [float(x) for x in np.asarray(bound_min, dtype=np.float32) - step / np.float32(2)]
    ws = torch.empty((int(lib.dif_mesh_simplify_workspace_bytes(V, K)),), dtype=torch.uint8, device=DEV)
    out = [torch.empty_like(getattr(mesh, n)) for n in ("vertices", "normals", "vertex_std", "triangles", "triangle_flatten_id")]
    cluster = torch.empty((V,), dtype=torch.int32, device=DEV)
    counts = torch.zeros((_lib.SIMPLIFY_COUNT,), dtype=torch.int32, device=DEV)
    P = _lib.ptr
    row = dict(name=name, vertices=V, triangles=K, workspace_mb=round(ws.numel() / 2 ** 20, 1), warmup=warmup, reps=reps, weld_ms=weld_ms,
               components_ms=components_ms(mesh, warmup, reps), before=census(mesh), cells=[], checked=bool(check))
    host = mesh.cpu() if check else None
    for n in STEPS:
        cell = float(np.float32(n) * step)
        args = M.simplify_args(cell, origin)

        def call():
            _lib.check(lib.dif_mesh_simplify(P(mesh.vertices), P(mesh.vertex_std), P(mesh.triangles), P(mesh.triangle_flatten_id), V, K, None, None,
                                             ctypes.byref(args), P(ws), ws.numel(), P(out[0]), P(out[1]), P(out[2]), P(out[3]), P(out[4]), None, P(cluster),
                                             P(counts), _lib.stream_ptr()), "dif_mesh_simplify")

        t = timed(call, warmup, reps)
        small = M.simplify(mesh.vertices, mesh.vertex_std, mesh.triangles, mesh.triangle_flatten_id, cell, origin)
        c = small.counts
        assert c["status"] == 0 and counts.cpu().tolist()[:9] == [c[k] for k in M.SIMPLIFY_COUNT_NAMES], c
        if check:
            want = S.simplify(host.vertices.numpy(), host.vertex_std.numpy(), host.triangles.numpy(), host.triangle_flatten_id.numpy(), cell, origin)
            g = small.cpu()
            assert [c[k] for k in S.COUNT_NAMES] == want["counts"], (c, want["counts"])
            for k in S.MESH_NAMES + ("vertex_cluster",):
                assert getattr(g, k).numpy().tobytes() == np.ascontiguousarray(want[k]).tobytes(), k
        row["cells"].append(dict(lattice_steps=n, cell=cell, ms=t, counts={k: c[k] for k in M.SIMPLIFY_COUNT_NAMES}, vertex_ratio=round(c["vertices"] / V, 4),
                                 triangle_ratio=round(c["triangles"] / K, 4), after=census(small)))
    return row


def write_md(path, rows, a):
    def cell(t):
        return "-" if t is None else f"{t['median']} ({t['min']} - {t['max']})"
    with open(path, "w") as f:
        f.write("# Simplifying an indexed mesh by vertex clustering\n\n"
                f"`python tools/bench_simplify.py --warmup {a.warmup} --reps {a.reps} --frames {a.frames}{' --check' if a.check else ''} --md profiles/mesh_simplify.md` "
                "on one MI355X.\n\n"
                f"Per mesh and cell: {a.warmup} warm-up calls, then {a.reps} calls each between its own pair of HIP events (the whole launch chain of "
                "`dif_mesh_simplify` into preallocated outputs, no read-back, no colours); median (min - max) in ms.  The grid is the one "
                "`DenseIndexedMap.indexed_mesh(simplify_cell=...)` uses: origin = bound_min - half a lattice step.  weld = `mesh.weld` on the soup the mesh came "
                "from, WITH its allocations and the read-back of its counts (profiles/mesh_weld.md has the bare chain); components = `dif_mesh_components` of the "
                "same mesh, bare.  Edge census (`IndexedMesh.topology()`): distinct edges / boundary edges (named by one triangle) / the most triangles on one edge.\n\n")
        for r in rows:
            b = r["before"]
            f.write(f"## {r['name']}\n\n{r['vertices']} vertices, {r['triangles']} triangles, {b['components']} components; edges {b['edges']} / {b['boundary_edges']} / "
                    f"{b['max_edge_use']}.  weld {cell(r['weld_ms'])} ms, components {cell(r['components_ms'])} ms.  Workspace {r['workspace_mb']} MiB.\n\n"
                    "| cell (lattice steps) | simplify, ms | vertices (ratio) | triangles (ratio) | collapsed | duplicate | isolated | flat | components | edges / boundary / max use |\n"
                    "|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|\n")
            for c in r["cells"]:
                k, e = c["counts"], c["after"]
                f.write(f"| {c['lattice_steps']} | {cell(c['ms'])} | {k['vertices']} ({c['vertex_ratio']}) | {k['triangles']} ({c['triangle_ratio']}) | {k['collapsed']} | "
                        f"{k['duplicate']} | {k['isolated']} | {k['flat']} | {e['components']} | {e['edges']} / {e['boundary_edges']} / {e['max_edge_use']} |\n")
            f.write("\n")
        if a.check:
            f.write("Every result compared with the numpy restatement (`--check`: all arrays and counts, byte for byte).\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--only", default=None, choices=("c3", "sheet"))
    ap.add_argument("--check", action="store_true", help="compare with the numpy restatement")
    ap.add_argument("--md", default=None, help="also write the tables as markdown")
    a = ap.parse_args()
    rows = []
    if a.only in (None, "c3"):
        model = net_util.networks_from_arrays(net_util.load_weights_npz())
        soup = bench_weld.c3_soup(model, a.frames)
        mesh, t = welded(soup, a.warmup, a.reps)
        rows.append(measure(f"C3 bench stream, cache after {a.frames} frames", mesh, t, soup[3], soup[4] / soup[5], a.warmup, a.reps, a.check))
    if a.only in (None, "sheet"):
        soup = bench_weld.sheet(1000000)
        mesh, t = welded(soup, a.warmup, a.reps)
        rows.append(measure("lattice sheet, 10^6 triangles", mesh, t, soup[3], soup[4] / soup[5], a.warmup, a.reps, a.check))
    for r in rows:
        print(json.dumps(r))
    if a.md:
        write_md(a.md, rows, a)


if __name__ == "__main__":
    main()
