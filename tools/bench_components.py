"""Times `dif_mesh_components`, `dif_mesh_edge_census` and `dif_mesh_select` with HIP events beside `dif_mesh_weld` on the same mesh, at the sizes
of profiles/mesh_weld.md — the mesh cache of the C3 bench stream after 20 frames and a lattice sheet of 10^6 triangles (both: a few giant
components) — and on 333,334 disjoint triangles (10^6 vertices: as many components as triangles).  `--check` compares every result with the numpy
restatement (tests/components_ref.py; tens of seconds of host time at these sizes).  Per-launch times: run this under
`rocprofv3 --kernel-trace --stats`, one mesh per run (`--only`).
Usage: python tools/bench_components.py [--warmup 3] [--reps 20] [--frames 20] [--only c3|sheet|disjoint] [--md profiles/mesh_components.md]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from di_fusion_amd import _lib                                   # noqa: E402
from di_fusion_amd.network import utility as net_util            # noqa: E402
from di_fusion_amd.system import mesh as M                       # noqa: E402
from tests import components_ref as C                            # noqa: E402
from tools import bench_weld                                     # noqa: E402

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


def measure(name, mesh: M.IndexedMesh, weld_ms, min_triangles, warmup, reps, check):
    lib = _lib.load()
    V, K = int(mesh.vertices.shape[0]), int(mesh.triangles.shape[0])
    i32 = dict(dtype=torch.int32, device=DEV)
    ws = torch.empty((max(int(lib.dif_mesh_components_workspace_bytes(V, K)), int(lib.dif_mesh_select_workspace_bytes(V, K)),
                          int(lib.dif_mesh_edge_census_workspace_bytes(K))),), dtype=torch.uint8, device=DEV)
    vc, tc, nv, nt = torch.empty((V,), **i32), torch.empty((K,), **i32), torch.empty((V,), **i32), torch.empty((V,), **i32)
    ne, nb = torch.empty((V,), **i32), torch.empty((V,), **i32)
    counts = torch.zeros((8,), **i32)
    out = [torch.empty_like(getattr(mesh, n)) for n in ("vertices", "normals", "vertex_std", "triangles", "triangle_flatten_id")]
    P, S = _lib.ptr, _lib.stream_ptr

    def comp():
        _lib.check(lib.dif_mesh_components(P(mesh.triangles), K, V, P(ws), ws.numel(), P(vc), P(tc), P(nv), P(nt), P(counts), S()), "dif_mesh_components")

    t_comp = timed(comp, warmup, reps)
    n_comp, status = counts.cpu().tolist()[:2]
    assert status == 0, status
    sizes = nt[:n_comp].clone()

    def edges():
        _lib.check(lib.dif_mesh_edge_census(P(mesh.triangles), K, V, P(vc), n_comp, P(ws), ws.numel(), P(ne), P(nb), P(counts), S()), "dif_mesh_edge_census")

    t_edge = timed(edges, warmup, reps)
    max_use, status = counts.cpu().tolist()[:2]
    assert status == 0, status
    keep = (sizes >= min_triangles)[tc.long()].view(torch.uint8)

    def select():
        _lib.check(lib.dif_mesh_select(*(P(getattr(mesh, n)) for n in ("vertices", "normals", "vertex_std", "triangles", "triangle_flatten_id")), V, K, P(keep),
                                       P(ws), ws.numel(), *(P(o) for o in out), P(counts), S()), "dif_mesh_select")

    t_sel = timed(select, warmup, reps)
    kept_v, kept_k, status = counts.cpu().tolist()[:3]
    assert status == 0, status
    if check:
        want = C.topology(mesh.triangles.cpu().numpy(), V)
        assert want["count"] == n_comp and np.array_equal(want["vertex_component"], vc.cpu().numpy()) and np.array_equal(want["n_triangles"], sizes.cpu().numpy())
        assert np.array_equal(want["n_edges"], ne[:n_comp].cpu().numpy()) and np.array_equal(want["n_boundary"], nb[:n_comp].cpu().numpy())
        assert want["max_edge_use"] == max_use
    return dict(name=name, vertices=V, triangles=K, components=n_comp, largest=int(sizes.max()) if n_comp else 0, max_edge_use=max_use,
                boundary_edges=int(nb[:n_comp].sum()), min_triangles=min_triangles, kept_vertices=kept_v, kept_triangles=kept_k, warmup=warmup, reps=reps,
                weld_ms=weld_ms, components_ms=t_comp, edge_census_ms=t_edge, select_ms=t_sel, checked=bool(check))


def welded(soup, warmup, reps):
    tri, std, ids, bm, vs, r, n_xyz = soup
    t = timed(lambda: M.weld(tri, std, ids, bm, vs, r, n_xyz), warmup, reps)        # (with its allocations and the read-back of its counts)
    return M.weld(tri, std, ids, bm, vs, r, n_xyz), t


def disjoint_mesh(n):
    tris, V = C.disjoint(n)
    z = torch.zeros((V, 3), dtype=torch.float32, device=DEV)
    return M.IndexedMesh(z, z.clone(), torch.zeros((V,), dtype=torch.float32, device=DEV), torch.from_numpy(tris).to(DEV),
                         torch.arange(n, dtype=torch.int64, device=DEV), {})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--only", default=None, choices=("c3", "sheet", "disjoint"))
    ap.add_argument("--check", action="store_true", help="compare with the numpy restatement (a Python union-find: tens of seconds at these sizes)")
    ap.add_argument("--md", default=None, help="also write the table as markdown")
    a = ap.parse_args()
    rows = []
    if a.only in (None, "c3"):
        model = net_util.networks_from_arrays(net_util.load_weights_npz())
        mesh, t = welded(bench_weld.c3_soup(model, a.frames), a.warmup, a.reps)
        rows.append(measure(f"C3 bench stream, cache after {a.frames} frames", mesh, t, 500, a.warmup, a.reps, a.check))
    if a.only in (None, "sheet"):
        mesh, t = welded(bench_weld.sheet(1000000), a.warmup, a.reps)
        rows.append(measure("lattice sheet, 10^6 triangles", mesh, t, 500, a.warmup, a.reps, a.check))
    if a.only in (None, "disjoint"):
        rows.append(measure("333,334 disjoint triangles", disjoint_mesh(333334), None, 1, a.warmup, a.reps, a.check))
    for r in rows:
        print(json.dumps(r))
    if a.md:
        with open(a.md, "w") as f:
            f.write("# Components, edge census and selection of an indexed mesh\n\n"
                    f"`python tools/bench_components.py --warmup {a.warmup} --reps {a.reps} --frames {a.frames} --md profiles/mesh_components.md` on one MI355X.\n\n"
                    f"Per mesh and entry point: {a.warmup} warm-up calls, then {a.reps} calls each between its own pair of HIP events (the whole launch chain "
                    "into preallocated outputs, no read-back); median (min - max) in ms.  weld = `mesh.weld` on the soup the mesh came from, timed the same "
                    "way but WITH its allocations and the read-back of its counts (profiles/mesh_weld.md has the bare chain).  select = the mask of "
                    "`remove_small_components(min_triangles)`.\n\n"
                    "| mesh | vertices | triangles | components | largest | boundary edges | max edge use | weld | components | edge census | select (kept triangles) |\n"
                    "|---|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|\n")
            for r in rows:
                def cell(t):
                    return "-" if t is None else f"{t['median']} ({t['min']} - {t['max']})"
                f.write(f"| {r['name']} | {r['vertices']} | {r['triangles']} | {r['components']} | {r['largest']} | {r['boundary_edges']} | {r['max_edge_use']} | "
                        f"{cell(r['weld_ms'])} | {cell(r['components_ms'])} | {cell(r['edge_census_ms'])} | {cell(r['select_ms'])} ({r['kept_triangles']}) |\n")


if __name__ == "__main__":
    main()
