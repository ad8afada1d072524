"""Times `dif_mesh_sampler_build` and `dif_mesh_sample` with HIP events on the mesh cache of the C3 bench stream after 20 frames (the mesh of
profiles/mesh_weld.md) and on a lattice sheet of 10^6 triangles, beside the weld of the same mesh in the same run: the build; `sample` at N = 10^5
and 10^6; the same draws from a sampler over ONE triangle (the hash, the strata's divisions and the stores: everything but the search over P and the
scattered gather of the chosen triangles — the difference bounds the search's share from above); `IndexedMesh.compare` end to end; and `simplify(cell)`
at 2 / 4 / 8 lattice steps measured with `compare` (area-sampled, both ways) beside `distance_to` (vertex-sampled).  `--check` compares the build and
a draw with the numpy restatement (tests/sample_ref.py).
Usage: python tools/bench_sample.py [--warmup 3] [--reps 20] [--frames 20] [--only c3|sheet] [--check] [--md profiles/mesh_sample.md]"""
import argparse
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
from tests import sample_ref as R                                # noqa: E402
from tools import bench_weld                                     # noqa: E402
from tools.bench_components import timed, welded                 # noqa: E402

DEV = torch.device("cuda:0")
STEPS = (2, 4, 8)
DRAWS = (100_000, 1_000_000)
NOTES = "## What the numbers say"        # write_md keeps the file from this heading on


def build_ms(smp: M.MeshSampler, warmup, reps):
    """The bare launch chain of the build into the sampler's own workspace."""
    lib = _lib.load()
    V, K = int(smp.vertices.shape[0]), int(smp.triangles.shape[0])
    counts = torch.empty((_lib.SAMPLER_COUNT,), dtype=torch.int32, device=DEV)
    total = torch.empty((1,), dtype=torch.int64, device=DEV)
    P = _lib.ptr
    return timed(lambda: _lib.check(lib.dif_mesh_sampler_build(P(smp.vertices), P(smp.triangles), V, K, P(smp.workspace), smp.workspace.numel(), P(counts), P(total),
                                                               _lib.stream_ptr()), "dif_mesh_sampler_build"), warmup, reps)


def sample_ms(smp: M.MeshSampler, N, warmup, reps):
    """The bare draw into preallocated outputs, no read-back."""
    lib = _lib.load()
    V, K = int(smp.vertices.shape[0]), int(smp.triangles.shape[0])
    f32 = dict(dtype=torch.float32, device=DEV)
    pt, tri, bc = torch.empty((N, 3), **f32), torch.empty((N,), dtype=torch.int32, device=DEV), torch.empty((N, 3), **f32)
    counts = torch.empty((_lib.SAMPLE_COUNT,), dtype=torch.int32, device=DEV)
    P = _lib.ptr
    return timed(lambda: _lib.check(lib.dif_mesh_sample(P(smp.vertices), P(smp.triangles), V, K, P(smp.workspace), smp.workspace.numel(), N, 1, P(pt), P(tri), P(bc),
                                                        P(counts), _lib.stream_ptr()), "dif_mesh_sample"), warmup, reps)


def rounded(d):
    return {k: (round(v, 6) if isinstance(v, float) else v) for k, v in d.items() if k != "d2"}


def measure(name, mesh: M.IndexedMesh, weld_ms, bound_min, lattice_step, a):
    V, K = int(mesh.vertices.shape[0]), int(mesh.triangles.shape[0])
    smp = mesh.sampler()
    one = M.sampler(torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], device=DEV), torch.tensor([[0, 1, 2]], dtype=torch.int32, device=DEV))
    row = dict(name=name, vertices=V, triangles=K, warmup=a.warmup, reps=a.reps, weld_ms=weld_ms, counts=smp.counts, total=smp.total, area=smp.area,
               workspace_mb=round(smp.workspace.numel() / 2 ** 20, 1), build_ms=build_ms(smp, a.warmup, a.reps), draws=[], simplify=[], checked=bool(a.check))
    for N in DRAWS:
        row["draws"].append(dict(n=N, sample_ms=sample_ms(smp, N, a.warmup, a.reps), one_triangle_ms=sample_ms(one, N, a.warmup, a.reps)))
    if a.check:
        h = mesh.cpu()
        b = R.build(h.vertices.numpy(), h.triangles.numpy())
        assert [smp.counts[k] for k in R.BUILD_NAMES] == b["counts"] and smp.total == b["total"], (smp.counts, b["counts"])
        got, want = smp.sample(DRAWS[0], 1).cpu(), R.sample(h.vertices.numpy(), h.triangles.numpy(), DRAWS[0], 1, b=b)
        for k in ("point", "triangle", "barycentric"):
            assert getattr(got, k).numpy().tobytes() == want[k].tobytes(), k
    step = np.float32(lattice_step)
    origin = [float(x) for x in np.asarray(bound_min, dtype=np.float32) - step / np.float32(2)]      # the grid of `indexed_mesh(simplify_cell=...)`
    for n in STEPS:
        c = float(np.float32(n) * step)
        small = mesh.simplify(c, origin)
        rr = float(np.float32(2.0 * c))
        taus = (float(step), rr)
        cmp = small.compare(mesh, rr, n_samples=DRAWS[0], thresholds=taus)
        s = dict(lattice_steps=n, cell=c, vertices=int(small.vertices.shape[0]), triangles=int(small.triangles.shape[0]), max_distance=rr, area=small.sampler().area,
                 compare_ms=timed(lambda: small.compare(mesh, rr, n_samples=DRAWS[0], thresholds=taus), 1, max(3, a.reps // 4)),
                 accuracy=rounded(cmp["accuracy"]), completeness=rounded(cmp["completeness"]), chamfer=round(cmp["chamfer"], 6), thresholds=taus,
                 fscore=[round(x, 4) for x in cmp["fscore"]],
                 vertex_simplified_to_full=rounded(small.distance_to(mesh, rr)), vertex_full_to_simplified=rounded(mesh.distance_to(small, rr)))
        row["simplify"].append(s)
    return row


def write_md(path, rows, a):
    def cell(t):
        return "-" if t is None else f"{t['median']} ({t['min']} - {t['max']})"
    notes = ""
    if Path(path).exists():                                                     # the hand-written reading of the numbers stays with the file
        old = Path(path).read_text()
        notes = old[old.index(NOTES):] if NOTES in old else ""
    with open(path, "w") as f:
        f.write("# Sampling and comparing indexed meshes\n\n"
                f"`python tools/bench_sample.py --warmup {a.warmup} --reps {a.reps} --frames {a.frames}{' --check' if a.check else ''} --md profiles/mesh_sample.md` "
                "on one MI355X.\n\n"
                f"Per call: {a.warmup} warm-up calls, then {a.reps} calls each between its own pair of HIP events; median (min - max) in ms.  build and sample: the "
                "bare launch chain into preallocated outputs, no read-back.  one triangle = the same draw from a sampler over a single triangle: the hash, the "
                "strata and the stores without a search over P or a scattered gather.  weld = `mesh.weld` on the soup the mesh came from, WITH its allocations "
                "and the read-back of its counts.  compare = `IndexedMesh.compare` end to end with 10^5 samples per side: two sampler builds, two draws, two "
                "locator builds, two closest queries, the float64 reductions, every allocation and read-back (1 warm-up, a quarter of the calls).\n\n")
        for r in rows:
            c = r["counts"]
            f.write(f"## {r['name']}\n\n{r['vertices']} vertices, {r['triangles']} triangles, area {r['area']:.6f}.  weld {cell(r['weld_ms'])} ms.  Sampler: "
                    f"{c['weighted']} weighted, {c['weightless']} weightless, {c['skipped']} skipped, {c['bad_index']} bad index, exponent {c['exponent']}, T = "
                    f"{r['total']}, workspace {r['workspace_mb']} MiB; build {cell(r['build_ms'])} ms.\n\n"
                    "| N | sample, ms | one triangle, ms | search and gather at most |\n|---:|---:|---:|---:|\n")
            for d in r["draws"]:
                share = max(0.0, 1.0 - d["one_triangle_ms"]["median"] / d["sample_ms"]["median"])
                f.write(f"| {d['n']} | {cell(d['sample_ms'])} | {cell(d['one_triangle_ms'])} | {100 * share:.0f} % |\n")
            f.write("\n`simplify(cell)` against the full mesh: `compare` (10^5 area samples per side, max_distance = two cells; accuracy = simplified -> full, "
                    "completeness = full -> simplified) beside `distance_to` (the vertices of the first against the surface of the second); metres:\n\n"
                    "| cell (lattice steps) | triangles | direction | sampled | mean | rms | median | max | far |\n|---:|---:|---|---|---:|---:|---:|---:|---:|\n")
            for s in r["simplify"]:
                for name, key, how in (("simplified -> full", "accuracy", "area"), ("simplified -> full", "vertex_simplified_to_full", "vertices"),
                                       ("full -> simplified", "completeness", "area"), ("full -> simplified", "vertex_full_to_simplified", "vertices")):
                    d = s[key]
                    f.write(f"| {s['cell']:.5f} ({s['lattice_steps']}) | {s['triangles']} | {name} | {how} | {d['mean']} | {d['rms']} | {d['median']} | {d['max']} | "
                            f"{d['far']} |\n")
            f.write("\n| cell (lattice steps) | area | Chamfer | F-score at one lattice step | F-score at two cells | compare, ms |\n|---:|---:|---:|---:|---:|---:|\n")
            for s in r["simplify"]:
                f.write(f"| {s['cell']:.5f} ({s['lattice_steps']}) | {s['area']:.6f} | {s['chamfer']} | {s['fscore'][0]} | {s['fscore'][1]} | {cell(s['compare_ms'])} |\n")
            f.write("\n")
        if a.check:
            f.write("Checked (`--check`): the build's counts and T and a draw of 10^5 samples equal the numpy restatement byte for byte.\n")
        if notes:
            f.write("\n" + notes)


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
        rows.append(measure(f"C3 bench stream, cache after {a.frames} frames", mesh, t, soup[3], soup[4] / soup[5], a))
    if a.only in (None, "sheet"):
        soup = bench_weld.sheet(1000000)
        mesh, t = welded(soup, a.warmup, a.reps)
        rows.append(measure("lattice sheet, 10^6 triangles", mesh, t, soup[3], soup[4] / soup[5], a))
    for r in rows:
        print(json.dumps(r))
    if a.md:
        write_md(a.md, rows, a)


if __name__ == "__main__":
    main()
