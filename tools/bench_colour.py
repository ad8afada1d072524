"""Times `dif_mesh_colour_view` (one RGB keyframe splatted onto the vertices of an indexed mesh) beside `dif_mesh_render` of the same view, and
`dif_mesh_colour_resolve`, with HIP events: the mesh and the poses of tools/bench_raster.py — the welded mesh of the C3 bench stream after
`--frames` frames at 640x480 from the stream's own poses.  Per view, in ONE loop that alternates them (so that a drift of the machine hits
all alike): the render, then the colour view without and with the depth frame of that pose and without and with the edge gate, and once with a grazing gate nothing passes.  The image
is random: what a pixel holds does not change the work.  Per launch: the kernels of one call as the torch profiler sees them.
Usage: python tools/bench_colour.py [--warmup 5] [--reps 50] [--frames 20] [--md profiles/mesh_colour.md]"""
import argparse
import ctypes
import json
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from di_fusion_amd import _lib                                  # noqa: E402
from di_fusion_amd.network import utility as net_util            # noqa: E402
from di_fusion_amd.system import mesh as M                       # noqa: E402
from tools import bench_raster as BR                             # noqa: E402

DEV = torch.device("cuda:0")
# (label, with the depth frame, edge gate, min_cos); the last form gates (nearly) every pixel as grazing: the splat's gathers and arithmetic without its atomics
VARIANTS = (("colour, no depth, no edge gate", False, False, 0.3), ("colour, depth, no edge gate", True, False, 0.3), ("colour, no depth, edge gate", False, True, 0.3),
            ("colour, depth, edge gate", True, True, 0.3), ("colour, min_cos 1: all grazing", False, False, 1.0))
FULL = VARIANTS[3][0]
KERNELS = ("memset", "k_raster_project", "k_raster_triangles", "k_raster_large", "k_raster_resolve", "k_colour_splat")


def timed_alternating(calls: dict, warmup, reps):
    """{name: call} -> {name: dict(median, min, max) in ms}: every repetition runs each call once, each between its own pair of events"""
    for _ in range(warmup):
        for call in calls.values():
            call()
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(reps):
        for k, call in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            torch.cuda.synchronize()
            ms[k].append(a.elapsed_time(b))
    return {k: dict(median=round(statistics.median(x), 4), min=round(min(x), 4), max=round(max(x), 4)) for k, x in ms.items()}


class Colourer:
    """the entry point with every buffer allocated once"""

    def __init__(self, mesh: M.IndexedMesh, H, W):
        self.lib = _lib.load()
        self.mesh = mesh
        self.V, self.K = int(mesh.vertices.shape[0]), int(mesh.triangles.shape[0])
        self.ws_bytes = int(self.lib.dif_mesh_colour_workspace_bytes(self.V, self.K, H, W))
        self.ws = torch.empty((self.ws_bytes,), dtype=torch.uint8, device=DEV)
        self.accum = M.colour_accumulator(self.V, DEV)
        self.counts = torch.empty((_lib.COLOUR_COUNT,), dtype=torch.int32, device=DEV)
        self.rgb8 = torch.empty((self.V, 3), dtype=torch.uint8, device=DEV)
        self.weight = torch.empty((self.V,), dtype=torch.float32, device=DEV)
        self.coloured = torch.empty((1,), dtype=torch.int32, device=DEV)

    def view(self, args, gates, rgb, depth):
        m, P = self.mesh, _lib.ptr
        _lib.check(self.lib.dif_mesh_colour_view(P(m.vertices), P(m.normals), P(m.triangles), self.V, self.K, ctypes.byref(args), ctypes.byref(gates), P(rgb),
                                                 P(depth), P(self.ws), self.ws_bytes, P(self.accum), P(self.counts), _lib.stream_ptr()), "dif_mesh_colour_view")

    def resolve(self):
        P = _lib.ptr
        _lib.check(self.lib.dif_mesh_colour_resolve(P(self.accum), self.V, 0, P(self.rgb8), P(self.weight), P(self.coloured), _lib.stream_ptr()),
                   "dif_mesh_colour_resolve")


def measure(name, mesh, pose, intr, depth, warmup, reps):
    H, W = intr.height, intr.width
    r, c = BR.Renderer(mesh, H, W), Colourer(mesh, H, W)
    args = M.raster_args(pose, intr, H, W)
    rgb = torch.rand((H, W, 3), dtype=torch.float32, device=DEV, generator=torch.Generator(device=DEV).manual_seed(0))
    calls = {"render": lambda: r.call(args)}
    for label, with_depth, edge, min_cos in VARIANTS:
        calls[label] = (lambda g=M.colour_args(min_cos=min_cos, edge_gate=edge), d=depth if with_depth else None: c.view(args, g, rgb, d))
    calls["resolve"] = c.resolve
    t = timed_alternating(calls, warmup, reps)
    # the counts of each variant, from one view onto a zeroed accumulator; the atomics follow from them
    counts = {}
    for label, with_depth, edge, min_cos in VARIANTS:
        c.accum = M.colour_accumulator(c.V, DEV)
        c.view(args, M.colour_args(min_cos=min_cos, edge_gate=edge), rgb, depth if with_depth else None)
        k = dict(zip(M.COLOUR_COUNT_NAMES, c.counts.cpu().tolist()))
        assert k["status"] == 0 and sum(k[n] for n in M.COLOUR_COUNT_NAMES[:6]) == H * W, k
        touched = int((c.accum.cpu().numpy()[:, 3] > 0).sum())
        counts[label] = dict(k, vertices_touched=touched, atomics_at_most=12 * k["used"], atomics_per_touched_vertex=round(12 * k["used"] / max(touched, 1), 2))
    launches = BR.per_launch(lambda: (r.call(args), calls[FULL]()), reps, kernels=r"k_raster_\w+|k_colour_\w+")
    return dict(name=name, vertices=c.V, triangles=c.K, image=f"{W}x{H}", warmup=warmup, reps=reps, ms=t, counts=counts, workspace_bytes=c.ws_bytes,
                per_launch_us_render_plus_colour=launches)


def write_md(path, rows, a):
    with open(path, "w") as f:
        f.write("# `dif_mesh_colour_view`: one RGB keyframe splatted onto the vertices of an indexed mesh\n\n"
                f"`python tools/bench_colour.py --warmup {a.warmup} --reps {a.reps} --frames {a.frames} --md {path}` on one MI355X.\n\n"
                f"Per view: {a.warmup} warm-up rounds, then {a.reps} rounds; a round runs `dif_mesh_render`, the five forms of `dif_mesh_colour_view` and "
                "`dif_mesh_colour_resolve` once each, every call between its own pair of HIP events (the whole chain of a call: memsets, project + z-buffer "
                "reset, triangles, large triangles, then resolve or splat); median (min - max) in milliseconds.  `depth` = the stream's input depth frame "
                "of the same pose, gate 2 cm; the grazing gate is at its default (cos 0.3) but in the last form, where min_cos = 1 gates nearly every pixel: "
                "the splat with its gathers and arithmetic and next to none of its atomics.  The accumulator keeps growing over the rounds "
                "(the sums do not change the work).\n\n"
                "| view | vertices | triangles | render | " + " | ".join(v[0] for v in VARIANTS) + " | resolve |\n|---|---:|---:|" + "---:|" * (len(VARIANTS) + 2) + "\n")
        cell = lambda t: f"{t['median']} ({t['min']} - {t['max']})"              # noqa: E731
        for r in rows:
            f.write(f"| {r['name']} | {r['vertices']} | {r['triangles']} | {cell(r['ms']['render'])} | " + " | ".join(cell(r["ms"][v[0]]) for v in VARIANTS) +
                    f" | {cell(r['ms']['resolve'])} |\n")
        f.write("\nWhere the pixels went (one view onto a zeroed accumulator) and what that costs in atomics: a used pixel sends at most twelve 64-bit "
                "`atomicAdd` (three vertices x four sums; a weight that rounds to zero sends none).\n\n"
                "| view | form | used | no hit | bad colour | depth | edge | grazing | vertices touched | atomics (at most) | per touched vertex |\n"
                "|---|---|---:|---:|---:|---:|---:|---:|---:|---:|---:|\n")
        for r in rows:
            for label, k in r["counts"].items():
                f.write(f"| {r['name']} | {label} | {k['used']} | {k['no_hit']} | {k['bad_colour']} | {k['depth']} | {k['edge']} | {k['grazing']} | {k['vertices_touched']} | "
                        f"{k['atomics_at_most']} | {k['atomics_per_touched_vertex']} |\n")
        f.write(f"\nPer launch (microseconds), one `dif_mesh_render` followed by one `{FULL}` (so the three visibility kernels and the memsets "
                "count twice):\n\n| view | " + " | ".join(KERNELS) + " |\n|---|" + "---:|" * len(KERNELS) + "\n")
        for r in rows:
            p = r["per_launch_us_render_plus_colour"] or {}
            f.write(f"| {r['name']} | " + " | ".join(str(p.get(k, "-")) for k in KERNELS) + " |\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--md", default=None, help="also write the tables as markdown")
    a = ap.parse_args()
    st, intr, _, mesh = BR.c3_scene(net_util.networks_from_arrays(net_util.load_weights_npz()), a.frames)
    rows = []
    for i in sorted({0, a.frames // 2, a.frames - 1}):
        rows.append(measure(f"C3 bench stream after {a.frames} frames, pose of frame {i}", mesh, BR.c3_pose(i), intr, st.depth[i].reshape(intr.height, intr.width),
                            a.warmup, a.reps))
    for r in rows:
        print(json.dumps(r))
    if a.md:
        write_md(a.md, rows, a)


if __name__ == "__main__":
    main()
