"""Indexed mesh: the triangle soup of the mesh cache welded by lattice edge, with area-weighted vertex normals (`dif_mesh_weld`), and a PLY
writer.  No reference counterpart: the reference hands its soup to Open3D (`merge_close_vertices`, `compute_vertex_normals`, commented out in
its main loop as too slow).  The key rule and why the weld is not by position: DESIGN.md "Indexed mesh".  On top of the weld: connected
components, an edge census and the selection of a sub-mesh (`dif_mesh_components`, `dif_mesh_edge_census`, `dif_mesh_select`; DESIGN.md
"Components of an indexed mesh").  And a look at it: depth, normal, std and triangle-index images from a camera pose (`dif_mesh_render`;
DESIGN.md "Rendering an indexed mesh").  And its colour: RGB keyframes splatted onto the vertices through that rasteriser (`dif_mesh_colour_view`,
`dif_mesh_colour_resolve`; DESIGN.md "Colouring an indexed mesh").  And a smaller one: vertex clustering on a grid (`dif_mesh_simplify`; DESIGN.md
"Simplifying an indexed mesh").  And its distance to anything: the exact closest point on its surface for a cloud of points
(`dif_mesh_locator_build`, `dif_mesh_closest`; DESIGN.md "Closest point on an indexed mesh").  And points ON it: samples drawn uniformly by
area, a pure function of (mesh, N, seed) (`dif_mesh_sampler_build`, `dif_mesh_sample`; DESIGN.md "Sampling an indexed mesh"), and on those the
two-sided comparison of two surfaces — accuracy, completeness, Chamfer distance, precision / recall / F-score (`IndexedMesh.compare`) — with
`read_ply` to load the other one.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import numpy as np
import torch

from .. import _lib

COUNT_NAMES = ("vertices", "triangles", "dropped", "unkeyed", "status")


class IndexedMesh:
    """vertices (V,3) f32, normals (V,3) f32 (unit, or zero for a vertex without a triangle), vertex_std (V,) f32, triangles (K,3) i32,
    triangle_flatten_id (K,) i64 — torch tensors on the device that welded them (`.cpu()` for a host copy) — and `counts`: vertices, triangles
    kept, triangles dropped (a repeated index after welding), unkeyed soup corners (not on the lattice: each a vertex of its own), status.
    A mesh derived from another carries its own vertices, triangles and status (`select`) and `components_removed` on top
    (`remove_small_components`).  A coloured one (`colourer().resolve()`) carries `colors` (V,3) uint8 and `color_weight` (V,) f32 as well, and
    `counts["coloured"]`; both are None otherwise.  A simplified one (`simplify`) carries `vertex_cluster` (V of the source,) i32 — the output
    vertex of every source vertex, or -1 — and in `counts` the classes of `SIMPLIFY_COUNT_NAMES`, `cell` and `origin`; it is None otherwise."""

    def __init__(self, vertices, normals, vertex_std, triangles, triangle_flatten_id, counts: dict, colors=None, color_weight=None):
        self.vertices = vertices
        self.normals = normals
        self.vertex_std = vertex_std
        self.triangles = triangles
        self.triangle_flatten_id = triangle_flatten_id
        self.counts = dict(counts)
        self.colors = colors
        self.color_weight = color_weight
        self.vertex_cluster = None

    def cpu(self) -> "IndexedMesh":
        m = IndexedMesh(self.vertices.cpu(), self.normals.cpu(), self.vertex_std.cpu(), self.triangles.cpu(), self.triangle_flatten_id.cpu(),
                        self.counts, None if self.colors is None else self.colors.cpu(),
                        None if self.color_weight is None else self.color_weight.cpu())
        m.vertex_cluster = None if self.vertex_cluster is None else self.vertex_cluster.cpu()
        return m

    def components(self) -> "MeshComponents":
        """Connected components (`components`): per vertex, per triangle, and the size of each."""
        return components(self.triangles, int(self.vertices.shape[0]))

    def topology(self) -> "MeshTopology":
        """`components()` plus, per component, its edges, its boundary edges (used by one triangle: 0 = closed) and V - E + F (2 = a sphere),
        and the most triangles on any one edge (above 2 = not a manifold)."""
        c = self.components()
        n_edges, n_boundary, max_edge_use, status = edge_census(self.triangles, c.vertex_component, c.count)
        return MeshTopology(c.vertex_component, c.triangle_component, c.n_vertices, c.n_triangles, c.count, c.status | status, n_edges, n_boundary,
                            c.n_vertices - n_edges + c.n_triangles, max_edge_use)

    def select(self, triangle_mask: torch.Tensor) -> "IndexedMesh":
        """The sub-mesh of the triangles where `triangle_mask` (K,) is set: the vertices they use, renumbered in ascending order, the triangles in
        their order.  Attributes are copied bit for bit; NORMALS ARE NOT RECOMPUTED — exact when whole components go (`remove_small_components`);
        a vertex on the cut of any other mask keeps the normal summed over its former triangles.  COLOURS ARE DROPPED (the result has
        `colors = None`): cull first, colour after."""
        return _select(self, triangle_mask, None)

    def remove_small_components(self, min_triangles: int = 0, keep_largest: Optional[int] = None) -> "IndexedMesh":
        """Without the components of fewer than `min_triangles` triangles; `keep_largest=k`: of the rest, only the k with the most triangles (ties
        go to the lower component id).  Vertices that no kept triangle uses go too.  The mask is built on the device; the only synchronisations
        are the two read-backs of counts.  `counts["components_removed"]` of the result says how many went.  Colours are dropped, as by
        `select`: cull first, colour after."""
        c = self.components()
        keep = c.n_triangles >= int(min_triangles)
        if keep_largest is not None:
            order = torch.sort(torch.where(keep, c.n_triangles, torch.full_like(c.n_triangles, -1)), descending=True, stable=True).indices
            largest = torch.zeros_like(keep)
            largest[order[:max(int(keep_largest), 0)]] = True
            keep = keep & largest
        tc = c.triangle_component.long()
        mask = (tc >= 0) & keep[tc.clamp(min=0)] if c.count > 0 else torch.zeros_like(tc, dtype=torch.bool)
        return _select(self, mask, c.count - (keep & (c.n_triangles > 0)).sum().to(torch.int32))

    def simplify(self, cell: float, origin: Sequence[float] = (0.0, 0.0, 0.0)) -> "IndexedMesh":
        """A smaller mesh by vertex clustering (`simplify`): the vertices inside one cube of edge `cell` (world units) of the grid through `origin`
        become their mean, triangles that collapse or repeat go, normals are recomputed.  Colours travel along when the mesh has them: the
        weighted mean of a cluster, resolved with `colour_resolve(min_weight=0)`.  The result carries `vertex_cluster` and, in `counts`, the
        classes, `cell` and `origin` (as the float32 the kernel saw).  Vertex clustering preserves neither manifoldness nor genus, places no
        vertex by a quadric, and fuses thin double-sided sheets closer than a cell."""
        return simplify(self.vertices, self.vertex_std, self.triangles, self.triangle_flatten_id, cell, origin, self.colors, self.color_weight)

    def locator(self, cell: Optional[float] = None) -> "MeshLocator":
        """A `MeshLocator` over this mesh's surface (`locator`): build once, query with `.closest` as often as needed."""
        return locator(self.vertices, self.triangles, cell)

    def closest(self, points: torch.Tensor, max_distance: float, cell: Optional[float] = None) -> "MeshClosest":
        """The closest point of this mesh's surface for every row of `points` (N,>=3) f32 within `max_distance` (`MeshLocator.closest`).  Builds a
        locator for the one call: keep `self.locator()` when there are several clouds."""
        return self.locator(cell).closest(points, max_distance)

    def distance_to(self, other: "IndexedMesh", max_distance: float, cell: Optional[float] = None) -> dict:
        """This mesh's VERTICES against `other`'s SURFACE: `d2` (V,) f32 on the device (inf where nothing of `other` lies within `max_distance`),
        and `mean`, `rms`, `max`, `median` of the distance over the vertices that found a point, `found` and `far` (NaN figures when none did).
        ONE-SIDED and VERTEX-SAMPLED: it does not see where `other` has surface that this mesh lacks, nor what happens inside this mesh's
        triangles — call it both ways for a symmetric figure.  Unsigned.  The reductions run on the device; one read-back on top of the locator's.
        `cell`: the cell of `other`'s locator; default: `default_locator_cell`, or max_distance / 59 where that is larger, so that any
        `max_distance` stays within the ring limit (no answer depends on the cell)."""
        if cell is None:
            r = float(np.float32(max_distance))
            cell = default_locator_cell(other.vertices, other.triangles)
            if np.isfinite(r) and r > 0.0:
                cell = max(cell, float(np.float32(r / (_lib.LOCATOR_MAX_RATIO - 1))))
        c = other.locator(cell).closest(self.vertices, max_distance)
        with torch.cuda.device(self.vertices.device):
            d = torch.sqrt(c.d2[torch.isfinite(c.d2)]).double()
            if d.numel() > 0:
                stats = torch.stack([d.mean(), torch.sqrt((d * d).mean()), d.max(), d.median()]).cpu().tolist()
            else:
                stats = [float("nan")] * 4
        return dict(d2=c.d2, mean=stats[0], rms=stats[1], max=stats[2], median=stats[3], found=c.counts["found"], far=c.counts["far"])

    def interpolate(self, closest: "MeshClosest", values: torch.Tensor) -> torch.Tensor:
        """A per-vertex attribute `values` (V,) or (V,C) f32 of THIS mesh at the closest points of `closest` (a result of this mesh's locator):
        (b0 x0 + b1 x1) + b2 x2 per row with the barycentrics and the triangle's three vertices in index order, in float32 — what carries std,
        normals or colours from one mesh to the points (or the vertices) of another.  Rows without a closest point are NaN.
        A `MeshSamples` of this mesh (`sample`) has the same two fields: `interpolate(samples, self.normals)` is a normal per sample."""
        _lib.require_cuda(values, closest.triangle, closest.barycentric)
        V = int(self.vertices.shape[0])
        if values.dtype != torch.float32 or values.dim() not in (1, 2) or int(values.shape[0]) != V:
            raise RuntimeError(f"interpolate: values must be ({V},) or ({V},C) float32; got {tuple(values.shape)} {values.dtype}")
        return interpolate(self.triangles, closest.triangle, closest.barycentric, values)

    def sampler(self) -> "MeshSampler":
        """A `MeshSampler` over this mesh's surface (`sampler`): build once, draw with `.sample` as often as needed."""
        return sampler(self.vertices, self.triangles)

    def sample(self, n: int, seed: int = 0) -> "MeshSamples":
        """`n` points drawn uniformly by area from this mesh's surface (`MeshSampler.sample`), a pure function of (mesh, n, seed).  The result has
        the two fields `interpolate` reads, so `mesh.interpolate(mesh.sample(n), mesh.normals)` is a normal per sample: any mesh as an xyz +
        normal cloud.  Builds a sampler for the one call: keep `self.sampler()` when there are several draws."""
        return self.sampler().sample(n, seed)

    def compare(self, other: "IndexedMesh", max_distance: float, n_samples: int = 100_000, seed: int = 0,
                thresholds: Sequence[float] = (0.005, 0.01, 0.02), cell: Optional[float] = None) -> dict:
        """The two-sided, AREA-SAMPLED comparison of two surfaces: `n_samples` points on this mesh (seed) against `other`'s surface — `accuracy` —
        and `n_samples` points on `other` (seed + 1) against this one's — `completeness`.  Each direction is a dict of `mean`, `rms`, `median`,
        `max` of the distance over the samples that found a point within `max_distance` (NaN when none did; the median is the lower middle, as
        torch's), the counts `found` and `far`, and `within`: per threshold, how many samples lie at d <= tau (a far sample never does).  On top:
        `chamfer` = the mean of the two means, `thresholds`, and per threshold `precision` = within of accuracy / samples drawn, `recall` = the
        same of completeness, `fscore` = 2 P R / (P + R), or 0 when P + R = 0 (a surface without area draws no samples: 0).  d = sqrt(d2) in
        float64 from the closest operator's float32 d2; the reductions run on the device in float64.  Unsigned.  `cell`: the cell of both
        locators; default: `distance_to`'s rule for each.  Every threshold must be <= `max_distance` (ValueError)."""
        taus = [float(t) for t in thresholds]
        r = float(np.float32(max_distance))
        for t in taus:
            if not t <= r:
                raise ValueError(f"compare: threshold {t} is beyond max_distance {r} (as float32): a sample beyond max_distance finds nothing")
        n = int(n_samples)
        seed = int(seed)
        out = dict(thresholds=tuple(taus))
        for name, a, b, s in (("accuracy", self, other, seed), ("completeness", other, self, seed + 1)):
            pts = a.sample(n, s)
            out[name] = _sampled_distance(pts.point, int(pts.counts["samples"]), b, max_distance, cell, taus)
        out["chamfer"] = 0.5 * (out["accuracy"]["mean"] + out["completeness"]["mean"])
        out["precision"] = [w / n if n else 0.0 for w in out["accuracy"]["within"]]
        out["recall"] = [w / n if n else 0.0 for w in out["completeness"]["within"]]
        out["fscore"] = [2.0 * p * q / (p + q) if p + q > 0 else 0.0 for p, q in zip(out["precision"], out["recall"])]
        return out

    def render(self, pose, intrinsics, height: int, width: int, z_near: float = 0.05, cull_backfaces: bool = False) -> "MeshRender":
        """Depth, normal, std and triangle-index images of this mesh from the camera-to-world `pose` (`render`)."""
        return render(self.vertices, self.normals, self.vertex_std, self.triangles, pose, intrinsics, height, width, z_near, cull_backfaces)

    def colourer(self) -> "MeshColourer":
        """A `MeshColourer` over this mesh: add RGB keyframes with `.add_view`, then `.resolve()` for the coloured mesh."""
        return MeshColourer(self)

    def write_ply(self, path):
        """Binary little-endian PLY: x y z nx ny nz quality (= std) as float32 per vertex — then red green blue as uchar if the mesh carries
        colours; without them the file is what it always was — faces as uchar count + three int indices."""
        v = self.vertices.cpu().numpy()
        floats = ("x", "y", "z", "nx", "ny", "nz", "quality")
        rgb = ("red", "green", "blue") if self.colors is not None else ()
        vert = np.empty((v.shape[0],), dtype=[(n, "<f4") for n in floats] + [(n, "u1") for n in rgb])
        n = self.normals.cpu().numpy()
        for k, name in enumerate(("x", "y", "z")):
            vert[name] = v[:, k]
            vert["n" + name] = n[:, k]
        vert["quality"] = self.vertex_std.cpu().numpy()
        if rgb:
            c = self.colors.cpu().numpy()
            for k, name in enumerate(rgb):
                vert[name] = c[:, k]
        t = self.triangles.cpu().numpy()
        face = np.empty((t.shape[0],), dtype=[("n", "u1"), ("v", "<i4", (3,))])
        face["n"] = 3
        face["v"] = t
        header = ("ply\nformat binary_little_endian 1.0\ncomment di_fusion_amd indexed mesh\n"
                  f"element vertex {vert.shape[0]}\n" + "".join(f"property float {name}\n" for name in floats) + "".join(f"property uchar {name}\n" for name in rgb) +
                  f"element face {face.shape[0]}\nproperty list uchar int vertex_indices\nend_header\n")
        with open(path, "wb") as f:
            f.write(header.encode("ascii"))
            f.write(vert.tobytes())
            f.write(face.tobytes())

    def to_open3d(self):
        """`open3d.geometry.TriangleMesh` with vertex normals, and vertex colours if the mesh carries them (raises ImportError without Open3D)."""
        import open3d as o3d
        m = o3d.geometry.TriangleMesh()
        m.vertices = o3d.utility.Vector3dVector(self.vertices.cpu().numpy().astype(np.float64))
        m.triangles = o3d.utility.Vector3iVector(self.triangles.cpu().numpy())
        m.vertex_normals = o3d.utility.Vector3dVector(self.normals.cpu().numpy().astype(np.float64))
        if self.colors is not None:
            m.vertex_colors = o3d.utility.Vector3dVector(self.colors.cpu().numpy().astype(np.float64) / 255.0)
        return m


def weld_args(bound_min: Sequence[float], voxel_size: float, resolution: int, n_xyz: Optional[Sequence[int]] = None) -> _lib.DifWeldArgs:
    a = _lib.DifWeldArgs()
    for k in range(3):
        a.bound_min[k] = float(bound_min[k])
        a.n_xyz[k] = int(n_xyz[k]) if n_xyz is not None else 0
    a.voxel_size = float(voxel_size)
    a.resolution = int(resolution)
    return a


def weld(vertices: torch.Tensor, std: torch.Tensor, ids: torch.Tensor, bound_min, voxel_size: float, resolution: int,
         n_xyz: Optional[Sequence[int]] = None) -> IndexedMesh:
    """The flat operator: soup (vertices (T,3,3) f32 world units, std (T,3) f32, ids (T,) i64 — the mesh-cache arrays, on the GPU) of a map with
    `bound_min`, `voxel_size`, extracted at `resolution` -> `IndexedMesh`.  Reads the counts back (one synchronisation) to slice the outputs."""
    _lib.require_cuda(vertices, std, ids)
    if vertices.dtype != torch.float32 or std.dtype != torch.float32 or ids.dtype != torch.int64:
        raise RuntimeError("weld: vertices and std must be float32, ids int64")
    T = int(vertices.shape[0])
    if tuple(vertices.shape) != (T, 3, 3) or tuple(std.shape) != (T, 3) or tuple(ids.shape) != (T,):
        raise RuntimeError(f"weld: expected (T,3,3), (T,3), (T,); got {tuple(vertices.shape)}, {tuple(std.shape)}, {tuple(ids.shape)}")
    if isinstance(bound_min, torch.Tensor):
        bound_min = bound_min.detach().cpu().tolist()
    dev = vertices.device
    lib = _lib.load()
    args = weld_args(bound_min, voxel_size, resolution, n_xyz)
    ws_bytes = int(lib.dif_mesh_weld_workspace_bytes(T))
    if ws_bytes < 0:
        raise RuntimeError(f"libdifusion: dif_mesh_weld cannot index {T} triangles (3 T must stay below 2^31)")
    with torch.cuda.device(dev):
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
        out_v = torch.empty((3 * T, 3), dtype=torch.float32, device=dev)
        out_n = torch.empty((3 * T, 3), dtype=torch.float32, device=dev)
        out_s = torch.empty((3 * T,), dtype=torch.float32, device=dev)
        out_t = torch.empty((T, 3), dtype=torch.int32, device=dev)
        out_i = torch.empty((T,), dtype=torch.int64, device=dev)
        counts = torch.empty((_lib.WELD_COUNT,), dtype=torch.int32, device=dev)
        _lib.check(lib.dif_mesh_weld(_lib.ptr(vertices), _lib.ptr(std), _lib.ptr(ids), T, ctypes.byref(args), _lib.ptr(ws), ws_bytes, _lib.ptr(out_v),
                                     _lib.ptr(out_n), _lib.ptr(out_s), _lib.ptr(out_t), _lib.ptr(out_i), _lib.ptr(counts), _lib.stream_ptr()),
                   "dif_mesh_weld")
        c = counts.cpu().tolist()
    if c[_lib.WELD_STATUS] != 0:
        raise RuntimeError(f"libdifusion: dif_mesh_weld reported status {c[_lib.WELD_STATUS]} (its class table overflowed)")
    V, K = c[_lib.WELD_VERTICES], c[_lib.WELD_KEPT]
    return IndexedMesh(out_v[:V], out_n[:V], out_s[:V], out_t[:K], out_i[:K], dict(zip(COUNT_NAMES, c[:len(COUNT_NAMES)])))


# ---- components, selection, edge census (DESIGN.md "Components of an indexed mesh") -----------------------------------------------------
class MeshComponents:
    """vertex_component (V,) i32, triangle_component (K,) i32 (-1: the triangle holds an index outside [0, V)), n_vertices (C,) i32 and
    n_triangles (C,) i32 — device tensors — `count` = C and `status` (0, or `_lib.MESH_STATUS_BAD_INDEX`).  Components are numbered in
    ascending order of their lowest vertex id; a vertex without a triangle is a component of its own."""

    def __init__(self, vertex_component, triangle_component, n_vertices, n_triangles, count: int, status: int = 0):
        self.vertex_component = vertex_component
        self.triangle_component = triangle_component
        self.n_vertices = n_vertices
        self.n_triangles = n_triangles
        self.count = int(count)
        self.status = int(status)


class MeshTopology(MeshComponents):
    """`MeshComponents` plus n_edges (C,), n_boundary (C,) (edges with one triangle), euler (C,) = V - E + F — device i32 — and `max_edge_use`."""

    def __init__(self, vertex_component, triangle_component, n_vertices, n_triangles, count, status, n_edges, n_boundary, euler, max_edge_use: int):
        super().__init__(vertex_component, triangle_component, n_vertices, n_triangles, count, status)
        self.n_edges = n_edges
        self.n_boundary = n_boundary
        self.euler = euler
        self.max_edge_use = int(max_edge_use)


def _check_status(status: int, what: str):
    if status & ~_lib.MESH_STATUS_BAD_INDEX:
        raise RuntimeError(f"libdifusion: {what} reported status {status} (an iteration bound or its edge table was exceeded)")


def _check_triangles(triangles: torch.Tensor, what: str) -> int:
    _lib.require_cuda(triangles)
    if triangles.dtype != torch.int32 or triangles.dim() != 2 or triangles.shape[1] != 3:
        raise RuntimeError(f"{what}: triangles must be (K,3) int32; got {tuple(triangles.shape)} {triangles.dtype}")
    return int(triangles.shape[0])


def components(triangles: torch.Tensor, n_vertices: int) -> MeshComponents:
    """The flat operator: triangles (K,3) i32 on the GPU over vertices 0..n_vertices-1 -> `MeshComponents`.  Reads the counts back (one
    synchronisation) to slice the per-component sizes."""
    K, V = _check_triangles(triangles, "components"), int(n_vertices)
    dev = triangles.device
    lib = _lib.load()
    ws_bytes = int(lib.dif_mesh_components_workspace_bytes(V, K))
    if ws_bytes < 0:
        raise RuntimeError(f"libdifusion: dif_mesh_components cannot index {V} vertices, {K} triangles (V and 3 K must stay below 2^31)")
    with torch.cuda.device(dev):
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
        vc = torch.empty((V,), dtype=torch.int32, device=dev)
        tc = torch.empty((K,), dtype=torch.int32, device=dev)
        nv = torch.empty((V,), dtype=torch.int32, device=dev)
        nt = torch.empty((V,), dtype=torch.int32, device=dev)
        counts = torch.empty((_lib.COMP_COUNT,), dtype=torch.int32, device=dev)
        _lib.check(lib.dif_mesh_components(_lib.ptr(triangles), K, V, _lib.ptr(ws), ws_bytes, _lib.ptr(vc), _lib.ptr(tc), _lib.ptr(nv), _lib.ptr(nt),
                                           _lib.ptr(counts), _lib.stream_ptr()), "dif_mesh_components")
        c = counts.cpu().tolist()
    _check_status(c[_lib.COMP_STATUS], "dif_mesh_components")
    C = c[_lib.COMP_COMPONENTS]
    return MeshComponents(vc, tc, nv[:C], nt[:C], C, c[_lib.COMP_STATUS])


def edge_census(triangles: torch.Tensor, vertex_component: torch.Tensor, n_components: int):
    """The flat operator: triangles (K,3) i32 and the component of every vertex (V,) i32 with values below `n_components`, on the GPU ->
    (n_edges (C,) i32, n_boundary (C,) i32, max_edge_use, status).  An edge is counted with the component of its lower end point; a triangle
    side with equal end points is no edge.  One synchronisation (the counts)."""
    K = _check_triangles(triangles, "edge_census")
    _lib.require_cuda(vertex_component)
    if vertex_component.dtype != torch.int32 or vertex_component.dim() != 1:
        raise RuntimeError("edge_census: vertex_component must be (V,) int32")
    V, C = int(vertex_component.shape[0]), int(n_components)
    dev = triangles.device
    lib = _lib.load()
    ws_bytes = int(lib.dif_mesh_edge_census_workspace_bytes(K))
    if ws_bytes < 0:
        raise RuntimeError(f"libdifusion: dif_mesh_edge_census cannot index {K} triangles (6 K must not pass 2^31)")
    with torch.cuda.device(dev):
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
        ne = torch.empty((C,), dtype=torch.int32, device=dev)
        nb = torch.empty((C,), dtype=torch.int32, device=dev)
        counts = torch.empty((_lib.EDGE_COUNT,), dtype=torch.int32, device=dev)
        _lib.check(lib.dif_mesh_edge_census(_lib.ptr(triangles), K, V, _lib.ptr(vertex_component), C, _lib.ptr(ws), ws_bytes, _lib.ptr(ne), _lib.ptr(nb),
                                            _lib.ptr(counts), _lib.stream_ptr()), "dif_mesh_edge_census")
        c = counts.cpu().tolist()
    _check_status(c[_lib.EDGE_STATUS], "dif_mesh_edge_census")
    return ne, nb, c[_lib.EDGE_MAX_USE], c[_lib.EDGE_STATUS]


def select(vertices: torch.Tensor, normals: torch.Tensor, vertex_std: torch.Tensor, triangles: torch.Tensor, triangle_flatten_id: torch.Tensor,
           keep: torch.Tensor) -> IndexedMesh:
    """The flat operator behind `IndexedMesh.select`: the arrays of an indexed mesh on the GPU and `keep` (K,) bool or uint8 -> `IndexedMesh`.
    `counts`: vertices, triangles, status (`_lib.MESH_STATUS_BAD_INDEX`: a kept triangle held an index outside [0, V) and was dropped)."""
    return _select(IndexedMesh(vertices, normals, vertex_std, triangles, triangle_flatten_id, {}), keep, None)


def _select(m: IndexedMesh, keep: torch.Tensor, components_removed: Optional[torch.Tensor]) -> IndexedMesh:
    """`components_removed`: a device int32 scalar that travels back with the counts (no synchronisation of its own)."""
    K = _check_triangles(m.triangles, "select")
    _lib.require_cuda(m.vertices, m.normals, m.vertex_std, m.triangle_flatten_id, keep)
    V = int(m.vertices.shape[0])
    if m.vertices.dtype != torch.float32 or m.normals.dtype != torch.float32 or m.vertex_std.dtype != torch.float32 or \
            m.triangle_flatten_id.dtype != torch.int64:
        raise RuntimeError("select: vertices, normals and vertex_std must be float32, triangle_flatten_id int64")
    if tuple(m.vertices.shape) != (V, 3) or tuple(m.normals.shape) != (V, 3) or tuple(m.vertex_std.shape) != (V,) or \
            tuple(m.triangle_flatten_id.shape) != (K,) or tuple(keep.shape) != (K,):
        raise RuntimeError(f"select: expected (V,3), (V,3), (V,), (K,3), (K,), (K,); got {tuple(m.vertices.shape)}, {tuple(m.normals.shape)}, "
                           f"{tuple(m.vertex_std.shape)}, {tuple(m.triangles.shape)}, {tuple(m.triangle_flatten_id.shape)}, {tuple(keep.shape)}")
    if keep.dtype not in (torch.bool, torch.uint8):
        raise RuntimeError(f"select: the mask must be bool or uint8; got {keep.dtype}")
    dev = m.triangles.device
    lib = _lib.load()
    ws_bytes = int(lib.dif_mesh_select_workspace_bytes(V, K))
    if ws_bytes < 0:
        raise RuntimeError(f"libdifusion: dif_mesh_select cannot index {V} vertices, {K} triangles (V and 3 K must stay below 2^31)")
    with torch.cuda.device(dev):
        keep8 = keep.view(torch.uint8) if keep.dtype == torch.bool else keep
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
        out_v = torch.empty((V, 3), dtype=torch.float32, device=dev)
        out_n = torch.empty((V, 3), dtype=torch.float32, device=dev)
        out_s = torch.empty((V,), dtype=torch.float32, device=dev)
        out_t = torch.empty((K, 3), dtype=torch.int32, device=dev)
        out_i = torch.empty((K,), dtype=torch.int64, device=dev)
        counts = torch.empty((_lib.SELECT_COUNT + 1,), dtype=torch.int32, device=dev)
        _lib.check(lib.dif_mesh_select(_lib.ptr(m.vertices), _lib.ptr(m.normals), _lib.ptr(m.vertex_std), _lib.ptr(m.triangles),
                                       _lib.ptr(m.triangle_flatten_id), V, K, _lib.ptr(keep8), _lib.ptr(ws), ws_bytes, _lib.ptr(out_v), _lib.ptr(out_n),
                                       _lib.ptr(out_s), _lib.ptr(out_t), _lib.ptr(out_i), _lib.ptr(counts), _lib.stream_ptr()), "dif_mesh_select")
        counts[_lib.SELECT_COUNT:] = components_removed if components_removed is not None else 0
        c = counts.cpu().tolist()
    _check_status(c[_lib.SELECT_STATUS], "dif_mesh_select")
    nv, nk = c[_lib.SELECT_VERTICES], c[_lib.SELECT_TRIANGLES]
    out = dict(vertices=nv, triangles=nk, status=c[_lib.SELECT_STATUS])
    if components_removed is not None:
        out["components_removed"] = c[_lib.SELECT_COUNT]
    return IndexedMesh(out_v[:nv], out_n[:nv], out_s[:nv], out_t[:nk], out_i[:nk], out)


# ---- simplification (DESIGN.md "Simplifying an indexed mesh") --------------------------------------------------------------------------
SIMPLIFY_COUNT_NAMES = ("vertices", "triangles", "unkeyed", "collapsed", "duplicate", "isolated", "bad_std", "flat", "status")


def simplify_args(cell: float, origin: Sequence[float] = (0.0, 0.0, 0.0)) -> _lib.DifSimplifyArgs:
    a = _lib.DifSimplifyArgs()
    if isinstance(origin, torch.Tensor):
        origin = origin.detach().cpu().tolist()
    if len(origin) != 3:
        raise ValueError(f"simplify: origin must have three components; got {len(origin)}")
    for k in range(3):
        a.origin[k] = float(origin[k])
    a.cell = float(cell)
    if not (a.cell > 0.0 and np.isfinite(a.cell)) or not all(np.isfinite(a.origin[k]) for k in range(3)):
        raise ValueError(f"simplify: cell must be positive and finite, origin finite (as float32); got {cell}, {tuple(origin)}")
    return a


def simplify(vertices: torch.Tensor, vertex_std: torch.Tensor, triangles: torch.Tensor, triangle_flatten_id: torch.Tensor, cell: float,
             origin: Sequence[float] = (0.0, 0.0, 0.0), colors: Optional[torch.Tensor] = None, color_weight: Optional[torch.Tensor] = None) -> IndexedMesh:
    """The flat operator: the arrays of an indexed mesh on the GPU -> the `IndexedMesh` of its vertex clusters on the grid of cubes of edge
    `cell` through `origin` (`dif_mesh_simplify`, include/difusion.h has the contract).  `colors` (V,3) uint8 and `color_weight` (V,) f32, both
    or neither: the result then carries the weighted cluster means as `colors` / `color_weight` and `counts["coloured"]`.  `counts`: the names of
    `SIMPLIFY_COUNT_NAMES` (status may hold `_lib.MESH_STATUS_BAD_INDEX`: such triangles are dropped), `cell` and `origin` as the float32 values
    the kernel saw; `vertex_cluster` (V,) i32 on the result.  One synchronisation (the counts), a second one with colours."""
    K = _check_triangles(triangles, "simplify")
    _lib.require_cuda(vertices, vertex_std, triangle_flatten_id, colors, color_weight)
    V = int(vertices.shape[0])
    if vertices.dtype != torch.float32 or vertex_std.dtype != torch.float32 or triangle_flatten_id.dtype != torch.int64:
        raise RuntimeError("simplify: vertices and vertex_std must be float32, triangle_flatten_id int64")
    if tuple(vertices.shape) != (V, 3) or tuple(vertex_std.shape) != (V,) or tuple(triangle_flatten_id.shape) != (K,):
        raise RuntimeError(f"simplify: expected (V,3), (V,), (K,3), (K,); got {tuple(vertices.shape)}, {tuple(vertex_std.shape)}, "
                           f"{tuple(triangles.shape)}, {tuple(triangle_flatten_id.shape)}")
    if (colors is None) != (color_weight is None):
        raise ValueError("simplify: colors and color_weight go together: both or neither")
    if colors is not None and (colors.dtype != torch.uint8 or tuple(colors.shape) != (V, 3) or color_weight.dtype != torch.float32 or
                               tuple(color_weight.shape) != (V,)):
        raise RuntimeError(f"simplify: colors must be ({V},3) uint8 and color_weight ({V},) float32; got {tuple(colors.shape)} {colors.dtype}, "
                           f"{tuple(color_weight.shape)} {color_weight.dtype}")
    args = simplify_args(cell, origin)
    dev = triangles.device
    lib = _lib.load()
    ws_bytes = int(lib.dif_mesh_simplify_workspace_bytes(V, K))
    if ws_bytes < 0:
        raise RuntimeError(f"libdifusion: dif_mesh_simplify cannot index {V} vertices, {K} triangles (V and 3 K must stay below 2^31)")
    with torch.cuda.device(dev):
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
        out_v = torch.empty((V, 3), dtype=torch.float32, device=dev)
        out_n = torch.empty((V, 3), dtype=torch.float32, device=dev)
        out_s = torch.empty((V,), dtype=torch.float32, device=dev)
        out_t = torch.empty((K, 3), dtype=torch.int32, device=dev)
        out_i = torch.empty((K,), dtype=torch.int64, device=dev)
        accum = colour_accumulator(V, dev) if colors is not None else None
        cluster = torch.empty((V,), dtype=torch.int32, device=dev)
        counts = torch.empty((_lib.SIMPLIFY_COUNT,), dtype=torch.int32, device=dev)
        _lib.check(lib.dif_mesh_simplify(_lib.ptr(vertices), _lib.ptr(vertex_std), _lib.ptr(triangles), _lib.ptr(triangle_flatten_id), V, K, _lib.ptr(colors),
                                         _lib.ptr(color_weight), ctypes.byref(args), _lib.ptr(ws), ws_bytes, _lib.ptr(out_v), _lib.ptr(out_n), _lib.ptr(out_s),
                                         _lib.ptr(out_t), _lib.ptr(out_i), _lib.ptr(accum), _lib.ptr(cluster), _lib.ptr(counts), _lib.stream_ptr()),
                   "dif_mesh_simplify")
        c = counts.cpu().tolist()
        _check_status(c[_lib.SIMPLIFY_STATUS], "dif_mesh_simplify")
        nv, nk = c[_lib.SIMPLIFY_VERTICES], c[_lib.SIMPLIFY_TRIANGLES]
        out = dict(zip(SIMPLIFY_COUNT_NAMES, c[:len(SIMPLIFY_COUNT_NAMES)]), cell=float(args.cell), origin=tuple(float(args.origin[k]) for k in range(3)))
        col = weight = None
        if accum is not None:
            col, weight, out["coloured"] = colour_resolve(accum[:nv], 0.0)
    m = IndexedMesh(out_v[:nv], out_n[:nv], out_s[:nv], out_t[:nk], out_i[:nk], out, col, weight)
    m.vertex_cluster = cluster
    return m


# ---- rendering (DESIGN.md "Rendering an indexed mesh") ---------------------------------------------------------------------------------
RENDER_COUNT_NAMES = ("pixels_hit", "drawn", "clipped", "degenerate", "culled", "offscreen", "large", "status")


class MeshRender:
    """depth (H,W) f32 (camera z; NaN where nothing was hit — the project's invalid depth: `ext.unproject_depth` turns it into NaN points),
    normal (H,W,3) f32 (unit, in the mesh's frame, NOT turned towards the camera; zero where nothing was hit), std (H,W) f32 (NaN where nothing
    was hit), triangle (H,W) i32 (index into the mesh's triangles, -1 where nothing was hit) — device tensors, `.cpu()` for a host copy — and
    `counts`: pixels hit, triangles drawn, clipped (a vertex at or behind `z_near`, non-finite, or far outside the image: THE WHOLE TRIANGLE
    GOES, there is no near-plane clipping), degenerate, culled, offscreen, large (the drawn ones a workgroup walked), status."""

    def __init__(self, depth, normal, std, triangle, counts: dict):
        self.depth = depth
        self.normal = normal
        self.std = std
        self.triangle = triangle
        self.counts = dict(counts)

    def cpu(self) -> "MeshRender":
        return MeshRender(self.depth.cpu(), self.normal.cpu(), self.std.cpu(), self.triangle.cpu(), self.counts)


def world_to_cam_rows(pose) -> np.ndarray:
    """camera-to-world pose (a `tracker.Pose`, a 4x4 array or tensor, anything `Pose.of` accepts) -> the 12 float32 of the row-major 3x4
    world-to-camera transform: R^T and -R^T t in float64, rounded once (like `tracker._rows34`)."""
    from .tracker import Pose
    if isinstance(pose, torch.Tensor):
        pose = pose.detach().cpu().numpy()
    if isinstance(pose, np.ndarray):
        if pose.shape != (4, 4):
            raise RuntimeError(f"render: a pose matrix must be 4x4; got {pose.shape}")
        pose = pose.astype(np.float64)
    p = Pose.of(pose)
    return np.concatenate([p.R.T, -(p.R.T @ p.t)[:, None]], axis=1).astype(np.float32).reshape(12)


def raster_args(pose, intrinsics, height: int, width: int, z_near: float = 0.05, cull_backfaces: bool = False) -> _lib.DifRasterArgs:
    a = _lib.DifRasterArgs()
    for k, x in enumerate(world_to_cam_rows(pose)):
        a.world_to_cam[k] = float(x)
    if all(hasattr(intrinsics, n) for n in ("fx", "fy", "cx", "cy")):
        intrinsics = (intrinsics.fx, intrinsics.fy, intrinsics.cx, intrinsics.cy)
    a.fx, a.fy, a.cx, a.cy = (float(x) for x in intrinsics)
    a.z_near = float(z_near)
    a.height, a.width, a.cull_backfaces = int(height), int(width), int(bool(cull_backfaces))
    return a


def render(vertices: torch.Tensor, normals: torch.Tensor, vertex_std: torch.Tensor, triangles: torch.Tensor, pose, intrinsics, height: int,
           width: int, z_near: float = 0.05, cull_backfaces: bool = False) -> MeshRender:
    """The flat operator: the arrays of an indexed mesh on the GPU, the camera-to-world `pose`, `intrinsics` = (fx, fy, cx, cy) or an object
    with those attributes -> `MeshRender` of `height` x `width` pixels.  Pixel (u, v) is column and row with its centre at integer
    coordinates, x = (u - cx) / fx * z (the convention of `ext.unproject_depth`).  One synchronisation (the counts)."""
    K = _check_triangles(triangles, "render")
    _lib.require_cuda(vertices, normals, vertex_std)
    V = int(vertices.shape[0])
    if vertices.dtype != torch.float32 or normals.dtype != torch.float32 or vertex_std.dtype != torch.float32:
        raise RuntimeError("render: vertices, normals and vertex_std must be float32")
    if tuple(vertices.shape) != (V, 3) or tuple(normals.shape) != (V, 3) or tuple(vertex_std.shape) != (V,):
        raise RuntimeError(f"render: expected (V,3), (V,3), (V,); got {tuple(vertices.shape)}, {tuple(normals.shape)}, {tuple(vertex_std.shape)}")
    args = raster_args(pose, intrinsics, height, width, z_near, cull_backfaces)
    H, W = int(args.height), int(args.width)
    dev = triangles.device
    lib = _lib.load()
    ws_bytes = int(lib.dif_mesh_render_workspace_bytes(V, K, H, W))
    if ws_bytes < 0:
        raise RuntimeError(f"libdifusion: dif_mesh_render failed: {_lib.ERRORS[-1]}: cannot index {V} vertices, {K} triangles, {H} x {W} pixels "
                           "(the image must not be empty; V, 3 K and H W must stay below 2^31)")
    with torch.cuda.device(dev):
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
        depth = torch.empty((H, W), dtype=torch.float32, device=dev)
        normal = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
        std = torch.empty((H, W), dtype=torch.float32, device=dev)
        triangle = torch.empty((H, W), dtype=torch.int32, device=dev)
        counts = torch.empty((_lib.RASTER_COUNT,), dtype=torch.int32, device=dev)
        _lib.check(lib.dif_mesh_render(_lib.ptr(vertices), _lib.ptr(normals), _lib.ptr(vertex_std), _lib.ptr(triangles), V, K, ctypes.byref(args),
                                       _lib.ptr(ws), ws_bytes, _lib.ptr(depth), _lib.ptr(normal), _lib.ptr(std), _lib.ptr(triangle), _lib.ptr(counts),
                                       _lib.stream_ptr()), "dif_mesh_render")
        c = counts.cpu().tolist()
    _check_status(c[_lib.RASTER_STATUS], "dif_mesh_render")
    return MeshRender(depth, normal, std, triangle, dict(zip(RENDER_COUNT_NAMES, c)))


# ---- colouring (DESIGN.md "Colouring an indexed mesh") ---------------------------------------------------------------------------------
COLOUR_COUNT_NAMES = ("used", "no_hit", "bad_colour", "depth", "edge", "grazing", "status")


def colour_args(depth_tol: float = 0.02, min_cos: float = 0.3, edge_gate: bool = True) -> _lib.DifColourArgs:
    """The gates of `colour_view`: `depth_tol` (metres; the depth gate against the view's depth frame, and the step that makes a pixel a
    silhouette pixel for the edge gate), `min_cos` (the least |cos| between the blended normal and the view ray; squared here in float64 and
    rounded to float32: the kernel compares cos^2), `edge_gate`."""
    a = _lib.DifColourArgs()
    a.depth_tol = float(depth_tol)
    a.min_cos2 = float(np.float32(np.float64(min_cos) * np.float64(min_cos)))
    a.edge_gate, a.reserved = int(bool(edge_gate)), 0
    return a


def colour_accumulator(n_vertices: int, device) -> torch.Tensor:
    """A zeroed (V,4) uint64 accumulator for `colour_view` on `device` (allocated as int64 and viewed: the same bits)."""
    return torch.zeros((int(n_vertices), 4), dtype=torch.int64, device=device).view(torch.uint64)


def _check_mesh_arrays(vertices, normals, triangles, what: str):
    K = _check_triangles(triangles, what)
    _lib.require_cuda(vertices, normals)
    V = int(vertices.shape[0])
    if vertices.dtype != torch.float32 or normals.dtype != torch.float32:
        raise RuntimeError(f"{what}: vertices and normals must be float32")
    if tuple(vertices.shape) != (V, 3) or tuple(normals.shape) != (V, 3):
        raise RuntimeError(f"{what}: expected (V,3), (V,3); got {tuple(vertices.shape)}, {tuple(normals.shape)}")
    return V, K


def colour_view(vertices: torch.Tensor, normals: torch.Tensor, triangles: torch.Tensor, accum: torch.Tensor, rgb: torch.Tensor, pose, intrinsics,
                depth: Optional[torch.Tensor] = None, z_near: float = 0.05, cull_backfaces: bool = False, gates: Optional[_lib.DifColourArgs] = None,
                workspace: Optional[torch.Tensor] = None) -> dict:
    """The flat operator: ADDS the view `rgb` (H,W,3) f32 in [0,1] — with its depth frame `depth` (H,W) f32, or None — seen from the
    camera-to-world `pose` to `accum` (V,4) uint64 (zeroed by the caller before the first view), all on the GPU.  Height and width are those
    of `rgb`; pose, intrinsics, `z_near` and `cull_backfaces` as for `render`; `gates` from `colour_args` (default: its defaults).  Returns
    the view's counts: pixels used, no_hit, bad_colour, depth, edge, grazing (each pixel in exactly one), status.  One synchronisation."""
    V, K = _check_mesh_arrays(vertices, normals, triangles, "colour_view")
    _lib.require_cuda(accum, rgb, depth)
    if rgb.dtype != torch.float32 or rgb.dim() != 3 or rgb.shape[2] != 3:
        raise RuntimeError(f"colour_view: rgb must be (H,W,3) float32; got {tuple(rgb.shape)} {rgb.dtype}")
    H, W = int(rgb.shape[0]), int(rgb.shape[1])
    if depth is not None and (depth.dtype != torch.float32 or tuple(depth.shape) != (H, W)):
        raise RuntimeError(f"colour_view: depth must be ({H},{W}) float32 like rgb; got {tuple(depth.shape)} {depth.dtype}")
    if accum.dtype != torch.uint64 or tuple(accum.shape) != (V, 4):
        raise RuntimeError(f"colour_view: accum must be ({V},4) uint64; got {tuple(accum.shape)} {accum.dtype}")
    view = raster_args(pose, intrinsics, H, W, z_near, cull_backfaces)
    gates = colour_args() if gates is None else gates
    dev = triangles.device
    lib = _lib.load()
    ws_bytes = int(lib.dif_mesh_colour_workspace_bytes(V, K, H, W))
    if ws_bytes < 0:
        raise RuntimeError(f"libdifusion: dif_mesh_colour_view failed: {_lib.ERRORS[-1]}: cannot index {V} vertices, {K} triangles, {H} x {W} pixels "
                           "(the image must not be empty; V, 3 K and H W must stay below 2^31)")
    with torch.cuda.device(dev):
        if workspace is None or workspace.numel() < ws_bytes:
            workspace = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
        counts = torch.empty((_lib.COLOUR_COUNT,), dtype=torch.int32, device=dev)
        _lib.check(lib.dif_mesh_colour_view(_lib.ptr(vertices), _lib.ptr(normals), _lib.ptr(triangles), V, K, ctypes.byref(view), ctypes.byref(gates),
                                            _lib.ptr(rgb), _lib.ptr(depth), _lib.ptr(workspace), int(workspace.numel()), _lib.ptr(accum), _lib.ptr(counts),
                                            _lib.stream_ptr()), "dif_mesh_colour_view")
        c = counts.cpu().tolist()
    _check_status(c[_lib.COLOUR_STATUS], "dif_mesh_colour_view")
    return dict(zip(COLOUR_COUNT_NAMES, c))


def colour_resolve(accum: torch.Tensor, min_weight: float = 0.0):
    """The flat operator: `accum` (V,4) uint64 on the GPU -> (colors (V,3) uint8, color_weight (V,) f32, vertices coloured).  A vertex whose
    summed weight (in pixels: one pixel seen head-on at the vertex weighs 1) is below `min_weight`, or zero, is grey (128, 128, 128) and
    not counted.  One synchronisation (the count)."""
    _lib.require_cuda(accum)
    if accum.dtype != torch.uint64 or accum.dim() != 2 or accum.shape[1] != 4:
        raise RuntimeError(f"colour_resolve: accum must be (V,4) uint64; got {tuple(accum.shape)} {accum.dtype}")
    if not (min_weight >= 0.0) or min_weight >= 2.0 ** 47:
        raise RuntimeError(f"colour_resolve: min_weight must lie in [0, 2^47); got {min_weight}")
    V = int(accum.shape[0])
    dev = accum.device
    lib = _lib.load()
    least = int(np.ceil(np.float64(min_weight) * _lib.COLOUR_WEIGHT_ONE))          # S >= ceil(x) <=> S >= x for the integer S
    with torch.cuda.device(dev):
        colors = torch.empty((V, 3), dtype=torch.uint8, device=dev)
        weight = torch.empty((V,), dtype=torch.float32, device=dev)
        counts = torch.empty((1,), dtype=torch.int32, device=dev)
        _lib.check(lib.dif_mesh_colour_resolve(_lib.ptr(accum), V, least, _lib.ptr(colors), _lib.ptr(weight), _lib.ptr(counts), _lib.stream_ptr()),
                   "dif_mesh_colour_resolve")
        n = int(counts.cpu()[0])
    return colors, weight, n


class MeshColourer:
    """The colour accumulator of one `IndexedMesh`: `accum` (V,4) uint64 on the mesh's device (sum w r, sum w g, sum w b, sum w per vertex),
    zeroed here; `views` = how many views went in.  The sums are integers, so the order of the views does not matter."""

    def __init__(self, mesh: IndexedMesh):
        _check_mesh_arrays(mesh.vertices, mesh.normals, mesh.triangles, "colourer")
        self.mesh = mesh
        self.views = 0
        with torch.cuda.device(mesh.triangles.device):
            self.accum = colour_accumulator(int(mesh.vertices.shape[0]), mesh.triangles.device)
        self._ws = None

    def add_view(self, rgb: torch.Tensor, pose, intrinsics, depth: Optional[torch.Tensor] = None, z_near: float = 0.05, cull_backfaces: bool = False,
                 **gates) -> dict:
        """Adds one keyframe (`colour_view`; `gates`: the keywords of `colour_args`) and returns its counts."""
        m = self.mesh
        H, W = int(rgb.shape[0]), int(rgb.shape[1])
        need = int(_lib.load().dif_mesh_colour_workspace_bytes(int(m.vertices.shape[0]), int(m.triangles.shape[0]), H, W))
        if need > 0 and (self._ws is None or self._ws.numel() < need):
            with torch.cuda.device(m.triangles.device):
                self._ws = torch.empty((need,), dtype=torch.uint8, device=m.triangles.device)
        c = colour_view(m.vertices, m.normals, m.triangles, self.accum, rgb, pose, intrinsics, depth, z_near, cull_backfaces, colour_args(**gates), self._ws)
        self.views += 1
        return c

    def resolve(self, min_weight: float = 0.0) -> IndexedMesh:
        """A new `IndexedMesh` that shares this mesh's geometry tensors and carries `colors`, `color_weight` and `counts["coloured"]`; vertices
        that no view saw (or saw with less than `min_weight`) are grey.  More views may be added afterwards, and resolved again."""
        m = self.mesh
        colors, weight, n = colour_resolve(self.accum, min_weight)
        return IndexedMesh(m.vertices, m.normals, m.vertex_std, m.triangles, m.triangle_flatten_id, dict(m.counts, coloured=n), colors, weight)


# ---- closest point (DESIGN.md "Closest point on an indexed mesh") ----------------------------------------------------------------------
LOCATOR_COUNT_NAMES = ("indexed", "large", "degenerate", "skipped", "bad_index", "pairs", "cells", "status")
CLOSEST_COUNT_NAMES = ("found", "far", "bad_point", "status")


def default_locator_cell(vertices: torch.Tensor, triangles: torch.Tensor) -> float:
    """Twice the mean longest box side of the triangles whose indices are in range and whose vertices are finite (not only the usable ones:
    a degenerate triangle counts, one beyond the key range too; no answer depends on the cell), from an INTEGER sum (sides in
    units of 2^-20, rounded, summed in int64: the same on every run), as a float32 value; 1.0 when there is no such triangle.  Any cell gives
    the same answers; this one keeps a triangle in about 2^3 cells or fewer.  One read-back."""
    V = int(vertices.shape[0])
    with torch.cuda.device(triangles.device):
        t = triangles.long()
        valid = ((t >= 0) & (t < V)).all(dim=1)
        if V == 0 or t.shape[0] == 0:
            return 1.0
        p = vertices[torch.where(valid[:, None], t, torch.zeros_like(t))]            # (K, corner, axis)
        side = (p.max(dim=1).values - p.min(dim=1).values).max(dim=1).values.double()
        good = valid & torch.isfinite(side) & (side < 2.0 ** 40)
        total = torch.round(torch.where(good, side, torch.zeros_like(side)) * 2.0 ** 20).long().sum()
        total, n = torch.stack([total, good.sum()]).cpu().tolist()
    cell = np.float32(2.0 * (float(total) / n) / 2.0 ** 20) if n else np.float32(1.0)
    return float(cell) if cell > 0 else 1.0


class MeshClosest:
    """d2 (N,) f32 (inf: nothing within max_distance), triangle (N,) i32 (-1), point (N,3) f32 (NaN), barycentric (N,3) f32 (NaN; the weights
    of the triangle's three vertices in index order) — device tensors, `.cpu()` for a host copy — `distance` = sqrt(d2), and `counts`: found,
    far, bad_point (a query that is not finite or outside the grid's key range), status."""

    def __init__(self, d2, triangle, point, barycentric, counts: dict):
        self.d2 = d2
        self.triangle = triangle
        self.point = point
        self.barycentric = barycentric
        self.counts = dict(counts)

    @property
    def distance(self) -> torch.Tensor:
        return torch.sqrt(self.d2)

    def cpu(self) -> "MeshClosest":
        return MeshClosest(self.d2.cpu(), self.triangle.cpu(), self.point.cpu(), self.barycentric.cpu(), self.counts)


class MeshLocator:
    """The grid over one mesh's triangles (`locator`): `workspace` (device bytes; it holds a copy of every usable triangle, so the mesh arrays
    may go), `args`, `n_triangles`, and `counts`: triangles indexed / on the large list / degenerate / skipped (not finite, or outside the key
    range) / bad_index, the (triangle, cell) pairs, the distinct cells, `cell` (the float32 the kernel saw), `max_cells`, status (may hold
    `_lib.MESH_STATUS_BAD_INDEX`)."""

    def __init__(self, workspace: torch.Tensor, args: _lib.DifLocatorArgs, n_triangles: int, counts: dict):
        self.workspace = workspace
        self.args = args
        self.n_triangles = int(n_triangles)
        self.counts = dict(counts)

    def closest(self, points: torch.Tensor, max_distance: float) -> MeshClosest:
        """points (N,3) or (N,>=3) f32 on the GPU (the first three columns are read: an (N,6) xyz + normal cloud goes as it is) -> `MeshClosest`:
        per point the triangle that minimises (d2, triangle index) among those with d2 <= max_distance^2 — a point exactly at `max_distance` is
        found.  The answer does not depend on the cell; the time grows with (max_distance / cell)^3 for points that find nothing, and depends on
        how coherent the order of the points is.  One synchronisation (the counts)."""
        _lib.require_cuda(points)
        if points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] < 3:
            raise RuntimeError(f"closest: points must be (N,>=3) float32; got {tuple(points.shape)} {points.dtype}")
        if points.device != self.workspace.device:
            raise RuntimeError(f"closest: points live on {points.device}, the locator on {self.workspace.device}")
        r = float(np.float32(max_distance))
        if not (r > 0.0 and np.isfinite(r)):
            raise ValueError(f"closest: max_distance must be positive and finite (as float32); got {max_distance}")
        if r / float(self.args.cell) > _lib.LOCATOR_MAX_RATIO:
            raise ValueError(f"closest: max_distance / cell = {r / float(self.args.cell):.1f} is beyond the ring limit {_lib.LOCATOR_MAX_RATIO}: "
                             "build the locator with a larger cell (`locator(cell=...)`, `closest(..., cell=...)`)")
        N, stride = int(points.shape[0]), int(points.shape[1])
        dev = points.device
        lib = _lib.load()
        with torch.cuda.device(dev):
            d2 = torch.empty((N,), dtype=torch.float32, device=dev)
            tri = torch.empty((N,), dtype=torch.int32, device=dev)
            point = torch.empty((N, 3), dtype=torch.float32, device=dev)
            bary = torch.empty((N, 3), dtype=torch.float32, device=dev)
            counts = torch.empty((_lib.CLOSEST_COUNT,), dtype=torch.int32, device=dev)
            _lib.check(lib.dif_mesh_closest(ctypes.byref(self.args), self.n_triangles, _lib.ptr(self.workspace), int(self.workspace.numel()), _lib.ptr(points), N,
                                            stride, r, _lib.ptr(d2), _lib.ptr(tri), _lib.ptr(point), _lib.ptr(bary), _lib.ptr(counts), _lib.stream_ptr()),
                       "dif_mesh_closest")
            c = counts.cpu().tolist()
        if c[_lib.CLOSEST_STATUS] != 0:
            raise RuntimeError(f"libdifusion: dif_mesh_closest reported status {c[_lib.CLOSEST_STATUS]} (the locator was not built)")
        return MeshClosest(d2, tri, point, bary, dict(zip(CLOSEST_COUNT_NAMES, c)))


def locator_args(cell: float, pair_capacity: int, max_cells: Optional[int] = None) -> _lib.DifLocatorArgs:
    a = _lib.DifLocatorArgs()
    a.cell = float(cell)
    a.max_cells = 0 if max_cells is None else int(max_cells)
    a.pair_capacity = int(pair_capacity)
    if not (a.cell > 0.0 and np.isfinite(a.cell)):
        raise ValueError(f"locator: cell must be positive and finite (as float32); got {cell}")
    if a.max_cells > 2 ** 20:
        raise ValueError(f"locator: max_cells must not pass 2^20; got {max_cells}")
    return a


def locator(vertices: torch.Tensor, triangles: torch.Tensor, cell: Optional[float] = None, pair_capacity: Optional[int] = None,
            max_cells: Optional[int] = None) -> MeshLocator:
    """The flat operator: vertices (V,3) f32 and triangles (K,3) i32 on the GPU -> `MeshLocator` (`dif_mesh_locator_build`, include/difusion.h has
    the contract).  `cell`: the edge of the grid's cubes, default `default_locator_cell` — no answer depends on it.  `pair_capacity`: room for
    the (triangle, cell) pairs, default 8 K; when the mesh needs more the build reports how many and is repeated ONCE with that number (the
    grow-and-retry of `extract_mesh_arrays`).  `max_cells`: a triangle whose box covers more cells goes to the large list that every query walks
    (default 64; negative: every triangle, the all-pairs search).  One synchronisation per build (the counts), one more for the default cell."""
    K = _check_triangles(triangles, "locator")
    _lib.require_cuda(vertices)
    V = int(vertices.shape[0])
    if vertices.dtype != torch.float32 or tuple(vertices.shape) != (V, 3):
        raise RuntimeError(f"locator: vertices must be (V,3) float32; got {tuple(vertices.shape)} {vertices.dtype}")
    if vertices.device != triangles.device:
        raise RuntimeError(f"locator: vertices live on {vertices.device}, triangles on {triangles.device}")
    if pair_capacity is not None and int(pair_capacity) < 1:
        raise ValueError(f"locator: pair_capacity must be at least 1; got {pair_capacity}")
    if cell is None:
        cell = default_locator_cell(vertices, triangles)
    capacity = max(1024, 8 * K) if pair_capacity is None else int(pair_capacity)
    dev = triangles.device
    lib = _lib.load()
    for attempt in range(2):
        args = locator_args(cell, capacity, max_cells)
        ws_bytes = int(lib.dif_mesh_locator_workspace_bytes(V, K, capacity))
        if ws_bytes < 0:
            raise RuntimeError(f"libdifusion: dif_mesh_locator_build cannot index {V} vertices, {K} triangles, {capacity} pairs (V and 3 K must stay "
                               "below 2^31, the pairs below 2^28)")
        with torch.cuda.device(dev):
            ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
            counts = torch.empty((_lib.LOCATOR_COUNT,), dtype=torch.int32, device=dev)
            _lib.check(lib.dif_mesh_locator_build(_lib.ptr(vertices), _lib.ptr(triangles), V, K, ctypes.byref(args), _lib.ptr(ws), ws_bytes, _lib.ptr(counts),
                                                  _lib.stream_ptr()), "dif_mesh_locator_build")
            c = counts.cpu().tolist()
        if not (c[_lib.LOCATOR_STATUS] & _lib.MESH_STATUS_PAIR_OVERFLOW):
            break
        capacity = c[_lib.LOCATOR_PAIRS]                                          # the exact number; one retry
    status = c[_lib.LOCATOR_STATUS]
    if status & ~_lib.MESH_STATUS_BAD_INDEX:
        raise RuntimeError(f"libdifusion: dif_mesh_locator_build reported status {status} ({c[_lib.LOCATOR_PAIRS]} pairs needed, room for {capacity})")
    out = dict(zip(LOCATOR_COUNT_NAMES, c), cell=float(args.cell), max_cells=int(args.max_cells) if args.max_cells else _lib.LOCATOR_MAX_CELLS)
    return MeshLocator(ws, args, K, out)


def interpolate(triangles: torch.Tensor, closest_triangle: torch.Tensor, barycentric: torch.Tensor, values: torch.Tensor) -> torch.Tensor:
    """The flat operator behind `IndexedMesh.interpolate`: plain torch indexing on the device, float32, (b0 x0 + b1 x1) + b2 x2."""
    found = closest_triangle >= 0
    corners = triangles.long()[closest_triangle.long().clamp(min=0)]                # (N,3)
    x = values[corners]                                                           # (N,3) or (N,3,C)
    b = barycentric if values.dim() == 1 else barycentric[:, :, None]
    out = (b[:, 0] * x[:, 0] + b[:, 1] * x[:, 1]) + b[:, 2] * x[:, 2]
    nan = torch.full_like(out, float("nan"))
    return torch.where(found if values.dim() == 1 else found[:, None], out, nan)


def _sampled_distance(points: torch.Tensor, drawn: int, target: IndexedMesh, max_distance: float, cell: Optional[float], taus) -> dict:
    """One direction of `IndexedMesh.compare`: `points` (the first `drawn` rows are samples) against `target`'s surface."""
    nan = float("nan")
    if drawn == 0:
        return dict(mean=nan, rms=nan, median=nan, max=nan, found=0, far=0, within=[0] * len(taus))
    if cell is None:
        r = float(np.float32(max_distance))
        cell = default_locator_cell(target.vertices, target.triangles)
        if np.isfinite(r) and r > 0.0:
            cell = max(cell, float(np.float32(r / (_lib.LOCATOR_MAX_RATIO - 1))))
    c = target.locator(cell).closest(points, max_distance)
    with torch.cuda.device(points.device):
        d = torch.sqrt(c.d2[torch.isfinite(c.d2)].double())
        within = [(d <= t).sum().double() for t in taus]
        if d.numel() > 0:
            stats = torch.stack([d.mean(), torch.sqrt((d * d).mean()), d.median(), d.max()] + within).cpu().tolist()
        else:
            stats = [nan] * 4 + [0.0] * len(taus)
    return dict(mean=stats[0], rms=stats[1], median=stats[2], max=stats[3], found=c.counts["found"], far=c.counts["far"] + c.counts["bad_point"],
                within=[int(w) for w in stats[4:]])


# ---- sampling (DESIGN.md "Sampling an indexed mesh") -----------------------------------------------------------------------------------
SAMPLER_COUNT_NAMES = ("weighted", "weightless", "skipped", "bad_index", "exponent", "status")
SAMPLE_COUNT_NAMES = ("samples", "status")


class MeshSamples:
    """point (N,3) f32, triangle (N,) i32, barycentric (N,3) f32 (the weights of the triangle's three vertices in index order) — device tensors,
    `.cpu()` for a host copy — in ascending triangle order, and `counts`: samples (N, or 0 when the mesh has no area: every row is then NaN / -1 /
    NaN), status.  `triangle` and `barycentric` are what `IndexedMesh.interpolate` reads: `mesh.interpolate(samples, mesh.normals)`."""

    def __init__(self, point, triangle, barycentric, counts: dict):
        self.point = point
        self.triangle = triangle
        self.barycentric = barycentric
        self.counts = dict(counts)

    def cpu(self) -> "MeshSamples":
        return MeshSamples(self.point.cpu(), self.triangle.cpu(), self.barycentric.cpu(), self.counts)


class MeshSampler:
    """The weights of one mesh's triangles (`sampler`): `workspace` (device bytes: the prefix sums), the mesh arrays it was built from (read again
    by every draw), `counts` — triangles weighted / weightless (degenerate, or 2^32 times smaller than the largest: they get no samples) / skipped
    (not finite, or a coordinate of 2^60) / bad_index, the exponent e of the largest doubled area, status (may hold `_lib.MESH_STATUS_BAD_INDEX`)
    — `total` = T, the sum of the integer weights, and `area` = 0.5 T 2^(e - 32): the float64 area of the float32 vertices, short by less than
    2^(e - 33) per triangle."""

    def __init__(self, workspace: torch.Tensor, vertices: torch.Tensor, triangles: torch.Tensor, counts: dict, total: int):
        self.workspace = workspace
        self.vertices = vertices
        self.triangles = triangles
        self.counts = dict(counts)
        self.total = int(total)
        self.area = float(np.ldexp(float(self.total), int(self.counts["exponent"]) - 33))

    def sample(self, n: int, seed: int = 0) -> MeshSamples:
        """`n` stratified samples (0 <= n < 2^31) -> `MeshSamples`: sample j lies in the j-th of n equal parts of the summed weights, so a triangle
        of weight w gets within 2 of n w / T samples, whatever the seed; the seed (any integer, taken modulo 2^64) moves the samples inside their
        strata and on their triangles.  Stratified jitter, not blue noise.  One synchronisation (the counts)."""
        n = int(n)
        if n < 0 or n >= 2 ** 31:
            raise ValueError(f"sample: n must be in [0, 2^31); got {n}")
        V, K = int(self.vertices.shape[0]), int(self.triangles.shape[0])
        dev = self.workspace.device
        lib = _lib.load()
        with torch.cuda.device(dev):
            point = torch.empty((n, 3), dtype=torch.float32, device=dev)
            tri = torch.empty((n,), dtype=torch.int32, device=dev)
            bary = torch.empty((n, 3), dtype=torch.float32, device=dev)
            counts = torch.empty((_lib.SAMPLE_COUNT,), dtype=torch.int32, device=dev)
            _lib.check(lib.dif_mesh_sample(_lib.ptr(self.vertices), _lib.ptr(self.triangles), V, K, _lib.ptr(self.workspace), int(self.workspace.numel()), n,
                                           int(seed) & (2 ** 64 - 1), _lib.ptr(point), _lib.ptr(tri), _lib.ptr(bary), _lib.ptr(counts), _lib.stream_ptr()),
                       "dif_mesh_sample")
            c = counts.cpu().tolist()
        if c[_lib.SAMPLE_STATUS] & ~_lib.MESH_STATUS_BAD_INDEX or c[_lib.SAMPLE_STATUS] != self.counts["status"]:
            raise RuntimeError(f"libdifusion: dif_mesh_sample reported status {c[_lib.SAMPLE_STATUS]} (the sampler was not built for this mesh)")
        return MeshSamples(point, tri, bary, dict(zip(SAMPLE_COUNT_NAMES, c)))


def sampler(vertices: torch.Tensor, triangles: torch.Tensor) -> MeshSampler:
    """The flat operator: vertices (V,3) f32 and triangles (K,3) i32 on the GPU -> `MeshSampler` (`dif_mesh_sampler_build`, include/difusion.h has
    the contract).  The weight of a triangle is an INTEGER — its doubled area in double, scaled by a power of two so that the largest lies in
    [2^31, 2^32), floored — so the prefix sums are exact and the same on every run.  One synchronisation (the counts and T)."""
    K = _check_triangles(triangles, "sampler")
    _lib.require_cuda(vertices)
    V = int(vertices.shape[0])
    if vertices.dtype != torch.float32 or tuple(vertices.shape) != (V, 3):
        raise RuntimeError(f"sampler: vertices must be (V,3) float32; got {tuple(vertices.shape)} {vertices.dtype}")
    if vertices.device != triangles.device:
        raise RuntimeError(f"sampler: vertices live on {vertices.device}, triangles on {triangles.device}")
    dev = triangles.device
    lib = _lib.load()
    ws_bytes = int(lib.dif_mesh_sampler_workspace_bytes(V, K))
    if ws_bytes < 0:
        raise RuntimeError(f"libdifusion: dif_mesh_sampler_build cannot index {V} vertices, {K} triangles (V and 3 K must stay below 2^31)")
    with torch.cuda.device(dev):
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
        back = torch.empty((_lib.SAMPLER_COUNT // 2 + 1,), dtype=torch.int64, device=dev)      # the counts (int32) and T behind them: one read-back
        _lib.check(lib.dif_mesh_sampler_build(_lib.ptr(vertices), _lib.ptr(triangles), V, K, _lib.ptr(ws), ws_bytes, _lib.ptr(back),
                                              ctypes.c_void_p(back.data_ptr() + 4 * _lib.SAMPLER_COUNT), _lib.stream_ptr()), "dif_mesh_sampler_build")
        host = back.cpu()
    c = host[:_lib.SAMPLER_COUNT // 2].view(torch.int32).tolist()
    total = int(host[-1].item()) & (2 ** 64 - 1)
    return MeshSampler(ws, vertices, triangles, dict(zip(SAMPLER_COUNT_NAMES, c)), total)


# ---- reading a PLY ---------------------------------------------------------------------------------------------------------------------
_PLY_SCALARS = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "<i2", "int16": "<i2", "ushort": "<u2", "uint16": "<u2",
                "int": "<i4", "int32": "<i4", "uint": "<u4", "uint32": "<u4", "float": "<f4", "float32": "<f4", "double": "<f8", "float64": "<f8"}


def read_ply(path, device="cuda") -> IndexedMesh:
    """A binary little-endian PLY as an `IndexedMesh` on `device` (numpy alone): the other mesh of a comparison, or what `write_ply` wrote, array
    for array and bit for bit.  Vertex properties: scalars of any PLY type in any order; `x y z` are required and, like `nx ny nz` and
    `quality` (-> vertex_std), taken as float32 — bit for bit when the file holds `float`; `red green blue` as uint8 when they are `uchar` (with
    color_weight 1).  Without them normals and std are zero and colours None.  Faces: `property list uchar int|uint vertex_indices` (or
    `vertex_index`), triangles only.  `triangle_flatten_id` is -1.  Elements after the faces are not read.  Anything else — ASCII, big-endian,
    a list property on a vertex, another face layout, a face that is not a triangle, a truncated file — raises ValueError and names what it found."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.find(b"end_header\n")
    if not data.startswith(b"ply") or end < 0:
        raise ValueError(f"read_ply: {path}: not a PLY file (no 'ply' magic or no end_header)")
    lines = [ln.strip() for ln in data[:end].decode("ascii", errors="replace").splitlines()]
    body = end + len(b"end_header\n")
    fmt = [ln.split() for ln in lines if ln.startswith("format")]
    if not fmt or fmt[0][1:] != ["binary_little_endian", "1.0"]:
        raise ValueError(f"read_ply: {path}: only 'format binary_little_endian 1.0' is read; found {' '.join(fmt[0]) if fmt else 'no format line'!r}")
    elements = []                                                                 # [name, count, [property tokens]]
    for ln in lines:
        tok = ln.split()
        if tok[:1] == ["element"]:
            elements.append([tok[1], int(tok[2]), []])
        elif tok[:1] == ["property"]:
            if not elements:
                raise ValueError(f"read_ply: {path}: a property before any element: {ln!r}")
            elements[-1][2].append(tok[1:])
    names = [e[0] for e in elements]
    if names[:2] != ["vertex", "face"]:
        raise ValueError(f"read_ply: {path}: the first two elements must be vertex and face; found {names}")
    (_, V, vprops), (_, K, fprops) = elements[:2]
    fields = []
    for p in vprops:
        if p[0] == "list" or p[0] not in _PLY_SCALARS or len(p) != 2:
            raise ValueError(f"read_ply: {path}: vertex properties must be scalars; found 'property {' '.join(p)}'")
        fields.append((p[1], _PLY_SCALARS[p[0]]))
    have = [n for n, _ in fields]
    if len(set(have)) != len(have) or not all(k in have for k in "xyz"):
        raise ValueError(f"read_ply: {path}: the vertex needs x, y and z, each once; found {have}")
    if len(fprops) != 1 or fprops[0][0] != "list" or len(fprops[0]) != 4 or fprops[0][1] not in ("uchar", "uint8") or \
            fprops[0][2] not in ("int", "int32", "uint", "uint32") or fprops[0][3] not in ("vertex_indices", "vertex_index"):
        raise ValueError(f"read_ply: {path}: faces must be 'property list uchar int|uint vertex_indices'; found {[' '.join(p) for p in fprops]}")
    vdt = np.dtype(fields)
    fdt = np.dtype([("n", "u1"), ("v", _PLY_SCALARS[fprops[0][2]], (3,))])
    need_v = V * vdt.itemsize
    if len(data) - body < need_v:
        raise ValueError(f"read_ply: {path}: truncated: {V} vertices of {vdt.itemsize} bytes need {need_v} bytes, the file has {len(data) - body} after its header")
    vert = np.frombuffer(data, dtype=vdt, count=V, offset=body)
    # (a face that is not a triangle shifts every later one: look at the counts one face at a time, as far as the file goes)
    avail = (len(data) - body - need_v) // fdt.itemsize
    face = np.frombuffer(data, dtype=fdt, count=min(K, avail), offset=body + need_v)
    wrong = np.nonzero(face["n"] != 3)[0]
    if wrong.size:
        raise ValueError(f"read_ply: {path}: face {int(wrong[0])} has {int(face['n'][wrong[0]])} vertices; only triangles are read")
    if avail < K:
        raise ValueError(f"read_ply: {path}: truncated: {K} faces of {fdt.itemsize} bytes need {K * fdt.itemsize} bytes, the file has {len(data) - body - need_v} after "
                         "its vertices")
    tri = face["v"]
    if tri.dtype.kind == "u" and K and int(tri.max()) >= 2 ** 31:
        raise ValueError(f"read_ply: {path}: a vertex index of {int(tri.max())} does not fit int32")

    def column(keys, default):
        if all(k in have for k in keys):
            return np.ascontiguousarray(np.stack([vert[k].astype(np.float32) for k in keys], axis=1))
        return np.full((V, len(keys)), default, dtype=np.float32)

    rgb = ("red", "green", "blue")
    coloured = all(k in have and vdt[k] == np.uint8 for k in rgb)
    dev = torch.device(device)
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return IndexedMesh(put(column("xyz", 0.0)), put(column(("nx", "ny", "nz"), 0.0)), put(column(("quality",), 0.0)[:, 0]), put(tri.astype(np.int32)),
                       put(np.full((K,), -1, dtype=np.int64)), dict(vertices=V, triangles=K, status=0),
                       put(np.stack([vert[k] for k in rgb], axis=1)) if coloured else None,
                       put(np.ones((V,), dtype=np.float32)) if coloured else None)
