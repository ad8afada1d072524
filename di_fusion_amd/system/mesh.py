"""Indexed mesh: the triangle soup of the mesh cache welded by lattice edge, with area-weighted vertex normals (`dif_mesh_weld`), and a PLY
writer.  No reference counterpart: the reference hands its soup to Open3D (`merge_close_vertices`, `compute_vertex_normals`, commented out in
its main loop as too slow).  The key rule and why the weld is not by position: DESIGN.md "Indexed mesh".
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
    kept, triangles dropped (a repeated index after welding), unkeyed soup corners (not on the lattice: each a vertex of its own), status."""

    def __init__(self, vertices, normals, vertex_std, triangles, triangle_flatten_id, counts: dict):
        self.vertices = vertices
        self.normals = normals
        self.vertex_std = vertex_std
        self.triangles = triangles
        self.triangle_flatten_id = triangle_flatten_id
        self.counts = dict(counts)

    def cpu(self) -> "IndexedMesh":
        return IndexedMesh(self.vertices.cpu(), self.normals.cpu(), self.vertex_std.cpu(), self.triangles.cpu(), self.triangle_flatten_id.cpu(),
                           self.counts)

    def write_ply(self, path):
        """Binary little-endian PLY: x y z nx ny nz quality (= std) as float32 per vertex, faces as uchar count + three int indices."""
        v = self.vertices.cpu().numpy()
        vert = np.empty((v.shape[0],), dtype=[(n, "<f4") for n in ("x", "y", "z", "nx", "ny", "nz", "quality")])
        n = self.normals.cpu().numpy()
        for k, name in enumerate(("x", "y", "z")):
            vert[name] = v[:, k]
            vert["n" + name] = n[:, k]
        vert["quality"] = self.vertex_std.cpu().numpy()
        t = self.triangles.cpu().numpy()
        face = np.empty((t.shape[0],), dtype=[("n", "u1"), ("v", "<i4", (3,))])
        face["n"] = 3
        face["v"] = t
        header = ("ply\nformat binary_little_endian 1.0\ncomment di_fusion_amd indexed mesh\n"
                  f"element vertex {vert.shape[0]}\n" + "".join(f"property float {name}\n" for name in vert.dtype.names) +
                  f"element face {face.shape[0]}\nproperty list uchar int vertex_indices\nend_header\n")
        with open(path, "wb") as f:
            f.write(header.encode("ascii"))
            f.write(vert.tobytes())
            f.write(face.tobytes())

    def to_open3d(self):
        """`open3d.geometry.TriangleMesh` with vertex normals (raises ImportError without Open3D)."""
        import open3d as o3d
        m = o3d.geometry.TriangleMesh()
        m.vertices = o3d.utility.Vector3dVector(self.vertices.cpu().numpy().astype(np.float64))
        m.triangles = o3d.utility.Vector3iVector(self.triangles.cpu().numpy())
        m.vertex_normals = o3d.utility.Vector3dVector(self.normals.cpu().numpy().astype(np.float64))
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
