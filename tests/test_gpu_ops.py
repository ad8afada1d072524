"""GPU parity of the flat ops (through the C ABI) against the oracle and the golden vectors of the reference."""
import numpy as np
import pytest
import torch

from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def test_library_loaded_and_version():
    from di_fusion_amd import _lib
    assert _lib.load().dif_version() == 100


def test_cpu_tensor_is_rejected(gpu_model):
    from di_fusion_amd.system import ext
    with pytest.raises(RuntimeError):
        ext.unproject_depth(torch.zeros((4, 4)), 1.0, 1.0, 0.0, 0.0)


def test_unproject_bit_exact():
    from di_fusion_amd.system import ext
    from oracle import difusion_oracle as O
    g = np.random.default_rng(0)
    d = (g.random((480, 640), dtype=np.float32) * 4 + 0.5).astype(np.float32)
    d[g.random((480, 640)) < 0.1] = np.nan
    got = ext.unproject_depth(_t(d), 481.2, 480.0, 319.5, 239.5).cpu().numpy()
    want = O.unproject_depth(d, 481.2, 480.0, 319.5, 239.5)
    assert np.array_equal(got, want, equal_nan=True)


def test_unproject_transform_bit_exact():
    from di_fusion_amd import _lib, synthetic as syn
    import ctypes
    intr = syn.Intrinsic()
    R, t = syn.orbit_pose(7)
    depth, ncam = syn.render_frame(syn.default_room(), R, t, intr)
    H, W = depth.shape
    xyz = torch.empty((H * W, 3), device=DEV); nrm = torch.empty((H * W, 3), device=DEV)
    Rf = (ctypes.c_float * 9)(*[float(np.float32(v)) for v in R.reshape(-1)])
    tf = (ctypes.c_float * 3)(*[float(np.float32(v)) for v in t])
    d, n = depth.to(DEV), ncam.to(DEV)
    _lib.check(_lib.load().dif_unproject_transform(_lib.ptr(d), _lib.ptr(n), _lib.ptr(xyz), _lib.ptr(nrm), H, W, intr.fx, intr.fy, intr.cx,
                                                   intr.cy, Rf, tf, _lib.stream_ptr()), "unproject_transform")
    ok = ~torch.isnan(xyz[:, 0])
    want_xyz, want_nrm = syn.frame_points(syn.default_room(), 7, intr)
    assert torch.equal(xyz[ok].cpu(), want_xyz)
    assert torch.equal(nrm[ok].cpu(), want_nrm)


def test_compute_normal_weight():
    from di_fusion_amd.system import ext
    from di_fusion_amd import synthetic as syn
    from oracle import difusion_oracle as O
    intr = syn.Intrinsic().scaled(0.1)
    R, t = syn.orbit_pose(0)
    depth, _ = syn.render_frame(syn.default_room(), R, t, intr)
    pc = O.unproject_depth(depth.numpy(), intr.fx, intr.fy, intr.cx, intr.cy)
    pc[np.isnan(pc)] = 0.0
    got = ext.compute_normal_weight(_t(pc)).cpu().numpy()
    want = O.compute_normal_weight(pc)
    valid = want[..., 3] > 0
    assert np.array_equal(got[..., 3] > 0, valid)
    assert np.abs(got[valid] - want[valid]).max() / np.abs(want[valid]).max() < 1e-4
    # the normals on their own (the bound above is relative to the largest WEIGHT, several hundred): differences, products, one sqrtf and
    # three divisions, all correctly rounded on both sides (tests/test_gpu_frontend_envelope.py holds them to the restatement's bits)
    assert np.abs(got[valid][:, :3] - want[valid][:, :3]).max() < 1e-6
    assert (got[~valid][:, 3] == -1).all()


def test_groupby_sum():
    from di_fusion_amd.system import ext
    from oracle import difusion_oracle as O
    g = np.random.default_rng(1)
    vals = g.standard_normal((5000, 29)).astype(np.float32)
    idx = g.integers(0, 37, 5000).astype(np.int64)
    s, c = ext.groupby_sum(_t(vals), _t(idx), 37)
    ws, wc = O.groupby_sum(vals, idx, 37)
    assert np.array_equal(c.cpu().numpy(), wc)
    assert np.abs(s.cpu().numpy() - ws).max() < 1e-3      # float atomics: order differs


def test_decoder_rows_vs_golden(gpu_model):
    g = np.load(GOLDEN / "networks.npz")
    sdf, std = gpu_model.decoder(_t(g["dec_x"]))
    ds = np.abs(sdf.cpu().numpy() - g["dec_sdf"]).max()
    dd = np.abs(std.cpu().numpy() - g["dec_std"]).max()
    print(f"decoder vs reference: sdf {ds:.3e} std {dd:.3e}")
    assert ds < 1e-5 and dd < 1e-5           # stated tolerance: 1e-5 abs


def test_decoder_rows_ragged_sizes(gpu_model, oracle_net):
    g = np.random.default_rng(3)
    for n in (1, 31, 32, 33, 1000, 4097):
        x = np.concatenate([g.standard_normal((n, 29)) * 0.3, g.random((n, 3)) * 2 - 1], 1).astype(np.float32)
        sdf, std = gpu_model.decoder(_t(x))
        ws, wd = oracle_net.decoder(x)
        assert np.abs(sdf.cpu().numpy() - ws).max() < 1e-5, n
        assert np.abs(std.cpu().numpy() - wd).max() < 1e-5, n


def test_encoder_rows_vs_golden(gpu_model):
    g = np.load(GOLDEN / "networks.npz")
    out = gpu_model.encoder(_t(g["enc_x"])).cpu().numpy()
    d = np.abs(out - g["enc_out"]).max()
    print(f"encoder vs reference: {d:.3e}")
    assert d < 2e-5


def test_marching_cubes_flat_vs_oracle_on_golden_cubes():
    """The reference's own MC argument tuple (recorded by the golden generator) through both implementations."""
    from di_fusion_amd.system import ext
    from oracle import difusion_oracle as O
    g = np.load(GOLDEN / "seq_small.npz")
    n_xyz = g["n_xyz"].tolist()
    for f in range(int(g["n_frames"])):
        indexer = -np.ones(int(np.prod(n_xyz)), dtype=np.int64)
        indexer[g[f"f{f}_int_indexer_nz"]] = g[f"f{f}_int_indexer_val"]
        vb, vbm = g[f"f{f}_mc_valid_blocks"], g[f"f{f}_mc_vec_batch_mapping"]
        cs, cd = g[f"f{f}_mc_cube_sdf"], g[f"f{f}_mc_cube_std"]
        for max_std in (0.15, 2000.0):
            wt, wi, ws = O.marching_cubes_interp(indexer.reshape(n_xyz), vb, vbm, cs, cd, int(4e6), n_xyz, max_std)
            tri, tid, tstd = ext.marching_cubes_interp(_t(indexer.reshape(n_xyz)), _t(vb), _t(vbm), _t(cs), _t(cd), int(4e6), n_xyz, max_std)
            assert tri.shape[0] == wt.shape[0], (f, max_std, tri.shape, wt.shape)
            assert np.array_equal(tid.cpu().numpy(), wi)
            assert np.abs(tri.cpu().numpy() - wt).max() < 1e-5
            assert np.abs(tstd.cpu().numpy() - ws).max() < 1e-5
        assert wt.shape[0] > 0


def test_marching_cubes_empty_and_truncation():
    from di_fusion_amd.system import ext
    g = np.load(GOLDEN / "seq_small.npz")
    n_xyz = g["n_xyz"].tolist()
    indexer = -np.ones(int(np.prod(n_xyz)), dtype=np.int64)
    indexer[g["f0_int_indexer_nz"]] = g["f0_int_indexer_val"]
    vb, vbm = g["f0_mc_valid_blocks"], g["f0_mc_vec_batch_mapping"]
    cs, cd = g["f0_mc_cube_sdf"], g["f0_mc_cube_std"]
    tri, tid, tstd = ext.marching_cubes_interp(_t(indexer.reshape(n_xyz)), _t(vb[:0]), _t(vbm), _t(cs), _t(cd), 100, n_xyz, 0.15)
    assert tri.shape[0] == 0
    tri, tid, tstd = ext.marching_cubes_interp(_t(indexer.reshape(n_xyz)), _t(vb), _t(vbm), _t(cs), _t(cd), 50, n_xyz, 2000.0)
    assert tri.shape[0] == 50


def test_filter_depth_vs_oracle():
    from di_fusion_amd.system import ext
    from di_fusion_amd import synthetic as syn
    from oracle import difusion_oracle as O
    intr = syn.Intrinsic().scaled(0.1)
    R, t = syn.orbit_pose(0)
    depth, _ = syn.render_frame(syn.default_room(), R, t, intr, noise_seed=3)
    d = torch.nan_to_num(depth, nan=0.0).numpy()
    out = torch.full(d.shape, -7.0, device=DEV)
    ext.filter_depth(_t(d), out)
    want = O.filter_depth(d)
    got = out.cpu().numpy()
    assert (got[:2] == -7).all() and (got[-2:] == -7).all() and (got[:, :2] == -7).all() and (got[:, -2:] == -7).all()   # border untouched
    assert np.abs(got[2:-2, 2:-2] - want[2:-2, 2:-2]).max() < 1e-5


def test_point_box_filter_vs_oracle():
    from di_fusion_amd.system import ext
    from di_fusion_amd import synthetic as syn
    from oracle import difusion_oracle as O
    xyz, nrm = syn.frame_points(syn.default_room(), 3, syn.Intrinsic().scaled(0.5))
    fp, fn = ext.point_box_filter(xyz.to(DEV), nrm.to(DEV), 0.02)
    wp, wn = O.point_box_filter(xyz.numpy(), nrm.numpy(), 0.02)
    assert fp.shape == wp.shape and fp.shape[0] < xyz.shape[0]
    assert np.abs(fp.cpu().numpy() - wp).max() < 2e-6
    assert np.abs(fn.cpu().numpy() - wn).max() < 2e-6
    # scratch bitmap restored: a second call gives the same answer
    fp2, _ = ext.point_box_filter(xyz.to(DEV), nrm.to(DEV), 0.02)
    assert torch.equal(fp, fp2)
    with pytest.raises(RuntimeError):
        ext.point_box_filter(xyz.to(DEV), nrm.to(DEV), 0.02, max_cells=1 << 12)


def test_point_box_filter_vs_the_references_own():
    """The HIP operator against what the REFERENCE's `point_box_filter` (system/tracker.py:13-23, plain torch) returned for the same cloud
    (tests/golden/box_filter.npz): the same boxes in the same order, means within float32 rounding, at the tracker's 2 cm and at 5 cm."""
    from di_fusion_amd.system import ext
    from di_fusion_amd import synthetic as syn
    from tests.conftest import GOLDEN
    g = np.load(GOLDEN / "box_filter.npz")
    xyz, nrm = syn.frame_points(syn.default_room(), 3, syn.Intrinsic().scaled(0.5))
    assert xyz.size(0) == int(g["n"])
    for vs in (0.02, 0.05):
        fp, fn = ext.point_box_filter(xyz.to(DEV), nrm.to(DEV), vs)
        wp, wn = g[f"vs{int(vs * 100)}_points"], g[f"vs{int(vs * 100)}_normals"]
        assert tuple(fp.shape) == wp.shape
        assert np.abs(fp.cpu().numpy() - wp).max() < 2e-6 and np.abs(fn.cpu().numpy() - wn).max() < 2e-6


def test_depth_frontend_equals_the_three_kernel_composition():
    """8f-2: filter_depth -> unproject_depth -> compute_normal_weight fused into one LDS-tiled pass, at full resolution (640x480 and a
    size that is not a multiple of the tile), on a noisy frame with NaN holes, zeros and depth discontinuities: bit-identical to the
    three flat ops called one after the other (which are checked against the oracle above)."""
    from di_fusion_amd.system import ext
    from di_fusion_amd import synthetic as syn
    for scale, seed in ((1.0, 5), (0.3, 6)):
        intr = syn.Intrinsic().scaled(scale)
        R, t = syn.orbit_pose(11)
        depth, _ = syn.render_frame(syn.default_room(), R, t, intr, noise_seed=seed)
        g = torch.Generator().manual_seed(seed)
        hole = torch.rand(depth.shape, generator=g)
        depth = depth.clone()
        depth[hole < 0.02] = float("nan")
        depth[(hole > 0.02) & (hole < 0.04)] = 0.0
        d = depth.to(DEV)
        for filt in (True, False):
            want_d = d.clone()
            if filt:
                ext.filter_depth(d, want_d)
            want_pc = ext.unproject_depth(want_d, intr.fx, intr.fy, intr.cx, intr.cy)
            want_nw = ext.compute_normal_weight(want_pc)
            got_d, got_pc, got_nw, fd, fn = ext.depth_frontend(d, intr.fx, intr.fy, intr.cx, intr.cy, filter=filt, want_frame=True)
            def same(x, y):         # the same bits, or NaN on both sides (which operand's NaN payload survives an operation is the compiler's choice)
                x, y = x.contiguous(), y.contiguous()
                return bool(((x.view(torch.int32) == y.view(torch.int32)) | (torch.isnan(x) & torch.isnan(y))).all())
            assert same(got_d, want_d)
            assert same(got_pc, want_pc)
            assert same(got_nw[..., 3], want_nw[..., 3])
            valid = want_nw[..., 3] > 0
            assert valid.float().mean() > 0.2
            assert same(got_nw[valid], want_nw[valid])
            # the integrate-ready pair: depth + normal where a normal exists, NaN elsewhere
            use = valid & ~torch.isnan(want_nw[..., 0])
            assert torch.equal(torch.isnan(fd), ~use) and torch.equal(torch.isnan(fn[..., 0]), ~use)
            assert torch.equal(fd[use], want_d[use]) and torch.equal(fn[use], want_nw[..., :3][use])


def test_depth_only_stream_integrates(gpu_model):
    """A stream that comes WITHOUT normals: depth -> `depth_frontend` -> frame descriptor -> `dif_integrate_frame` (a1 + a2 + a3..a10)."""
    import ctypes
    import struct
    from di_fusion_amd import _lib, synthetic as syn
    from di_fusion_amd.system import ext
    from di_fusion_amd.system.map import DenseIndexedMap
    intr = syn.Intrinsic().scaled(0.5)
    scene, cfg = syn.config_c2()
    R, t = syn.orbit_pose(0)
    depth, ncam = syn.render_frame(scene, R, t, intr, DEV)
    _, _, nw, fd, fn = ext.depth_frontend(depth, intr.fx, intr.fy, intr.cx, intr.cy, filter=False, want_frame=True)
    ok = ~torch.isnan(fd)
    assert ok.float().mean() > 0.9
    dots = (fn[ok] * ncam[ok]).sum(-1)
    assert dots.abs().median() > 0.99 and (dots > 0).float().mean() > 0.98           # same surface normal, oriented like the renderer's
    m = DenseIndexedMap(gpu_model, cfg.namespace(), 29, DEV)
    H, W = intr.height, intr.width
    xyz = torch.empty((H * W, 3), device=DEV); nrm = torch.empty((H * W, 3), device=DEV); mask = torch.empty((H * W,), dtype=torch.uint8, device=DEV)
    frame = torch.from_numpy(np.frombuffer(struct.pack("<QQ12f", fd.data_ptr(), fn.data_ptr(), *[float(np.float32(v)) for v in R.reshape(-1)],
                                                       *[float(np.float32(v)) for v in t]), dtype=np.uint8).copy()).to(DEV)
    lib = _lib.load()
    ws = torch.empty((int(lib.dif_integrate_workspace_bytes(H * W)),), dtype=torch.uint8, device=DEV)
    m._ensure_capacity(7 * (H * W // 17))
    w = gpu_model.packed.weights_struct(DEV)
    _lib.check(lib.dif_integrate_frame(ctypes.byref(m._cmap), ctypes.byref(w), _lib.ptr(frame), H, W, intr.fx, intr.fy, intr.cx, intr.cy, _lib.ptr(xyz),
                                       _lib.ptr(nrm), _lib.ptr(mask), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), "dif_integrate_frame")
    # the same points through the ordinary entry point
    m2 = DenseIndexedMap(gpu_model, cfg.namespace(), 29, DEV)
    keep = ~torch.isnan(xyz[:, 0])
    mask2 = m2.integrate_keyframe(xyz[keep].contiguous(), nrm[keep].contiguous())
    n = m.n_occupied
    assert n == m2.n_occupied and n > 500
    assert torch.equal(m.latent_vecs[:n], m2.latent_vecs[:n]) and torch.equal(m.voxel_obs_count[:n], m2.voxel_obs_count[:n])
    assert torch.equal(mask[keep].bool(), mask2)
    assert m.extract_mesh_arrays(4, int(4e6), max_std=0.15, to_host=False)[0].size(0) > 1000
