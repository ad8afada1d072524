"""GPU parity of the DenseIndexedMap path against (i) the golden vectors captured from the imported reference and
(ii) the oracle stepped on the same inputs.  Integer state (mask, indexer, slot order, counts, dirty set, MC voxel
lists) must be BIT-EXACT; latents / SDF / vertices within the stated tolerances."""
import numpy as np
import pytest
import torch

from di_fusion_amd import synthetic as syn
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

LATENT_TOL = 2e-5        # |z_gpu - z_ref| : fp32 sums of ~10^3 encoder outputs in a different order
# Cube values away from the 0.05 refinement threshold, end to end: the latents differ from the reference's by ~1e-6 (another summation
# order, another matrix pipe) and the decoder amplifies that by up to ~25x at a few samples (tests/test_oracle_golden.py: the oracle's
# own worst sample is 1.56e-5 from the reference with its own latents and 4.6e-6 with the reference's).  With the REFERENCE's latents
# loaded into the map the decode meets BASELINE.md's 1e-5 (test_decode_of_reference_latents_within_1e5).
SDF_TOL = 3e-5
SDF_TOL_REF_LATENTS = 1e-5

CASES = {
    "seq_small": (syn.Scene(kind="sphere", radius=1.3), syn.MapConfig((-1.6,) * 3, (1.6,) * 3, 0.4), syn.Intrinsic().scaled(0.125)),
    "seq_room16": (syn.default_room(), syn.MapConfig((-3.2,) * 3, (3.2,) * 3, 0.4), syn.Intrinsic().scaled(0.25)),
    # BASELINE configs C2 (64^3) and C3 (128^3) at their real size: two full 640x480 frames of the bench stream each
    "seq_c2": (*syn.config_c2(), syn.Intrinsic()),
    "seq_c3": (*syn.config_c3(), syn.Intrinsic()),
}


def frame_inputs(g, name, f):
    scene, cfg, intr = CASES[name]
    if f"f{f}_xyz" in g:
        return g[f"f{f}_xyz"], g[f"f{f}_nrm"]
    xyz, nrm = syn.frame_points(scene, f, intr, deg_per_frame=float(g["deg_per_frame"]))
    return xyz.numpy(), nrm.numpy()


def make_map(gpu_model, cfg):
    from di_fusion_amd.system.map import DenseIndexedMap
    return DenseIndexedMap(gpu_model, cfg.namespace(), 29, DEV, initial_capacity=1024)


def check_state(m, g, f, om=None):
    n = m.n_occupied
    assert n == int(g[f"f{f}_int_n_occupied"])
    idx = m.indexer.cpu().numpy()
    nz = np.nonzero(idx != -1)[0]
    assert np.array_equal(nz, g[f"f{f}_int_indexer_nz"])
    assert np.array_equal(idx[nz], g[f"f{f}_int_indexer_val"])
    assert np.array_equal(m.latent_vecs_pos[:n].cpu().numpy(), g[f"f{f}_int_latent_vecs_pos"])
    assert np.array_equal(m.voxel_obs_count[:n].cpu().numpy(), g[f"f{f}_int_voxel_obs_count"])
    assert m.latent_vecs.size(0) == int(g[f"f{f}_int_capacity"])
    assert np.array_equal(m.updated_vec_id.cpu().numpy(), g[f"f{f}_int_updated_vec_id"])
    d = np.abs(m.latent_vecs[:n].cpu().numpy() - g[f"f{f}_int_latent_vecs"]).max()
    print(f"  frame {f}: n_occupied={n} latent maxdiff vs reference {d:.3e} counters={m.last_counters}")
    assert d < LATENT_TOL
    if om is not None:
        assert np.abs(m.latent_vecs[:n].cpu().numpy() - om.latent_vecs[:n]).max() < LATENT_TOL


def check_state_oracle(m, om):
    """check_state against the oracle alone (weights the goldens were not recorded with): integer state bit for bit, latents within LATENT_TOL"""
    n = m.n_occupied
    assert n == om.n_occupied
    assert np.array_equal(m.indexer.cpu().numpy(), om.indexer)
    assert np.array_equal(m.latent_vecs_pos[:n].cpu().numpy(), om.latent_vecs_pos[:n])
    assert np.array_equal(m.voxel_obs_count[:n].cpu().numpy(), om.voxel_obs_count[:n])
    assert np.array_equal(m.updated_vec_id.cpu().numpy(), om.updated_vec_id)
    d = np.abs(m.latent_vecs[:n].cpu().numpy() - om.latent_vecs[:n]).max()
    print(f"  n_occupied={n} latent maxdiff vs oracle {d:.3e} counters={m.last_counters}")
    assert d < LATENT_TOL


def sort_tris(tri, tid):
    """canonical, permutation-invariant order: (voxel id, quantised centroid)"""
    c = np.round(tri.mean(axis=1) * 4096).astype(np.int64)
    return np.lexsort((c[:, 2], c[:, 1], c[:, 0], tid))


@pytest.mark.parametrize("name", ["seq_small", "seq_room16", "seq_c2", "seq_c3"])
def test_sequence_vs_golden_and_oracle(name, gpu_model, oracle_net):
    run_sequence(name, gpu_model, oracle_net, golden=True)


def run_sequence(name, gpu_model, oracle_net, golden):
    """The fixture's frames through the GPU map and through the oracle stepped on the same inputs.  golden: also against the vectors
    recorded from the reference (they belong to the shipped weights; tests/test_gpu_mlp_envelope.py runs other weight sets without)."""
    from oracle import difusion_oracle as O
    scene, cfg, intr = CASES[name]
    g = np.load(GOLDEN / f"{name}.npz")
    m = make_map(gpu_model, cfg)
    om = O.OracleMap(oracle_net, cfg.bound_min, cfg.bound_max, cfg.voxel_size)
    for f in range(int(g["n_frames"])):
        xyz, nrm = frame_inputs(g, name, f)
        mask = m.integrate_keyframe(torch.from_numpy(xyz).to(DEV), torch.from_numpy(nrm).to(DEV))
        omask = om.integrate_keyframe(xyz, nrm)
        assert np.array_equal(mask.cpu().numpy(), omask)
        if golden:
            assert np.array_equal(np.packbits(mask.cpu().numpy()), g[f"f{f}_unq_mask"])
            check_state(m, g, f, om)
        else:
            check_state_oracle(m, om)
        assert m.last_counters["M"] == om.last_stats["M"] and m.last_counters["C"] == om.last_stats["C"]

        # ---- extract: GPU pipeline, then the oracle on ITS state -------------------------------------------
        verts, vid, vstd = m.extract_mesh_arrays(4, int(4e6), max_std=0.15, no_cache=False)
        new_T = m.last_counters["T"]
        tens = m._xbuf[1]
        K, B = m.last_counters["K"], m.last_counters["B"]
        oa = om.extract_prepare(4)
        if golden:
            assert np.array_equal(tens["valid_blocks"][:K].cpu().numpy(), g[f"f{f}_mc_valid_blocks"])
            assert B == int(g[f"f{f}_mc_B"])
        else:
            assert np.array_equal(tens["valid_blocks"][:K].cpu().numpy(), oa["valid_blocks"]) and B == len(oa["occupied_vec_id"])
        assert np.array_equal(tens["occ_slot"][:B].cpu().numpy(), oa["occupied_vec_id"])
        cs = tens["cube_sdf"][:B].cpu().numpy(); cd = tens["cube_std"][:B].cpu().numpy()
        sel = g[f"f{f}_mc_cube_sel"] if f"f{f}_mc_cube_sel" in g else np.arange(B)
        # samples whose interpolated |sdf| sits within 1e-5 of the 0.05 threshold may legitimately flip between
        # "interpolated" and "re-decoded" (SURVEY.md section 7): excluded, and counted
        flip = np.zeros_like(cs, dtype=bool).reshape(B, -1)
        if len(oa["near_threshold"]):
            flip[oa["near_threshold"][:, 0], oa["near_threshold"][:, 1]] = True
        flip = flip.reshape(cs.shape)
        ds = np.abs(cs - oa["cube_sdf"]); dd = np.abs(cd - oa["cube_std"])
        print(f"  frame {f}: K={K} B={B} VH={m.last_counters['VH']} (oracle {oa['n_rows_refine']}) cube maxdiff sdf {ds[~flip].max():.2e} "
              f"std {dd[~flip].max():.2e} near-threshold {flip.sum()}")
        assert ds[~flip].max() < SDF_TOL and dd[~flip].max() < SDF_TOL
        if golden:
            assert np.abs(cs[sel] - g[f"f{f}_mc_cube_sdf"])[~flip[sel]].max() < SDF_TOL
        assert abs(m.last_counters["VH"] - oa["n_rows_refine"]) <= flip.sum()
        # marching cubes on the GPU's own cubes through the C oracle: isolates the MC kernel
        wt, wi, ws = O.marching_cubes_interp(oa["indexer"], oa["valid_blocks"], oa["vec_batch_mapping"], cs, cd, int(4e6), om.n_xyz, 0.15)
        assert new_T == wt.shape[0]
        ntri, nid, nstd = m.mesh_cache_tensors(new_only=True)
        assert ntri.size(0) == new_T
        gt = ntri.cpu().numpy()
        want = (wt * np.float32(cfg.voxel_size)).astype(np.float32) + om.bound_min
        assert np.array_equal(nid.cpu().numpy(), wi)
        if golden or new_T:                 # (a foreign decoder need not put a zero crossing into this scene: no triangles, nothing to compare)
            assert np.abs(gt - want).max() < 1e-5
            assert np.abs(nstd.cpu().numpy() - ws).max() < 1e-5
        assert new_T > 0 or not golden
    # ---- get_sdf ---------------------------------------------------------------------------------------------
    sdf, std, qmask = m.get_sdf(torch.from_numpy(g["probe_xyz"]).to(DEV))
    if golden:
        assert np.array_equal(qmask.cpu().numpy(), g["probe_mask"])
        assert np.abs(sdf.cpu().numpy() - g["probe_sdf"]).max() < SDF_TOL
        assert np.abs(std.cpu().numpy() - g["probe_std"]).max() < SDF_TOL
    else:
        osdf, ostd, omask = om.get_sdf(g["probe_xyz"])
        assert np.array_equal(qmask.cpu().numpy(), omask)
        assert np.abs(sdf.cpu().numpy() - osdf).max() < SDF_TOL and np.abs(std.cpu().numpy() - ostd).max() < SDF_TOL


@pytest.mark.parametrize("pipe", ["bf16x6", "f32"])
@pytest.mark.parametrize("name", ["seq_small", "seq_room16", "seq_c2", "seq_c3"])
def test_decode_of_reference_latents_within_1e5(name, pipe, gpu_model, gpu_model_f32):
    """BASELINE.md section 4's tolerance made honest: every frame's map state is checked against the reference run, then the map's
    latents are REPLACED by the reference's before the extract, so the decoded cubes isolate the decode path (lattice, folded MLP tiles on
    either matrix pipe, ATen-exact trilinear x2, threshold + refine): <= 1e-5 on SDF and std against the reference's cubes at every
    fixture size up to C3, near-threshold samples excluded as everywhere."""
    from oracle import difusion_oracle as O
    scene, cfg, intr = CASES[name]
    g = np.load(GOLDEN / f"{name}.npz")
    m = make_map(gpu_model if pipe == "bf16x6" else gpu_model_f32, cfg)
    worst = 0.0
    for f in range(int(g["n_frames"])):
        xyz, nrm = frame_inputs(g, name, f)
        m.integrate_keyframe(torch.from_numpy(xyz).to(DEV), torch.from_numpy(nrm).to(DEV))
        check_state(m, g, f)
        n = int(g[f"f{f}_int_n_occupied"])
        m._latent[:n] = torch.from_numpy(g[f"f{f}_int_latent_vecs"]).to(DEV)
        m.extract_mesh_arrays(4, int(4e6), max_std=0.15, to_host=False)
        B = m.last_counters["B"]
        assert B == int(g[f"f{f}_mc_B"])
        tens = m._xbuf[1]
        cs = tens["cube_sdf"][:B].cpu().numpy(); cd = tens["cube_std"][:B].cpu().numpy()
        sel = g[f"f{f}_mc_cube_sel"] if f"f{f}_mc_cube_sel" in g else np.arange(B)
        # near-threshold samples from the reference's own interpolated values: |  |low-lattice interpolation| - 0.05 | < 1e-5 cannot be told
        # from the cubes alone, so a sample counts as a flip when it differs by more than the bar AND its reference value is a re-decoded or
        # interpolated value within 2e-3 of the threshold band edge ... (counted, bounded)
        ds = np.abs(cs[sel] - g[f"f{f}_mc_cube_sdf"]); dd = np.abs(cd[sel] - g[f"f{f}_mc_cube_std"])
        bad = (ds >= SDF_TOL_REF_LATENTS) | (dd >= SDF_TOL_REF_LATENTS)
        near = np.abs(np.abs(g[f"f{f}_mc_cube_sdf"]) - 0.05) < 5e-3
        print(f"  {name} {pipe} frame {f}: B={B} sdf max {ds[~bad].max():.2e} std max {dd[~bad].max():.2e} over-the-bar samples {int(bad.sum())} "
              f"(all near the 0.05 threshold: {bool((near | ~bad).all())})")
        assert bad.sum() <= 8 and (near | ~bad).all()          # only refinement flips at the threshold may exceed the bar
        worst = max(worst, float(ds[~bad].max()), float(dd[~bad].max()))
    assert worst < SDF_TOL_REF_LATENTS


def test_mesh_cache_replace_by_voxel(gpu_model, oracle_net):
    """map.py:703-714: triangles of voxels that produced new triangles are replaced, the rest of the cache is kept
    (including the reference's quirk that a re-meshed voxel which now yields NO triangle keeps its stale ones).
    Expected cache = the reference's host-side rule applied to the C oracle's marching cubes of the GPU's OWN cubes (so a
    refinement-threshold flip in the decode cannot blur the comparison): same length, same voxel id at every position, same order
    (kept old triangles, then the new ones), vertices within 1e-5."""
    from oracle import difusion_oracle as O
    scene, cfg, intr = CASES["seq_small"]
    g = np.load(GOLDEN / "seq_small.npz")
    m = make_map(gpu_model, cfg)
    om = O.OracleMap(oracle_net, cfg.bound_min, cfg.bound_max, cfg.voxel_size)
    cache = None
    replaced = 0
    for f in range(3):
        xyz, nrm = frame_inputs(g, "seq_small", f)
        m.integrate_keyframe(torch.from_numpy(xyz).to(DEV), torch.from_numpy(nrm).to(DEV))
        om.integrate_keyframe(xyz, nrm)
        v, vid, vs = m.extract_mesh_arrays(4, int(4e6), max_std=0.15)
        B = m.last_counters["B"]
        oa = om.extract_prepare(4)
        assert np.array_equal(m._xbuf[1]["valid_blocks"][:m.last_counters["K"]].cpu().numpy(), oa["valid_blocks"])
        cs, cd = m._xbuf[1]["cube_sdf"][:B].cpu().numpy(), m._xbuf[1]["cube_std"][:B].cpu().numpy()
        wt, oid, ostd = O.marching_cubes_interp(oa["indexer"], oa["valid_blocks"], oa["vec_batch_mapping"], cs, cd, int(4e6), om.n_xyz, 0.15)
        ov = (wt * np.float32(cfg.voxel_size)).astype(np.float32) + om.bound_min                  # map.py:698
        before = 0 if cache is None else cache[0].shape[0]
        cache = O.mesh_cache_update(cache, ov, oid, ostd)         # the reference's host-side rule (pinned on its own code: mesh_cache.npz)
        replaced += before + ov.shape[0] - cache[0].shape[0]
        assert v.shape[0] == vid.shape[0] == vs.shape[0] == cache[0].shape[0], (f, v.shape, cache[0].shape)
        assert np.array_equal(vid, cache[1])
        assert np.abs(v - cache[0]).max() < 1e-5 and np.abs(vs - cache[2]).max() < 1e-5
    assert replaced > 0 and len(np.unique(vid)) > 10
    mesh = m.extract_mesh(4, int(4e6), max_std=0.15)
    assert mesh is not None and mesh.triangles.shape[0] == v.shape[0]


def test_mesh_cache_vs_reference(gpu_model):
    """The mesh cache after each of four frames against the REFERENCE's own post-marching-cubes code (map.py:698-714; tests/golden/mesh_cache.npz, where
    the CUDA marching cubes is played by the C oracle on the reference's cubes): the same triangles in the same order — voxel id at every position
    of the cache —, the new triangles' ids per frame, the final vertices and stds within what the cubes' 1e-5 allows."""
    g = np.load(GOLDEN / "mesh_cache.npz")
    scene, cfg, intr = CASES["seq_room16"]
    m = make_map(gpu_model, cfg)
    for f in range(int(g["n_frames"])):
        xyz, nrm = syn.frame_points(scene, f, intr, deg_per_frame=float(g["deg_per_frame"]))
        m.integrate_keyframe(xyz.to(DEV), nrm.to(DEV))
        v, vid, vs = m.extract_mesh_arrays(4, int(4e6), max_std=0.15)
        ntri, nid, nstd = m.mesh_cache_tensors(new_only=True)
        assert np.array_equal(nid.cpu().numpy(), g[f"f{f}_new_id"]), f
        assert np.array_equal(vid, g[f"f{f}_cache_id"]), f
        want = (g[f"f{f}_new_tri_voxel_units"] * np.float32(cfg.voxel_size)).astype(np.float32) + np.asarray(cfg.bound_min, dtype=np.float32)
        d = np.abs(ntri.cpu().numpy() - want).max()
        print(f"  frame {f}: {nid.shape[0]} new triangles, cache {vid.shape[0]}, new vertices within {d:.2e} m of the reference's")
        assert d < 2e-4
    assert np.abs(v - g["final_vertices"]).max() < 2e-4 and np.abs(vs - g["final_std"]).max() < 2e-4


def test_edge_cases(gpu_model):
    scene, cfg, intr = CASES["seq_small"]
    m = make_map(gpu_model, cfg)
    # nothing to mesh yet
    assert m.extract_mesh_arrays(4, 1000) is None
    # out-of-bounds and NaN points are ignored; too few points per voxel are pruned
    pts = torch.tensor([[100.0, 0, 0], [float("nan"), 0, 0], [0.1, 0.1, 0.1]], device=DEV)
    nrm = torch.tensor([[0.0, 0, 1]] * 3, device=DEV)
    mask = m.integrate_keyframe(pts, nrm)
    assert mask.sum().item() == 0 and m.n_occupied == 0
    # empty query
    sdf, std, qm = m.get_sdf(torch.zeros((0, 3), device=DEV))
    assert sdf.numel() == 0 and qm.numel() == 0
    # wrong device
    with pytest.raises(AssertionError):
        m.integrate_keyframe(torch.zeros((4, 3)), torch.zeros((4, 3)))


def test_scattered_points_without_pruning_vs_oracle(gpu_model, oracle_net):
    """Points in random order, pruning off: consecutive points share no voxel, a 256-point workgroup touches ~2,000 distinct voxels
    (more than its LDS row-count table holds: the overflow path), every voxel gets only a handful of rows.  State must still be
    bit-exact against the oracle."""
    from oracle import difusion_oracle as O
    cfg = syn.MapConfig((-1.6, -1.6, -1.6), (1.6, 1.6, 1.6), 0.1, prune_min_vox_obs=0)
    g = torch.Generator().manual_seed(7)
    xyz = ((torch.rand((6000, 3), generator=g) - 0.5) * 3.0).float()
    nrm = torch.nn.functional.normalize(torch.randn((6000, 3), generator=g), dim=1).float()
    m = make_map(gpu_model, cfg)
    om = O.OracleMap(oracle_net, cfg.bound_min, cfg.bound_max, cfg.voxel_size, prune_min_vox_obs=0)
    for rep in range(2):                                   # second pass: voxels already allocated, running average
        mask = m.integrate_keyframe(xyz.to(DEV), nrm.to(DEV))
        omask = om.integrate_keyframe(xyz.numpy(), nrm.numpy())
        assert mask is None or np.array_equal(mask.cpu().numpy(), omask)
        n = m.n_occupied
        assert n == om.n_occupied and n > 5000
        assert np.array_equal(m.indexer.cpu().numpy().reshape(-1), om.indexer.reshape(-1))
        assert np.array_equal(m.voxel_obs_count[:n].cpu().numpy(), om.voxel_obs_count[:n])
        assert np.abs(m.latent_vecs[:n].cpu().numpy() - om.latent_vecs[:n]).max() < 2e-5
        assert m.last_counters["M"] == om.last_stats["M"]


def test_capacity_growth_and_save_load(gpu_model, tmp_path):
    scene, cfg, intr = CASES["seq_room16"]
    g = np.load(GOLDEN / "seq_room16.npz")
    m = make_map(gpu_model, cfg)                       # initial capacity 1024 is enough; force growth through a tiny one
    m._alloc_state(1024)
    for f in range(2):
        xyz, nrm = frame_inputs(g, "seq_room16", f)
        m.integrate_keyframe(torch.from_numpy(xyz).to(DEV), torch.from_numpy(nrm).to(DEV))
        check_state(m, g, f)
        if f == 0:
            m.extract_mesh_arrays(4, int(4e6), max_std=0.15)      # the golden sequence meshes (and clears the dirty set) every frame
            m._alloc_state(m._capacity * 2)                         # grow mid-sequence: state must survive the re-allocation
    m.save(tmp_path / "map.pt")
    m2 = make_map(gpu_model, cfg)
    m2.load(tmp_path / "map.pt")
    n = m.n_occupied
    assert m2.n_occupied == n
    assert torch.equal(m2.indexer, m.indexer)
    assert torch.equal(m2.latent_vecs[:n], m.latent_vecs[:n])
    sdf1, _, _ = m.get_sdf(torch.from_numpy(g["probe_xyz"]).to(DEV))
    sdf2, _, _ = m2.get_sdf(torch.from_numpy(g["probe_xyz"]).to(DEV))
    assert torch.equal(sdf1, sdf2)


def test_loads_a_map_saved_by_the_reference(gpu_model, tmp_path):
    """tests/golden/ref_map_small.pt was written by the reference's own `DenseIndexedMap.save` (map.py:239-243) after the three
    seq_small frames; `load` must reproduce the golden state of frame 2, answer `get_sdf` like the reference, and a re-save
    must open again with the same content (wire format of SURVEY.md 8f-4)."""
    scene, cfg, intr = CASES["seq_small"]
    g = np.load(GOLDEN / "seq_small.npz")
    m = make_map(gpu_model, cfg)
    m.load(GOLDEN / "ref_map_small.pt")
    n = int(g["f2_int_n_occupied"])
    assert m.n_occupied == n
    idx = m.indexer.cpu().numpy().reshape(-1)
    nz = np.nonzero(idx != -1)[0]
    assert np.array_equal(nz, g["f2_int_indexer_nz"]) and np.array_equal(idx[nz], g["f2_int_indexer_val"])
    assert np.array_equal(m.latent_vecs_pos[:n].cpu().numpy(), g["f2_int_latent_vecs_pos"])
    assert np.array_equal(m.voxel_obs_count[:n].cpu().numpy(), g["f2_int_voxel_obs_count"])
    assert np.array_equal(m.latent_vecs[:n].cpu().numpy(), g["f2_int_latent_vecs"])       # the reference's own floats, bit for bit
    sdf, std, qmask = m.get_sdf(torch.from_numpy(g["probe_xyz"]).to(DEV))
    assert np.array_equal(qmask.cpu().numpy(), g["probe_mask"])
    assert np.abs(sdf.cpu().numpy() - g["probe_sdf"]).max() < SDF_TOL
    # a loaded map has no dirty voxels of its own: a full (no_cache) extraction meshes everything it holds
    verts, vid, vstd = m.extract_mesh_arrays(4, int(4e6), max_std=0.15, no_cache=True)
    assert verts.shape[0] > 0
    m.save(tmp_path / "again.pt")
    cv = torch.load(tmp_path / "again.pt", map_location="cpu")
    ref = torch.load(GOLDEN / "ref_map_small.pt", map_location="cpu")
    assert int(cv["n_occupied"]) == int(ref["n_occupied"])
    assert torch.equal(cv["indexer"].view(-1), ref["indexer"].view(-1))
    for k in ("latent_vecs", "latent_vecs_pos", "voxel_obs_count"):
        assert torch.equal(cv[k][:n], ref[k][:n]), k
    assert set(ref.keys()) <= set(cv.keys())


def test_determinism(gpu_model):
    """Same inputs twice -> bit-identical latents and triangles (the reference's float atomics cannot promise this)."""
    scene, cfg, intr = CASES["seq_small"]
    g = np.load(GOLDEN / "seq_small.npz")
    outs = []
    for rep in range(2):
        m = make_map(gpu_model, cfg)
        for f in range(2):
            xyz, nrm = frame_inputs(g, "seq_small", f)
            m.integrate_keyframe(torch.from_numpy(xyz).to(DEV), torch.from_numpy(nrm).to(DEV))
        v, vid, vs = m.extract_mesh_arrays(4, int(4e6), max_std=0.15)
        outs.append((m.latent_vecs.clone(), v.copy(), vid.copy()))
    assert torch.equal(outs[0][0], outs[1][0])
    assert np.array_equal(outs[0][1], outs[1][1]) and np.array_equal(outs[0][2], outs[1][2])


def test_c1_full_frame_vs_golden(gpu_model):
    """BASELINE.json configs[0]: one full 640x480 frame, 32^3 grid — the bit-exact voxel-id/allocation check."""
    scene, cfg = syn.config_c1()
    g = np.load(GOLDEN / "seq_c1.npz")
    xyz, nrm = syn.frame_points(scene, 0, syn.Intrinsic())
    m = make_map(gpu_model, cfg)
    mask = m.integrate_keyframe(xyz.to(DEV), nrm.to(DEV))
    assert np.array_equal(np.packbits(mask.cpu().numpy()), g["f0_unq_mask"])
    check_state(m, g, 0)
    m.extract_mesh_arrays(4, int(4e6), max_std=0.15)
    K, B = m.last_counters["K"], m.last_counters["B"]
    tens = m._xbuf[1]
    assert np.array_equal(tens["valid_blocks"][:K].cpu().numpy(), g["f0_mc_valid_blocks"])
    assert B == int(g["f0_mc_B"])
    sel = g["f0_mc_cube_sel"]
    d = np.abs(tens["cube_sdf"][:B].cpu().numpy()[sel] - g["f0_mc_cube_sdf"])
    print(f"  C1: cube sdf diff max {d.max():.2e}, >{SDF_TOL}: {(d > SDF_TOL).sum()} of {d.size}, T={m.last_counters['T']}")
    assert (d > SDF_TOL).mean() < 1e-4          # threshold flips only
    sdf, std, qmask = m.get_sdf(torch.from_numpy(g["probe_xyz"]).to(DEV))
    assert np.array_equal(qmask.cpu().numpy(), g["probe_mask"])
    assert np.abs(sdf.cpu().numpy() - g["probe_sdf"]).max() < SDF_TOL


def test_get_sdf_gradient_matches_autograd_and_finite_differences(gpu_model, raw_weights):
    """a17 / SURVEY 8f-1: d sdf / d xyz from the reverse MFMA chain vs (i) torch autograd through a plain fp32 torch
    re-statement of the decoder on the same latents, (ii) central finite differences of the kernel's own sdf."""
    from di_fusion_amd.network import packing
    scene, cfg, intr = CASES["seq_small"]
    g = np.load(GOLDEN / "seq_small.npz")
    m = make_map(gpu_model, cfg)
    for f in range(2):
        xyz, nrm = frame_inputs(g, "seq_small", f)
        m.integrate_keyframe(torch.from_numpy(xyz).to(DEV), torch.from_numpy(nrm).to(DEV))
    q = torch.from_numpy(g["probe_xyz"]).to(DEV).requires_grad_(True)
    sdf, std, mask = m.get_sdf(q)
    loss = sdf / std.detach()                                    # the tracker's residual (tracker.py:186)
    (gq,) = torch.autograd.grad(loss, [q], grad_outputs=torch.ones_like(loss))
    assert gq.shape == q.shape and mask.sum().item() == sdf.numel() > 100
    assert torch.all(gq[~mask] == 0)
    # (i) torch reference on CPU
    Ws, bs, Wu, bu = packing.fold_decoder(raw_weights)
    Ws = [torch.from_numpy(w) for w in Ws]; bs = [torch.from_numpy(b) for b in bs]
    qc = q.detach().cpu().double().requires_grad_(True)
    bmin = torch.tensor(cfg.bound_min, dtype=torch.float64)
    xn = (qc - bmin) / cfg.voxel_size
    gid = torch.ceil(xn.detach()) - 1
    lin = (gid[:, 2] + m.n_xyz[2] * gid[:, 1] + m.n_xyz[2] * m.n_xyz[1] * gid[:, 0]).long()
    slot = m.indexer.cpu()[lin]
    mk = mask.cpu()
    lat = m.latent_vecs.cpu()[slot[mk]].double()
    rel = xn[mk] - gid[mk] - 0.5
    x0 = torch.cat([lat, rel], 1)
    h = x0
    for l in range(4):
        if l == 3:
            h = torch.cat([h, x0], 1)
        h = torch.relu(h @ Ws[l].double().T + bs[l].double())
    ref_sdf = torch.tanh(h @ Ws[4].double().T + bs[4].double())[:, 0]
    ref_loss = ref_sdf / std.detach().cpu().double()
    (gref,) = torch.autograd.grad(ref_loss, [qc], grad_outputs=torch.ones_like(ref_loss))
    assert np.abs(sdf.detach().cpu().numpy() - ref_sdf.detach().numpy()).max() < SDF_TOL
    d = (gq.cpu().double() - gref).abs().max().item()
    scale = gref.abs().max().item()
    print(f"  get_sdf grad: max |diff| {d:.3e} (max |grad| {scale:.3e})")
    assert d < 1e-4 * max(scale, 1.0)
    # (ii) finite differences along x on the kernel itself (skip points close to a ReLU kink / voxel face)
    eps = 1e-3
    qp = q.detach().clone(); qp[:, 0] += eps
    qm = q.detach().clone(); qm[:, 0] -= eps
    sp, _, mp = m.get_sdf(qp)
    sm, _, mm = m.get_sdf(qm)
    both = (mask & mp & mm)
    idx = torch.cumsum(mask.long(), 0) - 1
    fd = (sp[(torch.cumsum(mp.long(), 0) - 1)[both]] - sm[(torch.cumsum(mm.long(), 0) - 1)[both]]) / (2 * eps)
    an = (gq[:, 0] * std.detach()[idx.clamp(min=0)])[both]        # undo the 1/std factor
    rel_err = ((fd - an).abs() / (an.abs() + 0.05)).median().item()
    assert rel_err < 0.05, rel_err


@pytest.mark.parametrize("pipe", ["bf16x6", "f32"])
@pytest.mark.parametrize("name", ["seq_small", "seq_c2"])
def test_get_sdf_gradient_vs_reference_autograd(name, pipe, gpu_model, gpu_model_f32):
    """SURVEY 8f-1 pinned on the reference itself: `probe_grad` is what the reference's tracker differentiates
    (`get_sdf(xyz.requires_grad_())`, residual sdf / std.detach(), `autograd.grad`; tracker.py:184-192, map.py:559-579), recorded on CPU by
    tests/golden/make_golden.py on the map the golden frames build.  The analytic gradient of the reverse MFMA chain, on both matrix
    pipes, must agree to 1e-4 of the gradient scale."""
    scene, cfg, intr = CASES[name]
    g = np.load(GOLDEN / f"{name}.npz")
    m = make_map(gpu_model if pipe == "bf16x6" else gpu_model_f32, cfg)
    for f in range(int(g["n_frames"])):
        xyz, nrm = frame_inputs(g, name, f)
        m.integrate_keyframe(torch.from_numpy(xyz).to(DEV), torch.from_numpy(nrm).to(DEV))
        m.extract_mesh_arrays(4, int(4e6), max_std=0.15, to_host=False)
    q = torch.from_numpy(g["probe_xyz"]).to(DEV).requires_grad_(True)
    sdf, std, mask = m.get_sdf(q)
    res = sdf / std.detach()
    (gq,) = torch.autograd.grad(res, [q], grad_outputs=torch.ones_like(res))
    assert np.array_equal(mask.cpu().numpy(), g["probe_mask"])
    got, want = gq[mask].cpu().numpy(), g["probe_grad"]
    assert got.shape == want.shape and want.shape[0] > 400
    scale = np.abs(want).max()
    d = np.abs(got - want)
    # a probe within rounding of a ReLU kink may take the other branch on another arithmetic: counted, must stay rare
    bad = (d > 1e-4 * scale).any(axis=1)
    print(f"  {name}/{pipe}: grad vs reference autograd: max |diff| {d[~bad].max():.3e} of scale {scale:.3e} ({int(bad.sum())} of {len(bad)} probes on a kink)")
    assert bad.sum() <= 2
    assert torch.all(gq[~mask] == 0)
    # the explicit entry point hands out the same Jacobian without torch's autograd engine
    s2, d2, m2, g2 = m.get_sdf_with_gradient(q.detach())
    assert torch.equal(m2, mask) and torch.equal(s2, sdf.detach()) and torch.equal(d2, std)
    assert torch.allclose(g2 / d2.unsqueeze(1), gq[mask], rtol=1e-6, atol=1e-6 * scale)


@pytest.mark.parametrize("resolution,fast,mc_grid", [(4, False, 0), (2, True, 0), (8, True, 0), (3, True, 0), (2, True, 3), (3, True, 5), (4, True, 2)])
def test_other_resolutions_and_exact_decode(resolution, fast, mc_grid, gpu_model, oracle_net, mc_grid_cap):
    """extract_mesh(voxel_resolution, fast) away from the shipped default (4, True): same pipeline, checked against the oracle.
    mc_grid > 0: the one-pass marching cubes capped at that many workgroups (dif_test_mc_grid_cap), i.e. in ticket mode with parked groups."""
    from oracle import difusion_oracle as O
    if mc_grid:
        mc_grid_cap(mc_grid)
    scene, cfg, intr = CASES["seq_small"]
    g = np.load(GOLDEN / "seq_small.npz")
    m = make_map(gpu_model, cfg)
    om = O.OracleMap(oracle_net, cfg.bound_min, cfg.bound_max, cfg.voxel_size)
    xyz, nrm = frame_inputs(g, "seq_small", 0)
    m.integrate_keyframe(torch.from_numpy(xyz).to(DEV), torch.from_numpy(nrm).to(DEV))
    om.integrate_keyframe(xyz, nrm)
    m.extract_mesh_arrays(resolution, int(4e6), fast=fast, max_std=0.15)
    oa = om.extract_prepare(resolution, fast=fast)
    B = m.last_counters["B"]
    tens = m._xbuf[1]
    cs = tens["cube_sdf"][:B].cpu().numpy(); cd = tens["cube_std"][:B].cpu().numpy()
    assert cs.shape == oa["cube_sdf"].shape
    flip = np.zeros(cs.shape, dtype=bool).reshape(B, -1)
    if len(oa["near_threshold"]):
        flip[oa["near_threshold"][:, 0], oa["near_threshold"][:, 1]] = True
    flip = flip.reshape(cs.shape)
    assert np.abs(cs - oa["cube_sdf"])[~flip].max() < SDF_TOL
    assert np.abs(cd - oa["cube_std"])[~flip].max() < SDF_TOL
    wt, wi, ws = O.marching_cubes_interp(oa["indexer"], oa["valid_blocks"], oa["vec_batch_mapping"], cs, cd, int(4e6), om.n_xyz, 0.15)
    ntri, nid, nstd = m.mesh_cache_tensors(new_only=True)
    assert ntri.size(0) == wt.shape[0] > 0
    want = (wt * np.float32(cfg.voxel_size)).astype(np.float32) + om.bound_min
    assert np.array_equal(nid.cpu().numpy(), wi)
    assert np.abs(ntri.cpu().numpy() - want).max() < 1e-5


def _variant_cubes(m, g, key, tol, oa):
    K, B = m.last_counters["K"], m.last_counters["B"]
    tens = m._xbuf[1]
    assert np.array_equal(tens["valid_blocks"][:K].cpu().numpy(), g[f"{key}_valid_blocks"])
    assert B == int(g[f"{key}_B"])
    sel = torch.from_numpy(g[f"{key}_cube_sel"]).to(DEV)
    cs, cd = tens["cube_sdf"][:B][sel].cpu().numpy(), tens["cube_std"][:B][sel].cpu().numpy()
    want_s, want_d = g[f"{key}_cube_sdf"], g[f"{key}_cube_std"]
    assert cs.shape == want_s.shape
    # samples whose interpolated |sdf| sits within 1e-5 of the 0.05 refinement threshold may be refined on one side only: excluded, as everywhere
    # (the oracle, stepped on the same inputs, says which)
    thr = np.zeros((B, want_s[0].size), dtype=bool)
    if len(oa["near_threshold"]):
        thr[oa["near_threshold"][:, 0], oa["near_threshold"][:, 1]] = True
    thr = thr.reshape((B,) + want_s.shape[1:])[g[f"{key}_cube_sel"]]
    assert thr.mean() < 2e-3
    d = max(np.abs(cs - want_s)[~thr].max(), np.abs(cd - want_d)[~thr].max())
    assert d < tol, (key, d)
    return d


def test_extract_variants_vs_reference(gpu_model, oracle_net):
    """`extract_mesh` away from the tracking loop's call, against the REFERENCE (tests/golden/extract_variants.npz): two integrates before ONE extract,
    fast=False, resolutions 2 / 3 / 8, no_cache=True — dirty list, B and the cubes handed to marching cubes."""
    from oracle import difusion_oracle as O
    g = np.load(GOLDEN / "extract_variants.npz")
    scene, cfg, intr = CASES["seq_room16"]
    m = make_map(gpu_model, cfg)
    om = O.OracleMap(oracle_net, cfg.bound_min, cfg.bound_max, cfg.voxel_size)
    for f in range(int(g["n_frames"])):
        xyz, nrm = syn.frame_points(scene, f, intr, deg_per_frame=float(g["deg_per_frame"]))
        m.integrate_keyframe(xyz.to(DEV), nrm.to(DEV))
        om.integrate_keyframe(xyz.numpy(), nrm.numpy())
    n = m.n_occupied
    assert n == int(g["int_n_occupied"])
    assert np.array_equal(m.latent_vecs_pos[:n].cpu().numpy(), g["int_latent_vecs_pos"])
    assert np.array_equal(m.voxel_obs_count[:n].cpu().numpy(), g["int_voxel_obs_count"])
    assert np.abs(m.latent_vecs[:n].cpu().numpy() - g["int_latent_vecs"]).max() < 5e-6
    for name in g["names"]:
        r, fast, nc = int(g[f"{name}_resolution"]), bool(g[f"{name}_fast"]), bool(g[f"{name}_no_cache"])
        out = m.extract_mesh_arrays(r, int(4e6), fast=fast, max_std=0.15, no_cache=nc)
        d = _variant_cubes(m, g, name, SDF_TOL, om.extract_prepare(r, fast=fast, no_cache=nc))
        print(f"  {name}: K={m.last_counters['K']} B={m.last_counters['B']} triangles {out[0].shape[0]} maxdiff {d:.2e}")
        assert out[0].shape[0] > 1000


def test_integrate_without_pruning_vs_reference(gpu_model, oracle_net):
    """`prune_min_vox_obs = 0` (reference map.py:372-378): no mask comes back, every point's voxel is allocated; state and cubes against the reference."""
    from di_fusion_amd.system.map import DenseIndexedMap
    from oracle import difusion_oracle as O
    g = np.load(GOLDEN / "extract_variants.npz")
    scene, cfg, intr = CASES["seq_room16"]
    args = cfg.namespace()
    args.prune_min_vox_obs = 0
    m = DenseIndexedMap(gpu_model, args, 29, DEV, initial_capacity=1024)
    om = O.OracleMap(oracle_net, cfg.bound_min, cfg.bound_max, cfg.voxel_size, prune_min_vox_obs=0)
    for f in range(int(g["n_frames"])):
        xyz, nrm = syn.frame_points(scene, f, intr, deg_per_frame=float(g["deg_per_frame"]))
        assert m.integrate_keyframe(xyz.to(DEV), nrm.to(DEV)) is None
        om.integrate_keyframe(xyz.numpy(), nrm.numpy())
        n = m.n_occupied
        assert n == int(g[f"noprune_f{f}_n_occupied"])
        idx = m.indexer.cpu().numpy()
        nz = np.nonzero(idx != -1)[0]
        assert np.array_equal(nz, g[f"noprune_f{f}_indexer_nz"]) and np.array_equal(idx[nz], g[f"noprune_f{f}_indexer_val"])
        assert np.array_equal(m.latent_vecs_pos[:n].cpu().numpy(), g[f"noprune_f{f}_latent_vecs_pos"])
        assert np.array_equal(m.voxel_obs_count[:n].cpu().numpy(), g[f"noprune_f{f}_voxel_obs_count"])
        assert np.abs(m.latent_vecs[:n].cpu().numpy() - g[f"noprune_f{f}_latent_vecs"]).max() < 5e-6
    m.extract_mesh_arrays(4, int(4e6), max_std=0.15)
    _variant_cubes(m, g, "noprune", SDF_TOL, om.extract_prepare())


def test_sdf_gauss_newton_pose_refinement(gpu_model):
    """The caller of the path: `SDFTracker.compute_sdf_Hg` (reference tracker.py:174-218) restated on top of `map.get_sdf` —
    residual sdf/std.detach(), Jacobian from autograd through the map, 6-DoF Gauss-Newton.  A perturbed camera pose must be
    pulled back towards the truth: this is what 'drops into the existing tracking loop' means for row a17."""
    scene = syn.default_room()                                   # boxes + walls constrain all 6 DoF (a sphere would not)
    cfg = syn.MapConfig((-3.2,) * 3, (3.2,) * 3, 0.2)
    intr = syn.Intrinsic().scaled(0.5)
    m = make_map(gpu_model, cfg)
    for f in range(3):
        xyz, nrm = syn.frame_points(scene, f, intr, deg_per_frame=4.0)
        m.integrate_keyframe(xyz.to(DEV), nrm.to(DEV))
    # observation: frame 1 in CAMERA coordinates
    R, t = syn.orbit_pose(1, deg_per_frame=4.0)
    depth, _ = syn.render_frame(scene, R, t, intr)
    pc = syn.unproject_reference_order(depth, intr).reshape(-1, 3)
    pc = pc[~torch.isnan(pc[:, 0])][::11].to(DEV).double()
    Rt = torch.tensor(R, device=DEV); tt = torch.tensor(t, device=DEV)

    def hat(w):
        z = torch.zeros((), dtype=torch.float64, device=DEV)
        return torch.stack([torch.stack([z, -w[2], w[1]]), torch.stack([w[2], z, -w[0]]), torch.stack([-w[1], w[0], z])])

    def residual_and_jac(Rc, tc):
        xyz = (pc @ Rc.T + tc).float().requires_grad_(True)
        sdf, std, mask = m.get_sdf(xyz)
        r = sdf / std.detach()
        (g,) = torch.autograd.grad(r, [xyz], grad_outputs=torch.ones_like(r))
        g = g[mask].double()                                      # d r / d xyz_world   (M,3)
        p = xyz.detach()[mask].double()
        J = torch.cat([g, torch.cross(p, g, dim=1)], dim=1)       # left perturbation: [translation | rotation]
        return r.detach().double(), J

    # perturb: 1.5 degrees about y, 2 cm translation
    a = np.deg2rad(1.5)
    dR = torch.tensor([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], device=DEV)
    Rc, tc = dR @ Rt, tt + torch.tensor([0.02, -0.01, 0.015], device=DEV)
    e0 = (residual_and_jac(Rc, tc)[0] ** 2).mean().item()
    err0 = (torch.linalg.norm(tc - tt).item(), np.rad2deg(np.arccos(np.clip((torch.trace(Rc @ Rt.T).item() - 1) / 2, -1, 1))))
    for it in range(8):
        r, J = residual_and_jac(Rc, tc)
        H = J.T @ J + 1e-6 * torch.eye(6, dtype=torch.float64, device=DEV)
        xi = -torch.linalg.solve(H, J.T @ r)
        W = hat(xi[3:])
        dRot = torch.linalg.matrix_exp(W)
        Rc, tc = dRot @ Rc, dRot @ tc + xi[:3]
    e1 = (residual_and_jac(Rc, tc)[0] ** 2).mean().item()
    err1 = (torch.linalg.norm(tc - tt).item(), np.rad2deg(np.arccos(np.clip((torch.trace(Rc @ Rt.T).item() - 1) / 2, -1, 1))))
    print(f"  GN on map.get_sdf: residual {e0:.4f} -> {e1:.4f}; pose error {err0[0]*100:.2f} cm / {err0[1]:.2f} deg -> {err1[0]*100:.2f} cm / {err1[1]:.2f} deg")
    assert e1 < 0.5 * e0
    assert err1[0] < 0.5 * err0[0] and err1[1] < 0.5 * err0[1]


def test_mesh_cache_log_garbage_collection(gpu_model):
    """The cache is an append-only log; compaction (on host access) and garbage collection must not change its content/order."""
    scene, cfg, intr = CASES["seq_small"]
    g = np.load(GOLDEN / "seq_small.npz")
    m = make_map(gpu_model, cfg)
    for f in range(3):
        xyz, nrm = frame_inputs(g, "seq_small", f)
        m.integrate_keyframe(torch.from_numpy(xyz).to(DEV), torch.from_numpy(nrm).to(DEV))
        v, vid, vs = m.extract_mesh_arrays(4, int(4e6), max_std=0.15)
    assert m.last_counters["cache_dead"] > 0                      # frames 1, 2 replaced earlier batches
    before = (v.copy(), vid.copy(), vs.copy())
    m._cache_gc()
    assert m.last_counters["cache_dead"] == 0 and m.last_counters["cache_T"] == before[0].shape[0]
    mc = m.mesh_cache
    mc.invalidate_host_copy()
    assert np.array_equal(mc.vertices, before[0]) and np.array_equal(mc.vertices_flatten_id, before[1]) and np.array_equal(mc.vertices_std, before[2])
    # a further frame after the GC still replaces the right batches: compare with a map that never collected
    m2 = make_map(gpu_model, cfg)
    for f in range(3):
        xyz, nrm = frame_inputs(g, "seq_small", f)
        m2.integrate_keyframe(torch.from_numpy(xyz).to(DEV), torch.from_numpy(nrm).to(DEV))
        m2.extract_mesh_arrays(4, int(4e6), max_std=0.15)
    xyz, nrm = frame_inputs(g, "seq_small", 0)
    for mm in (m, m2):
        mm.integrate_keyframe(torch.from_numpy(xyz).to(DEV), torch.from_numpy(nrm).to(DEV))
    a = m.extract_mesh_arrays(4, int(4e6), max_std=0.15)
    b = m2.extract_mesh_arrays(4, int(4e6), max_std=0.15)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_mesh_cache_log_grows_with_a_small_per_call_limit(gpu_model):
    """A caller that passes a small `max_n_triangles` per call on a map whose mesh keeps growing: the reference's host cache simply grows
    (map.py:703-714).  The device log starts at max(3 * limit, 65536) entries and must be compacted / doubled on the way, never
    overflow, and hold — entry for entry, in the same order — what the same sequence yields with a log that never needs to grow."""
    scene, cfg = syn.config_c2()
    intr = syn.Intrinsic().scaled(0.5)
    small, big = make_map(gpu_model, cfg), make_map(gpu_model, cfg)
    limit = 80000                       # above any single call's output here, far below the whole mesh
    caps = set()
    for f in range(12):
        xyz, nrm = syn.frame_points(scene, f, intr, deg_per_frame=30.0)
        xyz, nrm = xyz.to(DEV), nrm.to(DEV)
        outs = []
        for m, lim in ((small, limit), (big, int(4e6))):
            m.integrate_keyframe(xyz, nrm)
            outs.append(m.extract_mesh_arrays(4, lim, max_std=0.15, to_host=False))
        assert small.last_counters["T"] <= limit, "this test wants untruncated calls"
        caps.add(small._cache[0].size(0))
        for x, y in zip(outs[0], outs[1]):
            assert torch.equal(x, y), f
    assert outs[0][0].size(0) > 3 * limit and len(caps) > 1, (outs[0][0].shape, caps)  # the log had to grow beyond its first size
    assert small._gc_epoch > 0 and big._gc_epoch == 0


def test_extract_async_is_ordered_behind_the_integrates(gpu_model):
    """`extract_mesh(extract_async=True)` (reference map.py:716-720) on the meshing thread / stream while the main thread goes on
    integrating: the extract must see exactly the state of the integrates enqueued before it.  Compared with the same schedule run
    synchronously, over several rounds."""
    scene, cfg, intr = CASES["seq_room16"]
    frames = [tuple(t.to(DEV) for t in syn.frame_points(scene, f, intr, deg_per_frame=15.0)) for f in range(6)]

    def run(async_):
        m = make_map(gpu_model, cfg)
        meshes = []
        for f in range(0, 6, 2):
            m.integrate_keyframe(*frames[f])
            if async_:
                assert m.extract_mesh(4, int(4e6), max_std=0.15, extract_async=True) is None
                m.integrate_keyframe(*frames[f + 1])              # races with the meshing thread unless the streams are ordered
                mesh = m.extract_mesh(4, int(4e6), max_std=0.15, extract_async=False)       # joins the thread, returns its mesh
                assert m.meshing_thread is None or not m.meshing_thread.is_alive()
                m.meshing_thread = None
            else:
                mesh = m.extract_mesh(4, int(4e6), max_std=0.15)
                m.integrate_keyframe(*frames[f + 1])
            meshes.append(np.asarray(mesh.vertices).copy())
        torch.cuda.synchronize()
        n = m.n_occupied
        return meshes, m.latent_vecs[:n].clone(), m.voxel_obs_count[:n].clone()

    a, za, wa = run(False)
    b, zb, wb = run(True)
    assert torch.equal(za, zb) and torch.equal(wa, wb)
    for x, y in zip(a, b):
        assert x.shape == y.shape and x.shape[0] > 0 and np.array_equal(x, y)


def test_allocate_block(gpu_model):
    """reference map.py:310-319 as an external entry point: new ids get slots in ascending order, ids that are already allocated keep
    their slot and their latent bits."""
    scene, cfg, intr = CASES["seq_small"]
    g = np.load(GOLDEN / "seq_small.npz")
    m = make_map(gpu_model, cfg)
    xyz, nrm = frame_inputs(g, "seq_small", 0)
    m.integrate_keyframe(torch.from_numpy(xyz).to(DEV), torch.from_numpy(nrm).to(DEV))
    n0 = m.n_occupied
    z0, w0, idx0 = m.latent_vecs[:n0].clone(), m.voxel_obs_count[:n0].clone(), m.indexer.clone()
    free = torch.nonzero(idx0 == -1).flatten()[:5]
    taken = torch.nonzero(idx0 != -1).flatten()[:5]
    ids = torch.sort(torch.cat([free, taken]))[0]
    m.allocate_block(ids)
    assert m.n_occupied == n0 + 5
    assert torch.equal(m.indexer[free].cpu(), torch.arange(n0, n0 + 5))
    assert torch.equal(m.latent_vecs_pos[n0:n0 + 5].cpu(), free.cpu())
    assert torch.equal(m.indexer[taken], idx0[taken])
    assert torch.equal(m.latent_vecs[:n0], z0) and torch.equal(m.voxel_obs_count[:n0], w0)      # bit for bit
    assert float(m.voxel_obs_count[n0:n0 + 5].abs().sum()) == 0.0
    # any order, duplicates included (the reference accepts whatever its caller passes, map.py:310-319): slots still go out in ascending id
    more = torch.nonzero(m.indexer == -1).flatten()[:4]
    m.allocate_block(torch.cat([torch.flip(more, [0]), more[:2], taken]))
    assert m.n_occupied == n0 + 9
    assert torch.equal(m.indexer[more].cpu(), torch.arange(n0 + 5, n0 + 9))
    assert torch.equal(m.latent_vecs[:n0], z0) and torch.equal(m.voxel_obs_count[:n0], w0)
    m.allocate_block(torch.zeros((0,), dtype=torch.long))
    assert m.n_occupied == n0 + 9


@pytest.mark.parametrize("pipe", ["bf16x6", "f32"])
def test_latent_optimisation_vs_reference_and_oracle(pipe, gpu_model, gpu_model_f32, oracle_net):
    """8f-4, `integrate_keyframe(do_optimize=True)` (map.py:459-513, :80-113, :321-335), on both matrix pipes (`k_optim_grad<true>`: the
    optimiser's forward + reverse chain as six-slice bf16 products, `<false>`: f32-input MFMA): which voxels are optimised, how many samples are
    gathered for them, the dirty set and the observation counts must equal the reference's run bit for bit; the optimised latents agree
    to what five Adam steps in fp32 allow — the same algorithm evaluated in float64 instead of float32 moves them by up to 2e-4 (mean
    6e-6), the reference's own fp32 result sits 3e-4 (mean 9e-6) from the float64 one (Adam's g / sqrt(v) amplifies rounding where a
    gradient component is near zero) — so: max 1e-3, mean 5e-5, and the likelihood loss must fall."""
    from oracle import difusion_oracle as O
    g = np.load(GOLDEN / "seq_optim.npz")
    scene, cfg, intr = CASES["seq_small"]
    args = cfg.namespace()
    args.optim_n_iters, args.code_regularization, args.code_reg_lambda = int(g["optim_n_iters"]), True, float(g["code_reg_lambda"])
    from di_fusion_amd.system.map import DenseIndexedMap
    m = DenseIndexedMap(gpu_model if pipe == "bf16x6" else gpu_model_f32, args, 29, DEV, initial_capacity=1024)
    om = O.OracleMap(oracle_net, cfg.bound_min, cfg.bound_max, cfg.voxel_size)
    om.optim_n_iters, om.code_regularization, om.code_reg_lambda = args.optim_n_iters, True, args.code_reg_lambda
    for f in range(int(g["n_frames"])):
        xyz, nrm = syn.frame_points(scene, f, intr, deg_per_frame=float(g["deg_per_frame"]))
        m.optimize_noise = torch.from_numpy(g[f"f{f}_noise"])
        m.integrate_keyframe(xyz.to(DEV), nrm.to(DEV), do_optimize=True)
        om.integrate_keyframe(xyz.numpy(), nrm.numpy(), do_optimize=True, noise=g[f"f{f}_noise"])
        n = m.n_occupied
        assert m.last_counters["opt_rows"] == g[f"f{f}_noise"].shape[0] == om.last_stats["optim_rows"]
        assert m.last_counters["opt_voxels"] == om.last_stats["optim_voxels"]
        assert np.array_equal(m.voxel_optimized[:n].cpu().numpy(), g[f"f{f}_voxel_optimized"])
        assert np.array_equal(m.voxel_obs_count[:n].cpu().numpy(), g[f"f{f}_voxel_obs_count"])
        assert np.array_equal(m.updated_vec_id.cpu().numpy(), g[f"f{f}_updated_vec_id"])
        z = m.latent_vecs[:n].cpu().numpy()
        opt_now = g[f"f{f}_voxel_optimized"]
        d_ref, d_or = np.abs(z - g[f"f{f}_latent_vecs"]), np.abs(z - om.latent_vecs[:n])
        losses = m.optimize_losses.cpu().numpy()[:args.optim_n_iters]
        print(f"  frame {f}: {m.last_counters['opt_voxels']} voxels / {m.last_counters['opt_rows']} rows optimised; latent vs reference max {d_ref.max():.2e} "
              f"mean {d_ref[opt_now].mean():.2e}, vs oracle max {d_or.max():.2e}; likelihood loss {losses}")
        assert d_ref.max() < 1e-3 and d_ref[opt_now].mean() < 5e-5
        assert d_or.max() < 1e-3 and d_or[opt_now].mean() < 5e-5
        assert d_ref[~opt_now].max() < LATENT_TOL                               # voxels the optimiser did not touch: the ordinary fusion bar
        if m.last_counters["opt_rows"]:
            # the likelihood loss before EVERY Adam step against what the reference's own run evaluated (recorded from its
            # CombinedChunkLoss, tests/golden/make_golden.py), to 1e-3 relative; and the oracle's
            want = g[f"f{f}_loss_ll"]
            assert want.shape[0] == args.optim_n_iters
            rel = np.abs(losses - want) / np.abs(want)
            rel_or = np.abs(np.asarray(om.last_stats["optim_losses"])[:args.optim_n_iters] - want) / np.abs(want)
            print(f"           loss vs reference: rel {rel.max():.2e} (oracle {rel_or.max():.2e})")
            assert rel.max() < 1e-3 and rel_or.max() < 1e-3
        m.extract_mesh_arrays(4, int(4e6), max_std=0.15)                        # the golden sequence meshes (clears the dirty set) every frame
        om.extract_prepare(4)
    assert int(m.voxel_optimized.sum()) > 50
    # without do_optimize nothing changes for the optimiser's bookkeeping, and async is declined
    with pytest.raises(NotImplementedError):
        m.integrate_keyframe(xyz.to(DEV), nrm.to(DEV), do_optimize=True, async_optimize=True)


def test_dirty_set_block_totals_match_the_counting_pass(gpu_model):
    """`dif_map_t.dirty_tot` (per-block totals of the dirty flags, kept by k_fuse) against the two-pass scan that counts the flags itself:
    two integrates before an extract (a voxel updated twice is counted once), a capacity growth in between (recount on re-allocation),
    a record merge (recount by the wrapper) and a `no_cache` extract — same valid_blocks, same mesh."""
    import ctypes
    from di_fusion_amd.system.map import DenseIndexedMap
    scene, cfg = syn.config_c2()
    intr = syn.Intrinsic().scaled(0.5)
    frames = [tuple(t.to(DEV) for t in syn.frame_points(scene, f, intr, deg_per_frame=2.0)) for f in range(4)]

    def run(use_totals):
        m = DenseIndexedMap(gpu_model, cfg.namespace(), 29, DEV, initial_capacity=8192)
        outs = []

        def extract(**kw):
            if not use_totals:
                m._cmap.dirty_tot = None                    # dif_extract counts the flags itself
            v = m.extract_mesh_arrays(4, int(4e6), max_std=0.15, to_host=False, **kw)
            K = m.last_counters["K"]
            outs.append((m._xbuf[1]["valid_blocks"][:K].clone(), v[0].clone(), v[1].clone(), dict(m.last_counters)))

        def integrate(f):
            if not use_totals:
                m._cmap.dirty_tot = None
            m.integrate_keyframe(*frames[f])

        integrate(0); integrate(1); extract(no_cache=False)          # two integrates, one extract
        cap0 = m._capacity
        integrate(2); extract(no_cache=False)
        integrate(3)
        m._ensure_capacity(4 * cap0)                                 # grow between the integrate and its extract
        assert m._capacity > cap0
        extract(no_cache=False)
        other = DenseIndexedMap(gpu_model, cfg.namespace(), 29, DEV, initial_capacity=8192)
        other.integrate_keyframe(*frames[0])
        m.merge_records(other.export_records())                      # dirty flags set by the merge kernel
        extract(no_cache=False)
        extract(no_cache=True)                                       # every allocated voxel
        integrate(1); extract(no_cache=False)                        # and the totals are idle again afterwards
        return outs, m

    a, ma = run(True)
    b, mb = run(False)
    assert ma._cmap.dirty_tot and int(ma._dirty_tot.sum().item()) == 0
    for i, (x, y) in enumerate(zip(a, b)):
        assert x[3]["K"] == y[3]["K"] > 0 and x[3]["B"] == y[3]["B"] and x[3]["T"] == y[3]["T"], (i, x[3], y[3])
        assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) and torch.equal(x[2], y[2]), i


@pytest.mark.parametrize("withheld", [("mc_status",), ("chunk_sum", "mc_status")], ids=["count_emit", "count_scan_emit"])
def test_one_pass_marching_cubes_equals_count_and_emit_passes(withheld, gpu_model):
    """The stream path's single-launch marching cubes (count, decoupled look-back, emit) against the passes it replaces — without mc_status
    the count pass + emit pass over chunk_sum, without chunk_sum as well the count pass, the scan kernel and the emit pass:
    12.8 k dirty voxels (3,200 look-back groups over 512 resident workgroups, i.e. several groups per workgroup), then a second frame
    that replaces batches in the log — the same log, bit for bit, and the same bookkeeping."""
    from di_fusion_amd.system.map import DenseIndexedMap
    scene, cfg = syn.config_c3()
    intr = syn.Intrinsic()
    frames = [tuple(t.to(DEV) for t in syn.frame_points(scene, f, intr, deg_per_frame=0.5)) for f in range(2)]

    def run(one_pass):
        m = DenseIndexedMap(gpu_model, cfg.namespace(), 29, DEV, initial_capacity=32768)
        outs = []
        for f in range(2):
            m.integrate_keyframe(*frames[f])
            h = m.extract_mesh_enqueue(4, int(4e6), max_std=0.15)
            assert m._xbuf[1]["mc_status"].numel() > 0
            outs.append(h)
            m.extract_mesh_finish(h)
            t = m.mesh_cache_tensors()
            outs[-1] = (tuple(x.clone() for x in t), dict(m.last_counters), m._tri_start.clone(), m._tri_n.clone())
        return outs

    import di_fusion_amd.system.map as M
    a = run(True)
    orig = M.DenseIndexedMap._extract_buffers

    def without_optional(self, *args, **kw):
        t, b = orig(self, *args, **kw)
        for name in withheld:                                # dif_extract falls back to the count pass (+ scan kernel) + emit pass
            setattr(b, name, None)
        return t, b

    M.DenseIndexedMap._extract_buffers = without_optional
    try:
        b = run(False)
    finally:
        M.DenseIndexedMap._extract_buffers = orig
    for f, (x, y) in enumerate(zip(a, b)):
        assert x[1] == y[1] and x[1]["T"] > 100000 and x[1]["K"] > 10000, (f, x[1], y[1])
        for u, v in zip(x[0], y[0]):
            assert torch.equal(u, v), f
        assert torch.equal(x[2], y[2]) and torch.equal(x[3], y[3]), f
