"""CPU: the tracker's photometric term without a GPU — the numpy restatement (tests/photo_ref.py) against the fixtures the reference's own
`SDFTracker` produced (tests/golden/make_golden_photo.py), against torch's resizing on the CPU, and the additions to the C ABI.

What the fixtures pin and what they do not: the reference's CUDA image kernels cannot run where the fixtures are made, so its `rgb_odometry` /
`gradient_xy` were bound to the restatement; `_make_image_pyramid`, `compute_rgb_Hg` (mask, sign flip, robust weights, weight / M, the unscaled
K) and `gauss_newton` are the reference's own code.  The Python half of the term is pinned on the reference; the CUDA half only by reading
its 75 lines against the restatement."""
import json

import numpy as np
import pytest
import torch

from di_fusion_amd import synthetic as syn
from tests import photo_ref as P
from tests.conftest import GOLDEN, ROOT

INTR = [syn.Intrinsic().fx, syn.Intrinsic().fy, syn.Intrinsic().cx, syn.Intrinsic().cy]
NEW_SYMBOLS = ["dif_gradient_xy", "dif_photo_pyramid", "dif_rgb_odometry", "dif_rgb_hg_workspace_bytes", "dif_rgb_hg"]


def fixture_frames(g, noise, device="cpu"):
    """(rgb, depth) of the fixture's previous and current frame (frames 1 and 2 of the C2 orbit), checked against its hashes."""
    scene, _ = syn.config_c2()
    cut = tuple(float(x) for x in g["depth_cut"]) if "depth_cut" in g.files else (0.5, 5.0)
    frames = []
    for tag, f in (("prev", 1), ("cur", 2)):
        R, t = syn.orbit_pose(f)
        rgb, depth = syn.render_rgbd(scene, R, t, syn.Intrinsic(), depth_cut=cut, noise_seed=(1234 + f) if noise else None)
        assert P.sha(rgb.numpy()) == str(g[f"{tag}_rgb_sha"]) and P.sha(depth.numpy()) == str(g[f"{tag}_depth_sha"])
        frames.append((rgb.to(device), depth.to(device)))
    return frames


def restated_pyramids(g, noise):
    """The restatement's pyramids of both frames; the nine arrays of each against the hashes of the reference's (torch, CPU)."""
    pyrs = []
    for tag, (rgb, depth) in zip(("prev", "cur"), fixture_frames(g, noise)):
        pyr = P.pyramid(P.intensity_of(rgb.numpy()), depth.numpy())
        for l in range(3):
            for name, lst in zip("IDG", pyr):
                assert P.sha(lst[l]) == str(g[f"{tag}_{name}{l}_sha"]), f"{tag} {name}{l}"
        pyrs.append(pyr)
    return pyrs


def kernel_of(g, c):
    k = str(g[f"{c}_kernel"])
    return None if k == "None" else k


def within(x, x_ref, d_ref, S, slack, what):
    """|x - x_ref| <= d_ref + slack * S, entry by entry, in absolute terms (S: the sum of the absolute values of the entry's terms)."""
    err = np.abs(np.asarray(x) - np.asarray(x_ref))
    bar = np.asarray(d_ref) + slack * np.asarray(S)
    bad = np.nonzero(err > bar)[0]
    assert bad.size == 0, f"{what}: entries {bad[:6].tolist()} off by {err[bad][:6]} (bar {bar[bad][:6]})"


@pytest.mark.parametrize("name", ["photo_c2", "photo_c2_cut"])
def test_restatement_vs_the_references_term(name):
    g = np.load(GOLDEN / f"{name}.npz")
    prev, cur = restated_pyramids(g, noise=True)
    rgb_args = json.loads(str(g["rgb_args"]))
    flat = {}
    for n in range(int(g["n_cases"])):
        c = f"case{n}"
        level = int(g[f"{c}_level"])
        key = (level, str(g[f"{c}_pose"]))
        if key not in flat:
            krkinv, kt = P.warp_of(INTR, g[f"{c}_R"], g[f"{c}_t"])
            assert np.array_equal(krkinv, g[f"{c}_krkinv"]) and np.array_equal(kt, g[f"{c}_kt"])
            flat = {key: P.rgb_odometry(prev[0][level], prev[1][level], cur[0][level], cur[1][level], cur[2][level], INTR, krkinv, kt,
                                        rgb_args["min_grad_scale"], rgb_args["max_depth_delta"], True)}
        f, J = flat[key]
        out, S, mask = P.sums_of_flat(f, J, rgb_args["weight"], kernel_of(g, c), float(g[f"{c}_k"]))
        assert int(out[43]) == int(g[f"{c}_M"]) and P.sha(mask) == str(g[f"{c}_mask_sha"])
        assert np.allclose(S, g[f"{c}_S"], rtol=1e-9, atol=0.0)
        within(out[:43], g[f"{c}_x"], g[f"{c}_d_ref"], g[f"{c}_S"], 1e-12, f"{name} {c}")
        e_only, _, _ = P.sums_of_flat(f, None, rgb_args["weight"], kernel_of(g, c), float(g[f"{c}_k"]))
        assert e_only[42] == out[42] and not e_only[:42].any()


def test_restatement_vs_the_references_loop():
    """photo_track_c2: every evaluation of the photometric term the reference's `gauss_newton` made over the shipped iter_config."""
    g = np.load(GOLDEN / "photo_track_c2.npz")
    prev, cur = restated_pyramids(g, noise=False)
    assert json.loads(str(g["iter_config"])) == P.SHIPPED_ITERS and json.loads(str(g["rgb_args"])) == P.SHIPPED_RGB
    n_rgb = 0
    for j in range(int(g["gn_n_calls"])):
        term = str(g[f"gn{j}_term"])
        if term == "sdf":
            continue
        n_rgb += 1
        no_grad = bool(g[f"gn{j}_no_grad"])
        out, S, mask = P.compute_rgb_hg(prev, cur, int(term), INTR, g[f"gn{j}_delta_R"], g[f"gn{j}_delta_t"], P.SHIPPED_RGB, no_grad)
        assert int(out[43]) == int(g[f"gn{j}_M"]) and P.sha(mask) == str(g[f"gn{j}_mask_sha"])
        x_ref = np.concatenate([np.zeros(42) if no_grad else np.concatenate([g[f"gn{j}_H"].reshape(36), g[f"gn{j}_g"]]), [float(g[f"gn{j}_e"])]])
        within(out[:43], x_ref, g[f"gn{j}_d_ref"], g[f"gn{j}_S"], 1e-12, f"evaluation {j}")
    assert n_rgb >= 10


def test_pyramid_restatement_vs_torch_on_the_cpu():
    """`torch.mean` and `torch.nn.functional.interpolate` (bilinear, align_corners=False; nearest) on the CPU: bitwise at 640 x 480 (every
    scale is exactly 2, both weights exactly 0.5, rows of columns); at 481 x 641 within 3 x 2^-24 for inputs in [0, 1] (each order commits at
    most three roundings of at most 2^-25 of a partial sum <= 1).  The nearest resize is an index choice: equal at both sizes."""
    rng = np.random.default_rng(3)
    for (H, W), bitwise in (((480, 640), True), ((481, 641), False)):
        rgb = torch.from_numpy(rng.random((H, W, 3), dtype=np.float32))
        depth = torch.from_numpy((0.5 + 4.5 * rng.random((H, W), dtype=np.float32)))
        depth[rng.random((H, W)) < 0.1] = float("nan")
        I0 = torch.mean(rgb, dim=-1)
        assert np.array_equal(P.intensity_of(rgb.numpy()), I0.numpy())
        ti, td = I0[None, None], depth[None, None]
        for l in (1, 2):
            h, w = ti.shape[2] // 2, ti.shape[3] // 2
            mine_i, mine_d = P.resize_bilinear(ti[0, 0].numpy(), h, w), P.resize_nearest(td[0, 0].numpy(), h, w)      # (each level from torch's level above)
            ti = torch.nn.functional.interpolate(ti, (h, w), mode="bilinear")
            td = torch.nn.functional.interpolate(td, (h, w), mode="nearest")
            assert mine_i.shape == (h, w) and mine_i.dtype == np.float32
            assert np.array_equal(mine_d, td[0, 0].numpy(), equal_nan=True)
            if bitwise:
                assert np.array_equal(mine_i, ti[0, 0].numpy()), f"level {l} at {H} x {W}"
            else:
                assert np.abs(mine_i - ti[0, 0].numpy()).max() <= 3 * 2.0 ** -24, f"level {l} at {H} x {W}"
        Is, Ds, Gs = P.pyramid(I0.numpy(), depth.numpy())
        assert [i.shape for i in Is] == [(H, W), (H // 2, W // 2), (H // 2 // 2, W // 2 // 2)] and Gs[2].shape == Is[2].shape + (2,)
        if bitwise:
            assert np.array_equal(Is[2], ti[0, 0].numpy()) and np.array_equal(Ds[2], td[0, 0].numpy(), equal_nan=True)


def test_sobel_of_an_affine_image():
    a, b, c = 0.25, -0.5, 3.0                       # (exactly representable: the stencil is exact)
    u, v = np.meshgrid(np.arange(37, dtype=np.float32), np.arange(23, dtype=np.float32))
    G = P.gradient_xy(np.float32(a) * u + np.float32(b) * v + np.float32(c))
    assert G.shape == (23, 37, 2) and G.dtype == np.float32
    assert np.all(G[1:-1, 1:-1, 0] == np.float32(a)) and np.all(G[1:-1, 1:-1, 1] == np.float32(b))
    border = np.ones((23, 37), dtype=bool)
    border[1:-1, 1:-1] = False
    assert np.isnan(G[border]).all() and not np.isnan(G[~border]).any()


def test_rounding_of_the_warp_target():
    """Half to even, NaN -> 0, saturation: CUDA's __float2int_rn, which the kernel writes out."""
    q = np.array([0.5, 1.5, 2.5, -0.5, -1.5, np.nan, np.inf, -np.inf, 3e9, -3e9, 7.49], dtype=np.float32)
    assert P._rn(q).tolist() == [0, 2, 2, 0, -2, 0, 2147483647, -2147483648, 2147483647, -2147483648, 7]


def test_the_abi_additions_exist():
    """The five new entry points are declared, bound and exported, `dif_version()` is unchanged, and the two kernels of the term are in the code
    object without scratch memory.  Fails without the feature; needs no GPU."""
    import ctypes
    from di_fusion_amd import _build, _lib
    from tests.test_abi import _kernel_isa, header_symbols
    lib_path = _build.build()
    syms = header_symbols()
    h = ctypes.CDLL(str(lib_path))
    for s in NEW_SYMBOLS:
        assert s in syms, f"{s} not declared in difusion.h"
        assert s in _lib.SIGNATURES, f"{s} not bound in _lib.SIGNATURES"
        assert hasattr(h, s), f"{s} not exported"
    assert h.dif_version() == 100
    h.dif_rgb_hg_workspace_bytes.restype = ctypes.c_int64
    assert h.dif_rgb_hg_workspace_bytes() > 0 and h.dif_rgb_hg_workspace_bytes() % 256 == 0
    assert ctypes.sizeof(_lib.DifRgbHg) == 22 * 4 and ctypes.sizeof(_lib.DifPhotoPyramid) == 9 * 8
    hdr = (ROOT / "include" / "difusion.h").read_text()
    assert "float krkinv[9]" in hdr and "float kt[3]" in hdr and "float intr[4]" in hdr
    isa = _kernel_isa(["k_rgb_hg", "k_rgb_odometry", "k_photo_level", "k_gradient_xy"])
    for k, text in isa.items():
        assert "scratch_" not in text, f"{k} uses scratch memory"
    hg = isa["k_rgb_hg"]
    # the hand-back of k_sdf_hg_reduce: write-through stores, sc1 loads, no cache write-back / invalidate
    import re
    assert re.search(r"global_store_dwordx2 .* sc1", hg) and re.search(r"global_load_dwordx2 .* sc1", hg) and re.search(r"global_store_dwordx2 .* sc0 sc1", hg)
    assert "buffer_wbl2" not in hg and "buffer_inv" not in hg


def test_host_side_of_rgb_hg_matches_the_fixture():
    """`tracker.photo_warp` (K, K R K^-1, K t in float64) for `Pose`s, 4x4 matrices and Isometry-like objects against what the reference's
    `compute_rgb_Hg` handed to its kernel; `level_scale` scales the four intrinsics."""
    from types import SimpleNamespace
    from di_fusion_amd.system.tracker import Pose, photo_warp
    g = np.load(GOLDEN / "photo_c2.npz")
    calib = SimpleNamespace(fx=INTR[0], fy=INTR[1], cx=INTR[2], cy=INTR[3])
    for n in range(0, int(g["n_cases"]), 3):
        p = Pose(g[f"case{n}_R"], g[f"case{n}_t"])
        iso = SimpleNamespace(q=SimpleNamespace(rotation_matrix=p.R.copy()), t=p.t.copy())
        for pose in (p, p.matrix, iso):
            intr, krkinv, kt = photo_warp(calib, pose)
            assert intr == INTR
            assert np.abs(np.array(krkinv) - g[f"case{n}_krkinv"]).max() < 1e-12 and np.abs(np.array(kt) - g[f"case{n}_kt"]).max() < 1e-12
        intr, krkinv, kt = photo_warp(calib, p, 0.25)
        assert intr == [x * 0.25 for x in INTR]
        k2, t2 = P.warp_of(intr, p.R, p.t)
        assert np.abs(np.array(krkinv) - k2).max() < 1e-12 and np.abs(np.array(kt) - t2).max() < 1e-12


def test_texture_and_render_rgbd():
    """Two views of a surface point see one colour; colours are in [0, 1] and finite whatever the depth cut; `render_frame` is the depth."""
    scene, _ = syn.config_c2()
    intr = syn.Intrinsic().scaled(0.25)
    (R1, t1), (R2, t2) = syn.orbit_pose(1), syn.orbit_pose(9)
    rgb1, d1 = syn.render_rgbd(scene, R1, t1, intr, depth_cut=(0.5, 3.0), noise_seed=7)
    assert rgb1.shape == (120, 160, 3) and rgb1.dtype == torch.float32 and float(rgb1.min()) >= 0.0 and float(rgb1.max()) <= 1.0
    assert not torch.isnan(rgb1).any() and torch.isnan(d1).any()
    d_ref, _ = syn.render_frame(scene, R1, t1, intr, depth_cut=(0.5, 3.0), noise_seed=7)
    assert torch.equal(torch.nan_to_num(d1), torch.nan_to_num(d_ref))
    # a world point and its colour, seen from the second camera: project and compare with the rendered pixel's neighbourhood
    rgb_e, d_e = syn.render_rgbd(scene, R1, t1, intr, depth_cut=(0.0, float("inf")))
    rgb2, d2 = syn.render_rgbd(scene, R2, t2, intr, depth_cut=(0.0, float("inf")))
    pc = syn.unproject_reference_order(d_e, intr).double().reshape(-1, 3)
    pw = pc @ torch.tensor(R1).T + torch.tensor(t1)
    assert torch.equal(syn.texture(pw).reshape(120, 160, 3)[::7, ::7], syn.texture(pw.reshape(120, 160, 3)[::7, ::7]))
    assert (syn.texture(pw).reshape(120, 160, 3) - rgb_e).abs().max() < 1e-5          # (float32 back-projection against the float64 hit point)
    p2 = (pw - torch.tensor(t2)) @ torch.tensor(R2)
    u = torch.round(p2[:, 0] / p2[:, 2] * intr.fx + intr.cx).long()
    v = torch.round(p2[:, 1] / p2[:, 2] * intr.fy + intr.cy).long()
    ok = (u >= 0) & (u < 160) & (v >= 0) & (v < 120)
    same = ok.clone()
    same[ok] = (d2[v[ok], u[ok]].double() - p2[ok, 2]).abs() < 0.02         # the same surface, not an occluder
    assert same.sum() > 10000
    a, b = rgb2[v[same], u[same]], rgb_e.reshape(-1, 3)[same]
    diff, control = (a - b).abs().mean(), (a - b.roll(4001, 0)).abs().mean()
    # the projection lands up to half a pixel from the pixel's own ray: ~1.25 cm at 3 m and a quarter of the resolution, times the texture's
    # typical slope of ~2 / m; an unrelated pairing differs by the texture's own spread
    print(f"  texture seen twice: mean difference {float(diff):.4f}, unrelated pixels {float(control):.4f}")
    assert diff < 0.03 and control > 5 * diff
