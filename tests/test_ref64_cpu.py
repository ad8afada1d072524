"""Pins tests/ref64.py (the float64 statement of the networks) and the generators of tests/mlp_cases.py.  No GPU.

  * against tests/golden/networks.npz: the reference's own rows;
  * against OracleNetworks (float32) on every weight set and input class: the oracle's worst error is what float32 costs there;
  * the analytic input gradient against float64 torch.autograd on a plain torch restatement;
  * that every weight set reaches every branch of the epilogue (softplus below 20, above 20, where expf would overflow; tanh in its
    linear part and saturated) on at least 1 % of the rows of some case;
  * K of the GPU bar, re-measured (see mlp_cases.K_BAR), and K_NLL of the optimiser's gradient bar (optim_cases.K_NLL);
  * the optimiser's loss and gradient (Ref64.decoder_nll_grad) against float64 autograd of the loss written with
    torch.distributions.Normal(...).log_prob, the Adam step and the code regulariser against torch.optim.Adam in float64, and the NumPy
    restatement of the optimiser's gather (optim_cases.gather_rows) against OracleMap._optimize_stage;
  * the NumPy restatement of the integrate chain (integrate_cases.restate, fuse32) against OracleMap.integrate_keyframe on the cases of
    tests/test_gpu_integrate_envelope.py, and that those cases reach the paths they are there for.

`python tests/test_ref64_cpu.py` prints the table of profiles/mlp_envelope_k.md.
"""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from oracle import difusion_oracle as O  # noqa: E402
from tests import mlp_cases as C  # noqa: E402
from tests import optim_cases as OC  # noqa: E402
from tests.ref64 import Ref64  # noqa: E402

GOLDEN = Path(__file__).resolve().parent / "golden"
F32 = np.float32


def test_ref64_matches_reference_rows():
    """The reference's float32 outputs on its 384 golden rows: within float32's own error of the float64 values (the oracle is pinned
    on the same rows at 2e-6 / 5e-6 by test_oracle_golden)."""
    g = np.load(GOLDEN / "networks.npz")
    ref = Ref64(C.weight_set("shipped"))
    sdf, std, _, _ = ref.decoder(g["dec_x"])
    assert np.abs(sdf - g["dec_sdf"][:, 0]).max() < 2e-6 and np.abs(std - g["dec_std"][:, 0]).max() < 2e-6
    assert np.abs(ref.encoder(g["enc_x"]) - g["enc_out"]).max() < 5e-6


def test_ref64_lattice_and_upsample_match_reference():
    g = np.load(GOLDEN / "networks.npz")
    a, b = -(4 // 2) * (1. / 4), 1. + (4 - 1) // 2 * (1. / 4)
    assert np.array_equal(Ref64.samples(4, a, b).astype(F32), g["extract_low_l4"]) and np.array_equal(Ref64.samples(8, a, b).astype(F32), g["extract_high_R8"])
    up = Ref64.upsample(g["tri_low"][:, 0].astype(np.float64), 8)
    assert np.abs(up - g["tri_up"][:, 0]).max() < 4 * np.spacing(F32(np.abs(g["tri_up"]).max()))


@pytest.mark.parametrize("name", C.WEIGHT_SETS)
def test_weight_sets_are_what_they_claim(name):
    raw = C.weight_set(name)
    if name == "shipped":
        return
    for i in range(5):
        v, g = raw[f"decoder.lin{i}.weight_v"], raw[f"decoder.lin{i}.weight_g"]
        assert (np.abs(v).max(axis=1) > 0).all(), "weight norm divides by the row's norm"
        if i < 4:
            assert (g > 0).any() and (g < 0).any()
            nz = np.abs(v[v != 0])
            assert 0.05 < (v == 0).mean() < 0.15 and np.log2(nz.max() / np.median(nz)) > 4
    for i in range(3):
        p = f"encoder.mlp.layer{i}.normlayer.bn."
        assert (raw[p + "weight"] < 0).any() and (raw[p + "running_mean"] != 0).all()
        assert raw[p + "running_var"].min() < 1e-2 and raw[p + "running_var"].max() > 3
    if name == "bf16":
        ref = Ref64(raw)
        for W in ref.dec_W + [ref.unc_W, ref.enc_last_W]:
            assert C._is_bf16(W.astype(F32)).all()
        for W, gamma, _, _, var in ref.enc:
            assert C._is_bf16((W * (gamma / np.sqrt(var + 1e-5))[:, None]).astype(F32)).all()


@pytest.mark.parametrize("name", C.WEIGHT_SETS)
def test_oracle_against_float64_and_branch_coverage(name):
    """The float32 oracle agrees with float64 to float32's error on every case (a disagreement beyond that is a different operation, not
    rounding), the encoder stays inside the range the fixed-point sums assume, and every epilogue branch is reached."""
    b = C.bundle(name)
    cover = dict(sp_log=0.0, sp_10_20=0.0, sp_20_88=0.0, sp_over_88=0.0, tanh_linear=0.0, tanh_saturated=0.0)
    for case, x in b.dec.items():
        assert x.shape == (C.N_ROWS, 32) and x.dtype == F32 and np.isfinite(x).all()
        sdf, std, ps, pu = b.dec64[case]
        e_sdf, e_std = b.dec_e_ref(case)
        # float32 carries 2^-24 per operation through four layers of 128-term sums: 1e-4 of the largest pre-activation bounds it amply
        assert e_sdf < 1e-4 * max(1.0, np.abs(ps).max()) and e_std < 1e-4 * max(1.0, np.abs(pu).max()), (case, e_sdf, e_std)
        for key, frac in (("sp_log", (pu <= 10).mean()), ("sp_10_20", ((pu > 10) & (pu <= 20)).mean()), ("sp_20_88", ((pu > 20) & (pu <= 88)).mean()),
                          ("sp_over_88", (pu > 88).mean()), ("tanh_linear", (np.abs(sdf) < 0.9).mean()), ("tanh_saturated", (np.abs(sdf) > 0.999).mean())):
            cover[key] = max(cover[key], float(frac))
    assert min(cover.values()) >= 0.01, (name, cover)
    for case, x in b.enc.items():
        assert x.shape == (C.N_ROWS, 6) and x.dtype == F32
        assert np.abs(b.enc64[case]).max() < C.ENC_LIMIT, (case, np.abs(b.enc64[case]).max())
        assert max(b.enc_e_ref(case)) < 1e-4 * max(1.0, np.abs(b.enc64[case]).max()), case


def _torch_decoder(ref, x, dtype):
    """plain torch restatement of di_decoder.py:55-86 on ref's folded weights -> sdf (N,), std (N,)"""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    x0 = x
    h = x0
    for layer in range(4):
        if layer == 3:
            h = torch.cat([h, x0], dim=1)
        h = torch.relu(torch.nn.functional.linear(h, t(ref.dec_W[layer]), t(ref.dec_b[layer])))
    std = 0.05 + 0.5 * torch.nn.functional.softplus(torch.nn.functional.linear(h, t(ref.unc_W), t(ref.unc_b)))
    return torch.tanh(torch.nn.functional.linear(h, t(ref.dec_W[4]), t(ref.dec_b[4])))[:, 0], std[:, 0]


def _torch_grad(ref, x, dtype):
    xt = torch.from_numpy(x).to(dtype).requires_grad_(True)
    sdf, _ = _torch_decoder(ref, xt, dtype)
    (g,) = torch.autograd.grad(sdf.sum(), xt)
    return sdf.detach().numpy(), g[:, 29:].numpy()


@pytest.mark.parametrize("name", C.WEIGHT_SETS)
def test_gradient_against_float64_autograd(name):
    b = C.bundle(name)
    for s in (0.3, 4.0, 16.0):
        x = C.decoder_rows_scale(s, 1024, seed=7)
        sdf, _, g = b.ref.decoder_xyz_grad(x)
        ts, tg = _torch_grad(b.ref, x, torch.float64)
        assert np.abs(sdf - ts).max() < 1e-12 and np.abs(g - tg).max() <= 1e-12 * max(1.0, np.abs(tg).max())


@pytest.mark.parametrize("name", C.WEIGHT_SETS)
def test_query_set_keeps_the_oracle_under_the_kink_cap(name):
    """The very query rows of test_gpu_mlp_envelope.test_point_queries (an OracleMap on seq_small with the planted latents; no GPU
    needed): the rows set aside for a ReLU kink are at most 1 % of each set, and on the rest the float32 oracle's own gradient is a
    float32 error away from float64, not a kink's jump."""
    b = C.bundle(name)
    for scale in C.QUERY_SCALES:
        om, n, _, _ = C.planted_oracle_map(b.oracle, C.WEIGHT_SETS.index(name), scale)
        _, rows = C.query_rows(om, n, C.N_ROWS, C.QUERY_SEED)
        keep = b.grad_keep(rows)
        assert (~keep).mean() <= 0.01, (name, scale, (~keep).mean())
        g64 = b.ref.decoder_xyz_grad(rows)[2]
        e = C.max_err(b.oracle.decoder_xyz_grad(rows)[2][keep], g64[keep])
        assert e <= 1e-4 * max(1.0, np.abs(g64[keep]).max()), (name, scale, e)


# ---- the optimiser's loss, Adam, the regulariser -----------------------------------------------------------------------------------
def _torch_nll(ref, x, gt, n, dtype):
    """map.py:88-95 as torch writes it -> loss (scalar tensor), x (the leaf)"""
    xt = torch.from_numpy(np.ascontiguousarray(x)).to(dtype).requires_grad_(True)
    sdf, std = _torch_decoder(ref, xt, dtype)
    gtc = torch.clamp(torch.from_numpy(np.ascontiguousarray(gt)).to(dtype), -0.2, 0.2)
    ll = -torch.distributions.Normal(loc=torch.clamp(sdf, -0.2, 0.2), scale=std).log_prob(gtc)
    return ll.sum() / n, xt


def _nll_rows(name, s, n=1024, seed=9):
    g = np.random.default_rng([seed, int(s * 10)])
    return C.decoder_rows_scale(s, n, seed=seed), (0.05 * OC.planted_noise(g, n)).astype(F32)


@pytest.mark.parametrize("name", C.WEIGHT_SETS)
def test_nll_gradient_against_float64_autograd(name):
    """Ref64.decoder_nll_grad against float64 autograd of the loss written with torch.distributions.Normal(...).log_prob: the loss, the
    gradient with respect to all 32 inputs, and that its two parts add up to it.  (F.softplus in float64 has the `> 20` shortcut; it
    differs from the plain sigmoid by < 2.1e-9 relative on the uncertainty head's part only.)"""
    b = C.bundle(name)
    for s in (0.3, 4.0, 16.0):
        x, gt = _nll_rows(name, s)
        n = x.shape[0]
        r = b.ref.decoder_nll_grad(x, gt, n)
        loss, xt = _torch_nll(b.ref, x, gt, n, torch.float64)
        (tg,) = torch.autograd.grad(loss, xt)
        tg = tg.numpy()
        assert abs(r["loss"].sum() - loss.item()) <= 1e-12 * max(1.0, abs(loss.item()))
        tol = 1e-11 * max(1e-300, np.abs(tg).max()) + 2.1e-9 * (r["pu"] > 20)[:, None] * r["grad_abs"]
        assert (np.abs(r["grad"] - tg) <= tol).all(), (name, s, np.abs(r["grad"] - tg).max(), np.abs(tg).max())
        assert (r["grad_abs"] >= np.abs(r["grad"]) * (1 - 1e-12)).all()
        # the clamp passes the gradient on the closed interval: a row exactly at the clamp keeps its sdf-head part
        assert ((np.abs(r["sdf"]) <= 0.2).mean() > 0) or s > 0.3


def test_nll_gradient_closed_clamp_interval_and_target_clamp():
    """|sdf| = 0.2 exactly passes the gradient (torch.clamp's backward is `min <= x <= max`), and a target beyond +-0.2 is clamped."""
    x = torch.tensor([-0.2, 0.2, 0.2000001, -0.3], dtype=torch.float64, requires_grad=True)
    torch.clamp(x, -0.2, 0.2).sum().backward()
    assert x.grad.tolist() == [1.0, 1.0, 0.0, 0.0]
    b = C.bundle("shipped")
    x, gt = _nll_rows("shipped", 0.3, 64)
    far = b.ref.decoder_nll_grad(x, np.full(64, 7.0), 64)
    at = b.ref.decoder_nll_grad(x, np.full(64, 0.2), 64)
    assert np.array_equal(far["grad"], at["grad"]) and np.array_equal(far["loss"], at["loss"])


def test_adam_and_regulariser_against_torch_float64():
    """Five steps of torch.optim.Adam (float64, defaults, lr 1e-2) on a quadratic plus the code regulariser written as the reference
    writes it (map.py:98-99), against ref64.adam_step64 with code_reg_grad64; one all-zero latent, whose regulariser subgradient is 0
    (torch.norm's backward) while the float32 oracle's z / |z| divides 0 by 0 there."""
    from tests.ref64 import adam_step64, code_reg_grad64
    g = np.random.default_rng(3)
    z0 = g.standard_normal((7, 29))
    z0[2] = 0.0
    A, lam, n = g.standard_normal((29, 29)), 0.01, 13
    zt = torch.from_numpy(z0.copy()).requires_grad_(True)
    opt = torch.optim.Adam([zt], lr=1.0e-2)
    z, m, v = z0.copy(), np.zeros_like(z0), np.zeros_like(z0)
    for it in range(1, 6):
        opt.zero_grad()
        (((zt @ torch.from_numpy(A)) ** 2).sum() / n + lam * torch.sum(torch.norm(zt, dim=1)) / n).backward()
        grad = 2.0 * ((z @ A) @ A.T) / n + code_reg_grad64(z, lam, n)
        assert np.abs(grad - zt.grad.numpy()).max() <= 1e-13 * np.abs(grad).max()
        if it == 1:
            assert (code_reg_grad64(z, lam, n)[2] == 0).all() and np.isfinite(zt.grad.numpy()[2]).all()
        opt.step()
        z, m, v = adam_step64(z, m, v, grad, it)
        assert np.abs(z - zt.detach().numpy()).max() <= 1e-13, it
    with np.errstate(invalid="ignore", divide="ignore"):
        zz = np.zeros((1, 29), dtype=F32)
        assert np.isnan(F32(lam) * zz / np.sqrt((zz * zz).sum(axis=1, keepdims=True))).all()       # what OracleMap._optimize_stage evaluates there


def test_gather_restatement_matches_the_oracle():
    """optim_cases.gather_rows (points, normals, mask, map state -> rows) against OracleMap._optimize_stage's own gather on a map whose
    state is planted the same way: the oracle's rows are recovered from the rows it hands to decoder_nll_grad."""
    b = C.bundle("shipped")
    case = OC.block_case("shipped", 0.3)
    pm = case.pm
    om = O.OracleMap(b.oracle, OC.BOUND_MIN, tuple(-v for v in OC.BOUND_MIN), OC.VOXEL)
    om.allocate_block(pm.pos[:pm.n])
    om.latent_vecs[:pm.n], om.voxel_obs_count[:pm.n], om.voxel_optimized[:pm.n] = pm.latent[:pm.n], pm.obs[:pm.n], pm.optimized[:pm.n].astype(bool)
    om.optim_n_iters = 1
    seen = {}
    real = b.oracle.decoder_nll_grad
    try:
        b.oracle.decoder_nll_grad = lambda x, gt, n: (seen.update(x=x.copy(), gt=gt.copy(), n=n), real(x, gt, n))[1]
        xn, lin = om.voxelize(case.xyz)
        om._optimize_stage(xn, lin, case.normal, case.noise)
    finally:
        del b.oracle.decoder_nll_grad
    assert seen["n"] == case.n_rows and np.array_equal(seen["gt"], case.row_sdf)
    assert np.array_equal(seen["x"][:, 29:], case.row_xyz) and np.array_equal(seen["x"][:, :29], pm.latent[case.row_slot])
    assert om.last_stats["optim_voxels"] == case.uniq.size
    assert np.array_equal(np.nonzero(om.voxel_optimized)[0], np.union1d(case.uniq, np.nonzero(pm.optimized)[0]))
    # and on the scene that meets every clause of the gather (mask-0 points are what the caller prunes: the oracle sees the others;
    # NaN and out-of-grid points it cannot index, so they are left to the GPU test's restatement alone)
    pm, xyz, nrm, mask, noise = OC.messy_scene(513, 1024, 0)
    c = np.ceil(((xyz - pm.bound_min[None, :]) / F32(pm.voxel_size)).astype(F32))
    ok = mask.astype(bool) & np.isfinite(xyz).all(axis=1) & (c >= 1).all(axis=1) & (c <= OC.GRID).all(axis=1)
    om = O.OracleMap(b.oracle, OC.BOUND_MIN, tuple(-v for v in OC.BOUND_MIN), OC.VOXEL)
    om.allocate_block(pm.pos[:pm.n])
    om.latent_vecs[:pm.n], om.voxel_obs_count[:pm.n], om.voxel_optimized[:pm.n] = pm.latent[:pm.n], pm.obs[:pm.n], pm.optimized[:pm.n].astype(bool)
    om.optim_n_iters = 1
    try:
        b.oracle.decoder_nll_grad = lambda x, gt, n: (seen.update(x=x.copy(), gt=gt.copy(), n=n), real(x, gt, n))[1]
        xn, lin = om.voxelize(xyz[ok])
        om._optimize_stage(xn, lin, nrm[ok], noise)
    finally:
        del b.oracle.decoder_nll_grad
    slot, rxyz, rsdf = OC.gather_rows(pm, xyz, nrm, mask, noise)
    assert seen["n"] == slot.size > 1000 and np.array_equal(seen["gt"], rsdf) and np.array_equal(seen["x"][:, 29:], rxyz)
    assert np.array_equal(seen["x"][:, :29], pm.latent[slot]) and 0 not in pm.pos[slot]


# ---- the integrate chain's restatement (tests/integrate_cases.py) -------------------------------------------------------------------
def _integrate_cases():
    from tests import integrate_cases as IC
    return IC, [IC.faces_case(n, p) for n in IC.FACES_N for p in (0, 1)] + [IC.runs_case(4), IC.runs_case(0), IC.corners_case(), IC.alloc64_case(),
                                                                             IC.threshold_case(), IC.chain_case(n_frames=3), IC.frame_case(32, 48), IC.frame_case(24, 40)]


def test_integrate_restatement_matches_the_oracle():
    """integrate_cases.restate against OracleMap.integrate_keyframe on every case the oracle can take (all but the capacity overflow; NaN
    and out-of-grid points, invalid in both, are taken out of the oracle's cloud: it would index with them): mask, indexer, positions,
    counts, n_occupied, M, C and the update set bit for bit over all frames; latents, fused by fuse32 from the oracle's own float32
    encoder rows, to the oracle's rounding: its float32 running sum of cnt rows is off by at most cnt ulp of the sum of magnitudes, the
    fixed point by half a unit per row, and three more roundings follow."""
    IC, cases = _integrate_cases()
    _, oracle = IC.nets("shipped")
    for case in cases:
        pm = case.pm.clone()
        hi = tuple(float(v) + pm.grid * pm.voxel_size for v in OC.BOUND_MIN)
        om = O.OracleMap(oracle, OC.BOUND_MIN, hi, pm.voxel_size, prune_min_vox_obs=case.prune_min, encoder_count_th=IC.TH)
        assert om.n_xyz == [pm.grid] * 3, (case.label, om.n_xyz)
        om.allocate_block(pm.pos[:pm.n])
        om.latent_vecs[:pm.n], om.voxel_obs_count[:pm.n] = pm.latent[:pm.n], pm.obs[:pm.n]
        for f, (xyz, nrm) in enumerate(case.frames):
            label = f"{case.label} frame {f}"
            k = min(pm.capacity, om.latent_vecs.shape[0])
            pm.latent[:k] = om.latent_vecs[:k]                       # every frame is judged from the oracle's own previous latents
            z_old = pm.latent.copy()
            r = IC.restate(pm, xyz, nrm, case.prune_min)
            ok = r.pt_lin >= 0
            omask = om.integrate_keyframe(xyz[ok], nrm[ok])
            mask = np.zeros(r.N, dtype=np.uint8)
            mask[ok] = 1 if omask is None else omask
            assert np.array_equal(mask, r.mask), label
            assert om.n_occupied == pm.n and np.array_equal(om.indexer, pm.indexer) and np.array_equal(om.latent_vecs_pos[:pm.n], pm.pos[:pm.n]), label
            assert np.array_equal(om.voxel_obs_count[:pm.n].view(np.uint32), pm.obs[:pm.n].view(np.uint32)), label
            assert om.last_stats["M"] == r.M and om.last_stats["C"] == r.C, (label, om.last_stats, r.M, r.C)
            assert np.array_equal(np.nonzero(pm.dirty)[0], om.updated_vec_id), label
            if r.M:
                assert not IC.nonfinite_rows(r.rows).any(), label
                enc = oracle.encoder(r.rows)
                z_new, w_new = IC.fuse32(z_old[r.uniq], r.w_old[r.uniq], IC.fixed_sums(r, enc), r.cnt)
                pm.latent[r.uniq] = z_new
                assert np.array_equal(w_new.view(np.uint32), pm.obs[r.uniq].view(np.uint32)), label
                mag = np.zeros((r.C, 29))
                np.add.at(mag, r.inv, np.abs(enc.astype(np.float64)))
                with np.errstate(invalid="ignore"):
                    mag = (mag + np.abs(z_old[r.uniq].astype(np.float64)) * r.w_old[r.uniq][:, None]) / w_new[:, None]
                tol = (r.cnt[:, None] + 3.0) * 2.0 ** -24 * mag + r.cnt[:, None] * 2.0 ** -31 / w_new[:, None]
                err = np.abs(om.latent_vecs[r.uniq].astype(np.float64) - z_new)
                assert (err <= tol).all(), (label, float(np.nanmax(err / tol)))
            rest = np.ones(pm.capacity, dtype=bool)
            rest[r.uniq] = False
            rest[om.latent_vecs.shape[0]:] = False
            assert np.array_equal(om.latent_vecs[rest[:om.latent_vecs.shape[0]]].view(np.uint32), pm.latent[rest].view(np.uint32)), label


def test_integrate_cases_reach_their_paths():
    """What each case is there for, asserted from the restatement alone (the GPU test asserts the same from what it reads back): the
    chain case's slots with more run records than a directory holds (14) beside slots with fewer, a workgroup with more distinct slots
    than k_focus_gather's 256-entry table, alloc64's new voxels in at least three scan blocks, the overflow case 8 short, the frame
    cases on either walk with holes, zeros and kept points, exact voxel faces among the faces case's points, and the thresholds."""
    IC, _ = _integrate_cases()
    c = IC.chain_case(n_frames=1)
    pm = c.pm.clone()
    r = IC.restate(pm, *c.frames[0], c.prune_min)
    got = IC.reach(r)
    block = pm.indexer[OC.lin_of(np.stack(np.meshgrid(*[np.arange(6, 9)] * 3, indexing="ij"), axis=-1).reshape(-1, 3))]
    own = np.unique(np.stack([IC.workgroup_of(r.key, r.N), r.slot], axis=1)[np.isin(r.slot, block)], axis=0)
    assert np.bincount(own[:, 1])[block].min() >= 29, np.bincount(own[:, 1])[block].min()
    assert got["max_runs"] > IC.DIR_IDS and got["min_runs"] <= IC.DIR_IDS and got["max_slots_per_wg"] > 256, got
    assert r.M < 8 * r.N and r.M % 32 != 0                                   # a partly filled last tile
    c = IC.alloc64_case()
    pm = c.pm.clone()
    r = IC.restate(pm, *c.frames[0], c.prune_min)
    assert 280 <= r.alloc_new <= 330 and np.unique(r.candidates // 32 // 256).size >= 3 and r.n_before == 40, (r.alloc_new, r.n_before)
    assert pm.grid ** 3 // 32 > 4096
    c = IC.overflow_case()
    pm = c.pm.clone()
    r = IC.restate(pm, *c.frames[0], c.prune_min)
    assert r.overflow == 1 and pm.n == pm.capacity == r.n_before + r.alloc_new - 8 and (pm.indexer[r.candidates[-8:]] == -1).all()
    for hw in ((32, 48), (24, 40)):
        c = IC.frame_case(*hw)
        r = IC.restate(c.pm.clone(), *c.frames[0], c.prune_min)
        assert np.isnan(c.depth).sum() > 20 and (c.depth == 0).sum() > 5 and r.mask.sum() > r.N // 2 and r.M > 1000 and r.alloc_new > 20, (hw, r.M)
        assert (r.pt_lin < 0).sum() == np.isnan(c.depth).sum()
    c = IC.faces_case(257, 0)
    xyz = c.frames[0][0]
    with np.errstate(invalid="ignore"):
        xn = ((xyz - np.asarray(OC.BOUND_MIN, dtype=F32)) / F32(OC.VOXEL)).astype(F32)
    on_face = np.isfinite(xn) & (xn == np.round(xn))
    lin = IC.voxel_ids(c.pm, xyz)
    assert on_face.any(axis=1).sum() >= 20 and (xn == 0).any() and (xn == 16).any() and (lin < 0).sum() >= 20 and (lin >= 0).sum() >= 150
    top = (np.asarray(OC.BOUND_MIN, dtype=np.float64) + 16 * OC.VOXEL).astype(F32)
    assert IC.voxel_ids(c.pm, top[None, :])[0] == 16 ** 3 - 1 and IC.voxel_ids(c.pm, np.asarray(OC.BOUND_MIN, dtype=F32)[None, :])[0] == -1
    c = IC.threshold_case()
    pm = c.pm.clone()
    s = lambda v: pm.indexer[OC.lin_of(v)]
    r0 = IC.restate(pm, *c.frames[0], c.prune_min)
    assert s([4, 4, 4]) in r0.uniq and s([4, 4, 5]) not in r0.uniq and s([4, 4, 6]) not in r0.uniq          # th - 1 in; th + 1 and th out
    assert pm.obs[s([4, 4, 4])] >= IC.TH
    from_outside = r0.pt_lin[r0.i] == OC.lin_of([4, 4, 5])                       # points of the th + 1 voxel: focus passed, rows go to th - 1 alone
    assert from_outside.any() and (r0.slot[from_outside] == s([4, 4, 4])).all()
    r1 = IC.restate(pm, *c.frames[1], c.prune_min)
    assert s([4, 4, 4]) not in r1.uniq and s([13, 13, 2]) in r1.uniq
    c = IC.runs_case(4)
    r = IC.restate(c.pm.clone(), *c.frames[0], c.prune_min)
    cnt = np.bincount(r.pt_lin[r.pt_lin >= 0], minlength=4096)
    assert not r.mask[cnt[r.pt_lin] == 4].any() and r.mask[cnt[r.pt_lin] == 5].all() and (cnt[r.pt_lin] == 4).sum() == 8


# ---- K ------------------------------------------------------------------------------------------------------------------------------
def _seq_linear(h, W, b):
    """strict left-to-right float32 accumulation of h @ W.T, then + b"""
    acc = np.zeros((h.shape[0], W.shape[0]), dtype=F32)
    tmp = np.empty_like(acc)
    Wt = np.ascontiguousarray(W.T)
    for k in range(W.shape[1]):
        np.multiply(h[:, k:k + 1], Wt[k], out=tmp)
        acc += tmp
    return acc + b


def _seq_decoder(on, x):
    x0 = x.astype(F32)
    h = x0
    for layer in range(4):
        if layer == 3:
            h = np.concatenate([h, x0], axis=1)
        h = np.maximum(_seq_linear(h, on.dec_W[layer], on.dec_b[layer]), F32(0))
    std = (F32(0.05) + F32(0.5) * O._softplus(_seq_linear(h, on.unc_W, on.unc_b))).astype(F32)
    return np.tanh(_seq_linear(h, on.dec_W[4], on.dec_b[4])).astype(F32)[:, 0], std[:, 0]


def _seq_nll_sums(case):
    """OracleNetworks.decoder_nll_grad's arithmetic with every matrix product accumulated strictly left to right, per-voxel sums in row order"""
    import math
    on, x0, n = case.b.oracle, case.rows_at(case.pm.latent[case.uniq]).astype(F32), case.n_rows
    h, masks = x0, []
    for layer in range(4):
        if layer == 3:
            h = np.concatenate([h, x0], axis=1)
        h = _seq_linear(h, on.dec_W[layer], on.dec_b[layer])
        masks.append(h > 0)
        h = np.maximum(h, F32(0))
    ps, pu = _seq_linear(h, on.dec_W[4], on.dec_b[4])[:, 0], _seq_linear(h, on.unc_W, on.unc_b)[:, 0]
    mu, sigma = np.tanh(ps).astype(F32), (F32(0.05) + F32(0.5) * O._softplus(pu)).astype(F32)
    diff = (np.clip(case.row_sdf, F32(-0.2), F32(0.2)) - np.clip(mu, F32(-0.2), F32(0.2))).astype(F32)
    inv_n = F32(1.0 / n)
    d_mu = (-diff / (sigma * sigma) * ((mu >= F32(-0.2)) & (mu <= F32(0.2)))).astype(F32)
    d_sigma = (F32(1) / sigma - diff * diff / (sigma * sigma * sigma)).astype(F32)
    a = (inv_n * d_mu * (F32(1) - mu * mu)).astype(F32)
    with np.errstate(over="ignore"):
        bb = (inv_n * d_sigma * F32(0.5) * np.where(pu > F32(20), F32(1), F32(1) / (F32(1) + np.exp(-pu)))).astype(F32)
    gh = (a[:, None] * on.dec_W[4] + bb[:, None] * on.unc_W).astype(F32)
    gx = np.zeros_like(x0)
    for layer in (3, 2, 1, 0):
        gin = _seq_linear((gh * masks[layer]).astype(F32), np.ascontiguousarray(on.dec_W[layer].T), F32(0))
        if layer == 3:
            gx += gin[:, 96:]
            gin = gin[:, :96]
        gh = gin
    gx += gh
    return case.sums(gx[:, :29].astype(F32))


def _torch_nll_sums(case, ref32):
    """torch float32 autograd of the loss with respect to the per-voxel latents (the gather's backward adds the rows up)"""
    z = torch.from_numpy(case.pm.latent[case.uniq].copy()).requires_grad_(True)
    x = torch.cat([z[torch.from_numpy(case.inv)], torch.from_numpy(case.row_xyz)], dim=1)
    sdf, std = _torch_decoder(ref32, x, torch.float32)
    ll = -torch.distributions.Normal(loc=torch.clamp(sdf, -0.2, 0.2), scale=std).log_prob(torch.clamp(torch.from_numpy(case.row_sdf), -0.2, 0.2))
    (g,) = torch.autograd.grad(ll.sum() / case.n_rows, z)
    return g.numpy()


def _encoder_f32(on, x, linear):
    h = x.astype(F32)
    for l in on.enc:
        h = linear(h, l["W"], F32(0))
        h = np.maximum(((h - l["mean"]) / np.sqrt(l["var"] + F32(1e-5)) * l["gamma"] + l["beta"]).astype(F32), F32(0))
    return linear(h, on.enc_last_W, on.enc_last_b)


def _torch_linear(h, W, b):
    return (torch.nn.functional.linear(torch.from_numpy(np.ascontiguousarray(h)), torch.from_numpy(np.ascontiguousarray(W))).numpy() + b).astype(F32)


def k_table():
    """rows of (weight set, network, case, output, worst error of [oracle, torch float32, sequential float32], largest / smallest)"""
    from concurrent.futures import ThreadPoolExecutor
    bundles = [C.bundle(name) for name in C.WEIGHT_SETS]
    with ThreadPoolExecutor(len(bundles)) as pool:           # (the sequential accumulation is slow in numpy; its ufuncs release the GIL)
        return [r for rows in pool.map(_k_rows, bundles) for r in rows]


def _k_rows(b):
    rows, name = [], b.name
    ref32 = Ref64(b.raw)                                   # torch float32 runs on the float64-folded weights cast to float32
    for case, x in b.dec.items():
        o = b.oracle.decoder(x)
        with torch.no_grad():
            t = _torch_decoder(ref32, torch.from_numpy(x), torch.float32)
        s = _seq_decoder(b.oracle, x)
        for j, out in enumerate(("sdf", "std")):
            e = [C.max_err(o[j][:, 0], b.dec64[case][j]), C.max_err(t[j].numpy(), b.dec64[case][j]), C.max_err(s[j], b.dec64[case][j])]
            rows.append((name, "decoder", case, out, e, max(e) / min(e)))
    for case, x in b.enc.items():
        outs = [b.oracle.encoder(x), _encoder_f32(b.oracle, x, _torch_linear), _encoder_f32(b.oracle, x, _seq_linear)]
        for gi, g in enumerate(C.ENC_GROUPS):
            e = [C.max_err(o[:, g], b.enc64[case][:, g]) for o in outs]
            rows.append((name, "encoder", case, f"ch{4 * gi}-{g.stop - 1}", e, max(e) / min(e)))
    for s in (0.3, 4.0, 16.0):                            # gradient: the oracle's hand-written chain and torch float32 autograd
        x = C.decoder_rows_scale(s, C.N_ROWS, seed=7)
        g64 = b.ref.decoder_xyz_grad(x)[2]
        keep = b.grad_keep(x)                                 # rows on a ReLU kink: a cap of 1 %, met by the oracle alone
        assert (~keep).mean() <= 0.01, (name, s, (~keep).mean())
        e = [C.max_err(b.oracle.decoder_xyz_grad(x)[2][keep], g64[keep]), C.max_err(_torch_grad(ref32, x, torch.float32)[1][keep], g64[keep])]
        rows.append((name, "gradient", f"N(0,{s:g})", "d sdf / d xyz", e, max(e) / min(e)))
    # the optimiser's per-voxel gradient sums, on the very cases tests/test_gpu_optim_envelope.py runs (their points are filtered already)
    for ws, s in OC.ONE_STEP + [(w, OC.NEAR_SWITCH) for w in C.WEIGHT_SETS] + [("large_pu", 0.0)]:
        if name != (ws if ws != "large_pu" else "shipped"):
            continue
        case = OC.one_step_case(ws, s)
        g64 = case.grad64()["G"]
        e = [C.max_err(case.grad32()[0], g64), C.max_err(_torch_nll_sums(case, ref32), g64), C.max_err(_seq_nll_sums(case), g64)]
        rows.append((name, "nll gradient", case.label.split("/")[1], "d loss / d z per voxel", e, max(e) / min(e)))
    return rows


def test_k_of_the_bar():
    """K_BAR is twice the largest ratio between honest float32 evaluations: re-measured here, and not more than twice that again (a K
    that has drifted far above the measurement protects nothing)."""
    rows = k_table()
    nll = [r for r in rows if r[1] == "nll gradient"]
    rows = [r for r in rows if r[1] != "nll gradient"]
    worst_nll = max(r[5] for r in nll)
    print(f"nll gradient: largest ratio {worst_nll:.2f} over {len(nll)} cases; K_NLL = {OC.K_NLL}")
    for r in nll:
        print(f"  {r[0]} / {r[2]}: {r[5]:.2f}  errors {['%.3g' % e for e in r[4]]}")
    worst = max(r[5] for r in rows)
    print(f"largest ratio {worst:.2f} over {len(rows)} (weight set, case, output) triples; K_BAR = {C.K_BAR}")
    for net in ("decoder", "encoder", "gradient"):
        r = max((r for r in rows if r[1] == net), key=lambda r: r[5])
        print(f"  {net}: {r[5]:.2f} at {r[0]} / {r[2]} / {r[3]}  errors {['%.3g' % e for e in r[4]]}")
    # 10 % of slack on the upper side: the ratios depend on the BLAS build's summation order (3.19 where K_BAR was set); past that, or
    # below half of it, the constant no longer describes the measurement and has to be derived again
    assert C.K_BAR / 4.0 <= worst <= 1.1 * C.K_BAR / 2.0, worst
    assert OC.K_NLL / 4.0 <= worst_nll <= 1.1 * OC.K_NLL / 2.0, worst_nll


if __name__ == "__main__":
    rows = k_table()
    if "--all" in sys.argv:
        print("| weight set | network | case | output | oracle (BLAS) | torch float32 | sequential | largest / smallest |")
        print("|---|---|---|---|---|---|---|---|")
    else:                                      # per weight set and output kind: the triple with the largest ratio
        print("| weight set | network | output | case of the largest ratio | oracle (BLAS) | torch float32 | sequential | largest / smallest |")
        print("|---|---|---|---|---|---|---|---|")
        best = {}
        for r in rows:
            key = (r[0], r[1], r[3] if r[1] == "decoder" else r[2] if r[1] == "nll gradient" else "")
            if key not in best or r[5] > best[key][5]:
                best[key] = r
        rows = list(best.values())
    for name, net, case, out, e, r in rows:
        e = ["%.3g" % v for v in e] + ["-"] * (3 - len(e))
        cols = [name, net, case, out] if "--all" in sys.argv else [name, net, out, case]
        print("| " + " | ".join(cols + e + ["%.2f" % r]) + " |")
