"""Pins tests/ref64.py (the float64 statement of the networks) and the generators of tests/mlp_cases.py.  No GPU.

  * against tests/golden/networks.npz: the reference's own rows;
  * against OracleNetworks (float32) on every weight set and input class: the oracle's worst error is what float32 costs there;
  * the analytic input gradient against float64 torch.autograd on a plain torch restatement;
  * that every weight set reaches every branch of the epilogue (softplus below 20, above 20, where expf would overflow; tanh in its
    linear part and saturated) on at least 1 % of the rows of some case;
  * K of the GPU bar, re-measured (see mlp_cases.K_BAR).

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
    return rows


def test_k_of_the_bar():
    """K_BAR is twice the largest ratio between honest float32 evaluations: re-measured here, and not more than twice that again (a K
    that has drifted far above the measurement protects nothing)."""
    rows = k_table()
    worst = max(r[5] for r in rows)
    print(f"largest ratio {worst:.2f} over {len(rows)} (weight set, case, output) triples; K_BAR = {C.K_BAR}")
    for net in ("decoder", "encoder", "gradient"):
        r = max((r for r in rows if r[1] == net), key=lambda r: r[5])
        print(f"  {net}: {r[5]:.2f} at {r[0]} / {r[2]} / {r[3]}  errors {['%.3g' % e for e in r[4]]}")
    # 10 % of slack on the upper side: the ratios depend on the BLAS build's summation order (3.19 where K_BAR was set); past that, or
    # below half of it, the constant no longer describes the measurement and has to be derived again
    assert C.K_BAR / 4.0 <= worst <= 1.1 * C.K_BAR / 2.0, worst


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
            key = (r[0], r[1], r[3] if r[1] == "decoder" else "")
            if key not in best or r[5] > best[key][5]:
                best[key] = r
        rows = list(best.values())
    for name, net, case, out, e, r in rows:
        e = ["%.3g" % v for v in e] + ["-"] * (3 - len(e))
        cols = [name, net, case, out] if "--all" in sys.argv else [name, net, out, case]
        print("| " + " | ".join(cols + e + ["%.2f" % r]) + " |")
