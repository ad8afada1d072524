"""Float64 statement of the two networks and of the lattice decode.  TEST INFRASTRUCTURE ONLY.

Plain numpy float64, built from the raw weight dict the way the reference builds its modules: weight norm `v * g / ||v||` per output
row (di_decoder.py:37-40), eval-mode batch norm with eps = 1e-5 (pt_util.py:76-127), the skip connection into decoder layer 3
(di_decoder.py:61-62), `tanh` on the sdf head and `0.05 + 0.5 * softplus` on the uncertainty head (di_decoder.py:65-68,84).

It imports neither `oracle/` nor `di_fusion_amd.network.packing`: it is an independent statement of the operation that both the float32
oracle and the kernels are measured against (tests/test_ref64_cpu.py pins it, tests/test_gpu_mlp_envelope.py uses it).
"""
from __future__ import annotations

import numpy as np

F64 = np.float64
BN_EPS = 1e-5
NLL_CLAMP = 0.2             # map.py:90-91: prediction and target are clamped to +-0.2 before the likelihood
REFINE_TH = 0.05            # map.py:667: samples with |interpolated sdf| < 0.05 are decoded again


def softplus64(x):
    """log(1 + e^x) without overflow (no threshold: in float64 the `x > 20` shortcut of F.softplus differs from this by < 2.1e-9 absolute)."""
    x = np.asarray(x, dtype=F64)
    with np.errstate(invalid="ignore"):
        return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def code_reg_grad64(z, lam: float, n: int):
    """d / dz of  lam * sum_voxels |z_u| / n  (map.py:98-101): lam * z / |z| / n, with the subgradient 0 at z = 0 (torch.norm's backward).
    z (U,29) -> (U,29)."""
    z = np.asarray(z, dtype=F64)
    nrm = np.sqrt((z * z).sum(axis=1, keepdims=True))
    return np.where(nrm > 0, lam * z / np.where(nrm > 0, nrm, 1.0) / n, 0.0)


def adam_step64(z, m, v, g, it: int, lr=1e-2, b1=0.9, b2=0.999, eps=1e-8):
    """Step `it` (1-based) of torch.optim.Adam with its defaults (no weight decay, no amsgrad) -> z, m, v."""
    m = b1 * np.asarray(m, dtype=F64) + (1.0 - b1) * g
    v = b2 * np.asarray(v, dtype=F64) + (1.0 - b2) * g * g
    return adam_update64(z, m, v, it, lr, b1, b2, eps), m, v


def adam_update64(z, m, v, it: int, lr=1e-2, b1=0.9, b2=0.999, eps=1e-8):
    """The parameter update of that step from the moments it has just formed."""
    return np.asarray(z, dtype=F64) - (lr / (1.0 - b1 ** it)) * (m / (np.sqrt(v) / np.sqrt(1.0 - b2 ** it) + eps))


class Ref64:
    def __init__(self, weights: dict):
        w = {k: np.asarray(v, dtype=F64) for k, v in weights.items()}
        self.dec_W, self.dec_b = [], []
        for i in range(5):
            v, g = w[f"decoder.lin{i}.weight_v"], w[f"decoder.lin{i}.weight_g"]
            self.dec_W.append(v * (g / np.sqrt((v * v).sum(axis=1, keepdims=True))))
            self.dec_b.append(w[f"decoder.lin{i}.bias"])
        self.unc_W, self.unc_b = w["decoder.uncertainty_layer.weight"], w["decoder.uncertainty_layer.bias"]
        self.enc = []
        for i in range(3):
            p = f"encoder.mlp.layer{i}."
            self.enc.append((w[p + "conv.weight"][:, :, 0], w[p + "normlayer.bn.weight"], w[p + "normlayer.bn.bias"],
                             w[p + "normlayer.bn.running_mean"], w[p + "normlayer.bn.running_var"]))
        self.enc_last_W, self.enc_last_b = w["encoder.mlp.layer3.conv.weight"][:, :, 0], w["encoder.mlp.layer3.conv.bias"]

    # ---- decoder ------------------------------------------------------------------------------------------------------------
    def _trunk(self, x):
        """The four hidden layers.  -> (h3 after ReLU, the four pre-activations)."""
        x0 = np.asarray(x, dtype=F64)
        h, pre = x0, []
        with np.errstate(invalid="ignore", over="ignore"):
            for layer in range(4):
                if layer == 3:
                    h = np.concatenate([h, x0], axis=1)
                a = h @ self.dec_W[layer].T + self.dec_b[layer]
                pre.append(a)
                h = np.where(np.isnan(a), a, np.maximum(a, 0.0))        # torch.relu: NaN stays NaN
        return h, pre

    def decoder(self, x):
        """x (N,32) = [latent 29 | xyz 3] -> sdf (N,), std (N,), ps (N,), pu (N,): the outputs and the two pre-activations."""
        h, _ = self._trunk(x)
        with np.errstate(invalid="ignore", over="ignore"):
            ps = (h @ self.dec_W[4].T + self.dec_b[4])[:, 0]
            pu = (h @ self.unc_W.T + self.unc_b)[:, 0]
            return np.tanh(ps), 0.05 + 0.5 * softplus64(pu), ps, pu

    def decoder_xyz_grad(self, x):
        """d sdf / d x[:, 29:32] by the analytic reverse chain -> sdf (N,), std (N,), grad (N,3)."""
        h, pre = self._trunk(x)
        ps = (h @ self.dec_W[4].T + self.dec_b[4])[:, 0]
        pu = (h @ self.unc_W.T + self.unc_b)[:, 0]
        sdf = np.tanh(ps)
        gh = (1.0 - sdf * sdf)[:, None] * self.dec_W[4]
        gx = np.zeros((h.shape[0], 3), dtype=F64)
        for layer in (3, 2, 1, 0):
            gin = (gh * (pre[layer] > 0)) @ self.dec_W[layer]
            if layer == 3:
                gx += gin[:, 96 + 29:]
                gin = gin[:, :96]
            gh = gin
        gx += gh[:, 29:]
        return sdf, 0.05 + 0.5 * softplus64(pu), gx

    def decoder_nll_grad(self, x, gt, n):
        """The optimiser's loss (map.py:87-96) and its gradient with respect to all 32 decoder inputs, per row:
            loss_i = -log N(clamp(gt_i); clamp(sdf_i), std_i) / n        (clamps at +-0.2; torch.distributions.Normal.log_prob)
        The clamp passes the gradient inside the CLOSED interval [-0.2, 0.2] (torch.clamp's backward); softplus' is the plain sigmoid (no
        threshold: above 20 it differs from 1 by < 2.1e-9).
        -> dict(loss (N,), grad (N,32), grad_abs (N,32): |sdf-head part| + |uncertainty-head part| of grad (the magnitude a relative error of
        either upstream head acts on), grad_unc (N,32): the uncertainty-head part alone, sdf, std, ps, pu (N,), pre: the four hidden pre-activations)."""
        h, pre = self._trunk(x)
        gt = np.asarray(gt, dtype=F64)
        with np.errstate(invalid="ignore", over="ignore"):
            ps = (h @ self.dec_W[4].T + self.dec_b[4])[:, 0]
            pu = (h @ self.unc_W.T + self.unc_b)[:, 0]
            sdf, std = np.tanh(ps), 0.05 + 0.5 * softplus64(pu)
            diff = np.clip(gt, -NLL_CLAMP, NLL_CLAMP) - np.clip(sdf, -NLL_CLAMP, NLL_CLAMP)
            var = std * std
            loss = (np.log(std) + 0.5 * np.log(2.0 * np.pi) + diff * diff / (2.0 * var)) / n
            d_mu = np.where((sdf >= -NLL_CLAMP) & (sdf <= NLL_CLAMP), -diff / var, 0.0)
            d_sigma = 1.0 / std - diff * diff / (var * std)
            a = d_mu * (1.0 - sdf * sdf) / n                                   # through tanh
            b = d_sigma * 0.5 / (1.0 + np.exp(-pu)) / n                        # through 0.05 + 0.5 * softplus
        N = h.shape[0]
        gh = np.concatenate([a[:, None] * self.dec_W[4], b[:, None] * self.unc_W], axis=0)      # the two heads through one (linear) chain
        gx = np.zeros((2 * N, 32), dtype=F64)
        for layer in (3, 2, 1, 0):
            gin = (gh * np.tile(pre[layer] > 0, (2, 1))) @ self.dec_W[layer]
            if layer == 3:
                gx += gin[:, 96:]                                                # the latent_in skip
                gin = gin[:, :96]
            gh = gin
        gx += gh
        return dict(loss=loss, grad=gx[:N] + gx[N:], grad_abs=np.abs(gx[:N]) + np.abs(gx[N:]), grad_unc=gx[N:], sdf=sdf, std=std, ps=ps, pu=pu, pre=pre)

    # ---- encoder ------------------------------------------------------------------------------------------------------------
    def encoder(self, x):
        """x (N,6) = [rel xyz | normal] -> (N,29)."""
        h = np.asarray(x, dtype=F64)
        with np.errstate(invalid="ignore", over="ignore"):
            for W, gamma, beta, mean, var in self.enc:
                a = (h @ W.T - mean) / np.sqrt(var + BN_EPS) * gamma + beta
                h = np.where(np.isnan(a), a, np.maximum(a, 0.0))
            return h @ self.enc_last_W.T + self.enc_last_b

    # ---- lattice ------------------------------------------------------------------------------------------------------------
    @staticmethod
    def samples(res: int, a: float, b: float):
        """network/utility.py:129-149 in the float32 coordinates every implementation feeds its decoder (the lattice is an INPUT: the
        float32 rounding of the sample positions is part of the operation, not of its error), minus the 0.5 of map.py:645-646."""
        f = np.float32
        idx = np.arange(res ** 3, dtype=np.int64)
        vs, a32 = f((b - a) / (res - 1)), f(a)
        s = np.stack([(idx // (res * res)).astype(f) * vs + a32, ((idx // res) % res).astype(f) * vs + a32, (idx % res).astype(f) * vs + a32], axis=1)
        return (s.astype(f) - f(0.5)).astype(f).astype(F64)

    @staticmethod
    def upsample(low, R: int):
        """trilinear, align_corners=True (map.py:658-663): (B,l,l,l) -> (B,R,R,R) in float64."""
        l = low.shape[1]
        src = np.arange(R, dtype=F64) * ((l - 1) / (R - 1))
        i0 = np.minimum(np.floor(src).astype(np.int64), l - 1)
        i1 = np.minimum(i0 + 1, l - 1)
        w1 = src - i0
        out = low
        for axis in (3, 2, 1):
            shp = [1] * 4
            shp[axis] = R
            out = np.take(out, i0, axis=axis) * (1.0 - w1).reshape(shp) + np.take(out, i1, axis=axis) * w1.reshape(shp)
        return out

    def lattice_cubes(self, latents, r: int, fast: bool = True):
        """The cube values of extract_mesh (map.py:640-687) for the voxels whose latents are `latents` (B,29).
        -> dict(cube_sdf (B,2r,2r,2r) NEGATED as stored, cube_std, low_sdf / low_std (the first pass, un-negated), margin (B,(2r)^3):
        |(|interpolated sdf| - 0.05)| per sample (inf when not fast), refine (B,(2r)^3) bool: re-decoded samples)."""
        lat = np.asarray(latents, dtype=F64)
        B, R = lat.shape[0], 2 * r
        a, b = -(r // 2) * (1. / r), 1. + (r - 1) // 2 * (1. / r)
        lr = r if fast else R
        low = self.samples(lr, a, b)
        x = np.concatenate([np.repeat(lat, lr ** 3, axis=0), np.tile(low, (B, 1))], axis=1)
        sdf, std, _, _ = self.decoder(x)
        low_sdf, low_std = sdf.reshape(B, lr, lr, lr), std.reshape(B, lr, lr, lr)
        if not fast:
            return dict(cube_sdf=-low_sdf, cube_std=low_std, low_sdf=low_sdf, low_std=low_std,
                        margin=np.full((B, R ** 3), np.inf), refine=np.zeros((B, R ** 3), dtype=bool))
        hs, hd = self.upsample(low_sdf, R).reshape(B, R ** 3), self.upsample(low_std, R).reshape(B, R ** 3)
        margin = np.abs(np.abs(hs) - REFINE_TH)
        refine = np.abs(hs) < REFINE_TH
        bi, si = np.where(refine)
        if bi.size:
            high = self.samples(R, a, b)
            v_sdf, v_std, _, _ = self.decoder(np.concatenate([lat[bi], high[si]], axis=1))
            hs[bi, si], hd[bi, si] = v_sdf, v_std
        return dict(cube_sdf=-hs.reshape(B, R, R, R), cube_std=hd.reshape(B, R, R, R), low_sdf=low_sdf, low_std=low_std, margin=margin, refine=refine)
