"""Seeded weight sets and input classes for the MLP envelope tests (tests/test_ref64_cpu.py on the CPU, tests/test_gpu_mlp_envelope.py on
the GPU).  TEST INFRASTRUCTURE ONLY; everything here is a deterministic function of its seed.

Weight sets (all of the shipped topology):
  shipped       network/weights_default.npz
  hostile_a/b   random_weights(seed) made hostile: every element of a row scaled by its own power of two over nine binades, ~10 % exact
                zeros (never a whole row: weight norm divides by the row's norm), weight_g of both signs, biases of order 0.3, batch-norm
                statistics with running_mean != 0, running_var from 1e-3 to 10 and gamma of both signs
  <name>+zc     a hostile set with the sdf head's bias moved so that sdf = 0 passes through the seq_small scene (_with_zero_crossing)
  bf16          as hostile, but every FOLDED weight (g * v / |v|, conv * gamma / sqrt(var + eps)) is exactly bf16-representable, so the
                mid and lo slices of the bf16 pipe's weight fragments are zero
"""
from __future__ import annotations

import math

import numpy as np

F32 = np.float32
SCALES = (0.0, 1e-3, 0.3, 1.0, 4.0, 16.0, 64.0)
N_ROWS = 4096
WEIGHT_SETS = ("shipped", "hostile_a", "hostile_b", "bf16")
ENC_LIMIT = 2.0 ** 12          # kernels_integrate.hip.h: DIF_FIX_SCALE assumes |enc| < 2^12


def _bf16(x):
    """float32 -> the nearest bf16 (ties to even), as float32."""
    u = np.ascontiguousarray(x, dtype=F32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(F32).reshape(np.shape(x))


def _is_bf16(x):
    return (np.ascontiguousarray(x, dtype=F32).view(np.uint32) & 0xFFFF) == 0


def _hostile_matrix(g, o, k):
    """(o,k) float32: N(0,1) entries times 2^[-4, 4] each, ~10 % exact zeros, no all-zero row."""
    v = g.standard_normal((o, k)) * np.exp2(g.integers(-4, 5, size=(o, k)))
    z = g.random((o, k)) < 0.10
    z[np.arange(o), g.integers(0, k, size=o)] = False
    return np.where(z, 0.0, v).astype(F32)


def hostile_weights(seed: int, bf16: bool = False):
    from di_fusion_amd.network.utility import random_weights
    raw = random_weights(seed)
    g = np.random.default_rng(1000 + seed)
    for i in range(5):
        o, k = raw[f"decoder.lin{i}.weight_v"].shape
        # |g| around sqrt(2): with unit-direction rows that keeps the activation scale from layer to layer behind a ReLU
        gain = (g.uniform(0.7, 2.0, size=(o, 1)) * g.choice([-1.0, 1.0], size=(o, 1))).astype(F32)
        if i == 4:
            gain = np.full((1, 1), -1.5, dtype=F32)
        v = _hostile_matrix(g, o, k)
        if bf16:
            # folded W = v * (g / |v|) must be bf16: v = bf16(direction * |g|), g = +-fl32(|v|); rows whose quotient does not round back to v
            # are redrawn
            for r in range(o):
                for _ in range(200):
                    v[r] = _bf16(v[r] / np.linalg.norm(v[r].astype(np.float64)) * abs(gain[r, 0]))
                    nrm = np.linalg.norm(v[r].astype(np.float64))
                    gr = F32(math.copysign(1.0, gain[r, 0]) * F32(nrm))
                    w = (v[r].astype(np.float64) * (np.float64(gr) / nrm)).astype(F32)
                    if _is_bf16(w).all() and np.count_nonzero(v[r]):
                        gain[r, 0] = gr
                        break
                    v[r] = _hostile_matrix(g, 1, k)[0]
                else:
                    raise AssertionError("no bf16-exact row found")
        raw[f"decoder.lin{i}.weight_v"] = v
        raw[f"decoder.lin{i}.weight_g"] = gain.astype(F32)
        raw[f"decoder.lin{i}.bias"] = (g.standard_normal(o) * 0.3).astype(F32)
    u = _hostile_matrix(g, 1, 128) * F32(0.25)
    raw["decoder.uncertainty_layer.weight"] = _bf16(u) if bf16 else u
    raw["decoder.uncertainty_layer.bias"] = np.array([0.3], dtype=F32)
    feats = [6, 32, 64, 256]
    for i in range(3):
        p = f"encoder.mlp.layer{i}."
        o, k = feats[i + 1], feats[i]
        W = _hostile_matrix(g, o, k)
        W = (W / np.linalg.norm(W, axis=1, keepdims=True) * math.sqrt(2.0)).astype(F32)
        var = np.exp(g.uniform(math.log(1e-3), math.log(10.0), size=o)).astype(F32)
        gamma = (np.sqrt(var.astype(np.float64) + 1e-5) * g.uniform(0.5, 1.5, size=o) * g.choice([-1.0, 1.0], size=o)).astype(F32)
        if bf16:
            W = _bf16(W)
            for c in range(o):
                for _ in range(200):
                    s = np.float64(var[c]) + 1e-5
                    gc = F32(math.copysign(1.0, gamma[c]) * F32(math.sqrt(s)))
                    if _is_bf16((W[c].astype(np.float64) * (np.float64(gc) / math.sqrt(s))).astype(F32)).all():
                        gamma[c] = gc
                        break
                    var[c] = F32(math.exp(g.uniform(math.log(1e-3), math.log(10.0))))
                else:
                    raise AssertionError("no bf16-exact channel found")
        raw[p + "conv.weight"] = W[:, :, None]
        raw[p + "normlayer.bn.weight"] = gamma
        raw[p + "normlayer.bn.bias"] = (g.standard_normal(o) * 0.3).astype(F32)
        raw[p + "normlayer.bn.running_mean"] = (g.standard_normal(o) * 0.3).astype(F32)
        raw[p + "normlayer.bn.running_var"] = var
    W = (_hostile_matrix(g, 29, 256) / F32(64.0)).astype(F32)
    raw["encoder.mlp.layer3.conv.weight"] = (_bf16(W) if bf16 else W)[:, :, None]
    raw["encoder.mlp.layer3.conv.bias"] = (g.standard_normal(29) * 0.3).astype(F32)
    return raw


_CACHE = {}


def _with_zero_crossing(raw):
    """`raw` with the bias of the sdf head moved so that the surface sdf = 0 passes through seq_small's map: a random decoder keeps one
    sign over the whole scene (no refinement rows, no triangles), which would leave a whole-path run with nothing behind the lattice.
    The shift is minus the median of the float64 sdf pre-activation over the r = 4 lattice of the voxels seq_small occupies (the encoder,
    hence the latents, does not depend on it)."""
    from oracle import difusion_oracle as O
    from .ref64 import Ref64
    om, _ = seq_small_oracle_map(O.OracleNetworks(raw))
    n = om.n_occupied
    ref = Ref64(raw)
    low = ref.samples(4, -0.5, 1.25)
    x = np.concatenate([np.repeat(om.latent_vecs[:n].astype(np.float64), 64, axis=0), np.tile(low, (n, 1))], axis=1)
    out = dict(raw)
    out["decoder.lin4.bias"] = (raw["decoder.lin4.bias"].astype(np.float64) - np.median(ref.decoder(x)[2])).astype(F32)
    return out


def weight_set(name: str):
    if name not in _CACHE:
        if name.endswith("+zc"):
            _CACHE[name] = _with_zero_crossing(weight_set(name[:-3]))
        elif name == "shipped":
            from di_fusion_amd.network.utility import load_weights_npz
            _CACHE[name] = load_weights_npz()
        else:
            _CACHE[name] = {"hostile_a": lambda: hostile_weights(11), "hostile_b": lambda: hostile_weights(12),
                            "bf16": lambda: hostile_weights(13, bf16=True)}[name]()
    return _CACHE[name]


# ---- decoder rows ---------------------------------------------------------------------------------------------------------------
def _voxel_xyz(g, n):
    return (g.random((n, 3)) - 0.5).astype(F32)


def decoder_rows_scale(s: float, n: int = N_ROWS, seed: int = 0):
    g = np.random.default_rng([seed, int(s * 1000)])
    return np.concatenate([(g.standard_normal((n, 29)) * s).astype(F32), _voxel_xyz(g, n)], axis=1)


def decoder_rows_corners(n: int = N_ROWS, seed: int = 1):
    """xyz exactly at -0.5, 0, +0.5 (every combination), latents N(0, 0.3)."""
    g = np.random.default_rng(seed)
    x = decoder_rows_scale(0.3, n, seed)
    x[:, 29:] = g.choice(np.array([-0.5, 0.0, 0.5], dtype=F32), size=(n, 3))
    return x


def decoder_rows_onehot(n: int = N_ROWS, seed: int = 4):
    """each of the 32 features alone: amplitudes exactly +-1 and +-100, and log-uniform ones between them (n / 32 rows per feature)."""
    g = np.random.default_rng(seed)
    per = n // 32
    amp = np.exp(g.uniform(0.0, math.log(100.0), size=(32, per))) * g.choice([-1.0, 1.0], size=(32, per))
    amp[:, :4] = (1.0, -1.0, 100.0, -100.0)
    x = np.zeros((32, per, 32), dtype=F32)
    x[np.arange(32), :, np.arange(32)] = amp.astype(F32)
    return x.reshape(32 * per, 32)


def decoder_rows_tiny(n: int = N_ROWS, seed: int = 2):
    """-0.0, values of order 1e-30 and subnormals, mixed per element with N(0, 0.3) values."""
    g = np.random.default_rng(seed)
    x = decoder_rows_scale(0.3, n, seed)
    kind = g.integers(0, 5, size=x.shape)
    sign = g.choice(np.array([-1.0, 1.0], dtype=F32), size=x.shape)
    x = np.where(kind == 0, F32(-0.0), x)
    x = np.where(kind == 1, sign * F32(1e-30) * g.random(x.shape).astype(F32), x)
    x = np.where(kind == 2, sign * (g.integers(1, 1 << 23, size=x.shape).astype(np.uint32).view(F32)), x)      # subnormals
    x[: n // 8] = np.where(kind[: n // 8] >= 3, F32(-0.0), F32(0.0))                                          # rows of only +-0
    return x.astype(F32)


PU_BINS = ((10.0, 20.0), (20.0, 88.0), (88.0, 250.0))       # softplus: log1p(exp) below 20, the identity above, and where expf alone would overflow


def decoder_rows_large_pu(ref, n: int = N_ROWS, seed: int = 3):
    """Three cases of n rows whose float64 uncertainty pre-activation pu lies in (10, 20], (20, 88] and (88, 250].  Each bin is a case of
    its own, judged under its own e_ref: the rows above 88 have huge hidden activations and a float32 error to match, which would hide
    a misplaced threshold (0.5 e^-10 ~ 2e-5 on std) if the bins shared one bar.  Random rows
    almost never get there with the shipped weights (about one latent direction in a thousand has pu > 0), so: draw a pool of rows at
    latent scales 16 .. 256, take pu along each row's ray t -> [t * latent | xyz] as linear between t = 0 and t = 1, solve for a target in
    the bin, and then FILTER on the float64 value of the rescaled row: membership is a fact, not a hope."""
    g = np.random.default_rng(seed)
    m = 1 << 13
    while True:
        pool = np.concatenate([(g.standard_normal((m, 29)) * np.exp2(g.uniform(4, 8, size=(m, 1)))).astype(F32), _voxel_xyz(g, m)], axis=1)
        zero = pool.copy()
        zero[:, :29] = 0
        pu1, pu0 = ref.decoder(pool)[3], ref.decoder(zero)[3]
        ok = [(np.abs(pu1 - pu0) > 1.0) & ((0.5 * (lo + hi) - pu0) / (pu1 - pu0) > 0) & ((0.5 * (lo + hi) - pu0) / (pu1 - pu0) < 4) for lo, hi in PU_BINS]
        if min(int(o.sum()) for o in ok) >= 64 or m >= 1 << 18:
            break
        m *= 2
    out = {}
    per = n
    for (lo, hi), o in zip(PU_BINS, ok):
        assert o.sum() >= 16, f"the pool holds too few rows that can reach pu in ({lo}, {hi}]"
        rep = max(1, 2048 // int(o.sum()))
        seeds, a, b = np.tile(pool[o], (rep, 1)), np.tile(pu0[o], rep), np.tile((pu1 - pu0)[o], rep)
        got = np.zeros((0, 32), dtype=F32)
        for _ in range(48):
            target = np.exp(g.uniform(math.log(lo * 1.02), math.log(hi * 0.98), size=seeds.shape[0]))
            cand = seeds.copy()
            cand[:, :29] = (cand[:, :29] * ((target - a) / b)[:, None] * (1.0 + 0.03 * g.standard_normal((seeds.shape[0], 29)))).astype(F32)
            q = ref.decoder(cand)[3]
            got = np.concatenate([got, cand[(q > lo) & (q <= hi)]])
            if got.shape[0] >= per:
                break
        assert got.shape[0] >= per, (lo, hi, got.shape[0])
        out[f"pu({lo:g},{hi:g}]"] = got[:per].copy()
    return out


def decoder_cases(ref):
    """name -> (N,32) float32, every case N_ROWS rows."""
    cases = {f"N(0,{s:g})": decoder_rows_scale(s) for s in SCALES}
    cases["corners"] = decoder_rows_corners()
    cases["onehot"] = decoder_rows_onehot()
    cases["tiny"] = decoder_rows_tiny()
    cases.update(decoder_rows_large_pu(ref))
    return cases


# ---- encoder rows ---------------------------------------------------------------------------------------------------------------
ENC_SCALES = (0.0, 1e-3, 0.3, 1.0, 4.0, 16.0)


def encoder_cases():
    """name -> (N,6) float32 = [point relative to the voxel | normal]: points in the voxel with unit normals, with non-unit normals, a
    scale sweep of the whole row, and the +-0.5 / 0 positions."""
    g = np.random.default_rng(5)
    n = N_ROWS
    nrm = g.standard_normal((n, 3))
    unit = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(F32)
    cases = {"unit": np.concatenate([_voxel_xyz(g, n), unit], axis=1),
             "nonunit": np.concatenate([_voxel_xyz(g, n), (unit * np.exp2(g.uniform(-6, 3, size=(n, 1)))).astype(F32)], axis=1)}
    for s in ENC_SCALES:
        cases[f"N(0,{s:g})"] = (g.standard_normal((n, 6)) * s).astype(F32)
    c = cases["unit"].copy()
    c[:, :3] = g.choice(np.array([-0.5, 0.0, 0.5], dtype=F32), size=(n, 3))
    cases["corners"] = c
    t = cases["unit"].copy()
    t[:, :3] = np.where(g.random((n, 3)) < 0.5, F32(-0.0), g.integers(1, 1 << 23, size=(n, 3)).astype(np.uint32).view(F32))
    cases["tiny"] = t
    return cases


# ---- the bar --------------------------------------------------------------------------------------------------------------------
def max_err(got, want):
    """worst |got - want| over the rows (float64); a NaN anywhere is an error of inf."""
    d = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64))
    return float(np.inf) if np.isnan(d).any() else float(d.max())


# K of the bar  e_gpu <= K * e_ref + U ulp : twice the largest ratio between the worst errors (against float64) of three legitimate
# float32 evaluations of the same rows: the oracle (numpy float32, BLAS summation order), torch CPU float32, and strict left-to-right
# float32 accumulation.  Measured over every weight set, case and output by tests/test_ref64_cpu.py::test_k_of_the_bar (which fails if a
# later generator change moves it past the constant); the table is in profiles/mlp_envelope_k.md.
#   largest ratios measured: decoder 3.19 (hostile_b, "pu(88,250]", sdf: 1.69e-4 / 5.3e-5 / 1.70e-4; then 3.14: shipped, "tiny", sdf), encoder 2.95 (hostile_a, "N(0,0)", channels 16-19),
#   gradient 2.75 (shipped, N(0,4): 3.6e-5 oracle, 1.3e-5 torch); twice the largest is 6.4
K_BAR = 6.5
# the ulp errors the HIP math API documents for the device functions of the epilogue: tanhf 1; expf 1 + log1pf 1
U_SDF, U_STD, U_ENC, U_GRAD = 1.0, 2.0, 0.0, 2.0      # gradient: (1 - sdf^2) carries tanhf's error twice
ENC_GROUPS = [slice(4 * i, min(4 * i + 4, 29)) for i in range(8)]      # the encoder's outputs as the D fragment holds them: 4 channels per lane half


def bar(e_ref: float, out_max: float, u: float) -> float:
    return K_BAR * e_ref + u * float(np.spacing(F32(out_max)))


class Bundle:
    """One weight set with its float64 reference, its float32 oracle, its cases and the float64 results of those cases."""

    def __init__(self, name: str):
        from oracle import difusion_oracle as O
        from .ref64 import Ref64
        self.name, self.raw = name, weight_set(name)
        self.ref, self.oracle = Ref64(self.raw), O.OracleNetworks(self.raw)
        self.dec = decoder_cases(self.ref)
        self.enc = encoder_cases()
        self.dec64 = {k: self.ref.decoder(x) for k, x in self.dec.items()}              # sdf, std, ps, pu
        self.enc64 = {k: self.ref.encoder(x) for k, x in self.enc.items()}

    def dec_e_ref(self, case):
        s, d = self.oracle.decoder(self.dec[case])
        return max_err(s[:, 0], self.dec64[case][0]), max_err(d[:, 0], self.dec64[case][1])

    def grad_keep(self, rows):
        """Which rows a gradient check keeps: a row is set aside when one of its hidden pre-activations lies closer to zero than float32
        can tell (the gradient jumps there, and either side is an honest answer).  The margin is not a free constant: per row and layer
        it is K_BAR times the worst error of the float32 oracle's pre-activations of that row and layer against float64: the room the bar
        gives everything else; a unit further than that from its kink cannot honestly take the other side.  -> keep (N,) bool.
        Callers assert that at most 1 % of the rows are set aside."""
        _, pre64 = self.ref._trunk(rows)
        x0 = rows.astype(F32)
        h, keep = x0, np.ones(rows.shape[0], dtype=bool)
        for layer in range(4):
            if layer == 3:
                h = np.concatenate([h, x0], axis=1)
            a32 = (h @ self.oracle.dec_W[layer].T + self.oracle.dec_b[layer]).astype(F32)
            h = np.maximum(a32, F32(0))
            keep &= np.abs(pre64[layer]).min(axis=1) > K_BAR * np.abs(a32 - pre64[layer]).max(axis=1)
        return keep

    def enc_e_ref(self, case):
        o = self.oracle.encoder(self.enc[case])
        return [max_err(o[:, g], self.enc64[case][:, g]) for g in ENC_GROUPS]


# ---- maps with planted latents (point queries, lattice) -----------------------------------------------------------------------
def seq_small_oracle_map(oracle):
    """seq_small's frames (the small fixture of the map tests) through an OracleMap of `oracle` -> (OracleMap, the frames [(xyz, normal)])"""
    from oracle import difusion_oracle as O
    from .conftest import GOLDEN
    from .test_gpu_map import CASES, frame_inputs
    _, cfg, _ = CASES["seq_small"]
    g = np.load(GOLDEN / "seq_small.npz")
    om = O.OracleMap(oracle, cfg.bound_min, cfg.bound_max, cfg.voxel_size)
    frames = [frame_inputs(g, "seq_small", f) for f in range(int(g["n_frames"]))]
    for xyz, nrm in frames:
        om.integrate_keyframe(xyz, nrm)
    return om, frames


def planted_oracle_map(oracle, ws_seed: int, scale: float):
    """seq_small_oracle_map with every latent replaced by N(0, scale) and every count lifted over the decode gate
    -> (OracleMap, n_occupied, the planted latents, the frames)."""
    om, frames = seq_small_oracle_map(oracle)
    n = om.n_occupied
    lat = (np.random.default_rng([ws_seed, int(scale * 10)]).standard_normal((n, 29)) * scale).astype(F32)
    om.latent_vecs[:n] = lat
    om.voxel_obs_count[:n] = 100.0
    return om, n, lat, frames


def query_rows(om, n: int, count: int, seed: int):
    """`count` points uniform inside occupied voxels -> (xyz (count,3) float32, the decoder rows [latent | rel] the way map.py:559-579 forms them)"""
    g = np.random.default_rng(seed)
    pos = om.latent_vecs_pos[:n][g.integers(0, n, size=count)]
    ijk = om._unlinearize_id(pos).astype(np.float64)
    xyz = ((ijk + 0.02 + 0.96 * g.random((count, 3))) * om.voxel_size + np.asarray(om.bound_min, dtype=np.float64)).astype(F32)
    xn, lin = om.voxelize(xyz)
    gid = np.ceil(xn).astype(np.int64) - 1
    slot = om.indexer[lin]
    assert (slot >= 0).all()
    rel = ((xn - gid.astype(F32)).astype(F32) - F32(0.5)).astype(F32)
    return xyz, np.concatenate([om.latent_vecs[slot], rel], axis=1).astype(F32)


QUERY_SCALES = (0.3, 4.0, 16.0)
QUERY_SEED = 31


_BUNDLES = {}


def bundle(name: str) -> Bundle:
    if name not in _BUNDLES:
        _BUNDLES[name] = Bundle(name)
    return _BUNDLES[name]

