"""The MFMA encoder / decoder tiles (csrc/mlp.hip.h) against a float64 reference across their input envelope, on both matrix pipes.

The reference is tests/ref64.py (plain numpy float64, pinned by tests/test_ref64_cpu.py); weight sets and input classes are the seeded
generators of tests/mlp_cases.py: the shipped checkpoint, two hostile sets and one whose folded weights are exactly bf16.

THE BAR.  For a case, e_ref is the worst error of the float32 reference arithmetic (oracle.OracleNetworks, which the goldens pin on the
reference) against float64 over the case's rows and e_gpu the kernel's; required, per output (sdf, std, each group of four latent
channels, gradient):      e_gpu <= K_BAR * e_ref + U ulp of the output.
K_BAR = 6.5 is twice the largest ratio between three honest float32 evaluations of the same rows (BLAS order, torch CPU, strict
left-to-right), measured on the CPU over every case (mlp_cases.K_BAR, profiles/mlp_envelope_k.md); U is what the HIP math API documents
for the device functions of the epilogue (tanhf 1; expf 1 + log1pf 1).  Every test prints e_gpu / e_ref per case.

WHICH EPILOGUE IS REACHED WHERE.  mlp.hip.h writes `sdf = tanhf(ps); sp = pu > 20 ? pu : log1pf(expf(pu))` eight times; the three
"pu(lo,hi]" cases of every weight set hold 4,096 rows each with pu in (10, 20], (20, 88] and above 88 (a bar per bin), the N(0,4) .. N(0,64) cases saturate
tanh, and the planted maps below carry latents of scale 4 and 16 into the map kernels:
  decoder_tile            test_decoder_rows_values[*-f32]                     (k_decode<false>, explicit rows)
  decoder_tile_x6         test_decoder_rows_values[*-bf16x6]                  (k_decode_x6, explicit rows), test_point_queries (values)
  decoder_tile_grad       test_point_queries[*-f32]                           (k_decode<true>: get_sdf_with_gradient)
  decoder_tile_grad_x6    test_point_queries[*-bf16x6]                        (k_decode_grad_x6)
  decoder_tile_folded     test_lattice_cubes[*-f32]                           (k_decode_voxels<false>, refine rows of k_decode)
  decoder_tile_folded_x6  test_lattice_cubes[*-bf16x6]                        (k_decode_voxels<true>, k_decode_refine_x6)
  decoder_tile_nll_grad, decoder_tile_nll_grad_x6: the optimiser's tiles (k_optim_grad): tests/test_gpu_optim_envelope.py (its own per-tile table).
The map tests assert on the float64 values that their planted latents reach pu > 20 and |sdf| > 0.999 (pu > 20: the hostile sets; with
the shipped weights about one latent direction in a thousand has pu > 0, and only the explicit "pu(lo,hi]" rows get there).
test_lattice_rounds walks the lattice kernel's round structure, test_sequence_on_foreign_weights the whole frame path with the hostile sets.
"""
import numpy as np
import pytest
import torch

from di_fusion_amd import _lib
from di_fusion_amd.network import utility as net_util
from tests import mlp_cases as C

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PIPES = ("bf16x6", "f32")
F32 = np.float32
GUARD = 1024                                   # floats kept behind and in front of every output buffer
SENTINEL = 0x7FC0DEAD                          # a NaN whose payload no kernel produces


@pytest.fixture(scope="module")
def nets():
    """One Networks per (weight set, pipe), built on first use."""
    cache = {}

    def get(ws, pipe):
        if (ws, pipe) not in cache:
            cache[ws, pipe] = net_util.networks_from_arrays(C.weight_set(ws), x6=(pipe == "bf16x6"))
        return cache[ws, pipe]
    return get


def _kernel(net, pipe):
    return {("dec", "bf16x6"): "k_decode_x6 / decoder_tile_x6", ("dec", "f32"): "k_decode<false> / decoder_tile",
            ("enc", "bf16x6"): "k_encode_rows<true> / encoder_tile_x6", ("enc", "f32"): "k_encode_rows<false> / encoder_tile"}[net, pipe]


def _guarded(n_floats):
    buf = torch.full((n_floats + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)
    return buf, buf[GUARD:GUARD + n_floats]


def _guards_intact(buf):
    b = buf.view(torch.int32)
    return bool((b[:GUARD] == SENTINEL).all() and (b[-GUARD:] == SENTINEL).all())


def gpu_decode(model, x: np.ndarray):
    """dif_decode_rows into guarded buffers -> sdf (N,), std (N,) float32 numpy; asserts that nothing outside [0, N) was written."""
    n = x.shape[0]
    rows = torch.from_numpy(np.ascontiguousarray(x, dtype=F32)).to(DEV)
    bs, sdf = _guarded(n)
    bd, std = _guarded(n)
    w = model.packed.weights_struct(DEV)
    _lib.check(_lib.load().dif_decode_rows(w, _lib.ptr(rows), n, _lib.ptr(sdf), _lib.ptr(std), _lib.stream_ptr()), "dif_decode_rows")
    torch.cuda.synchronize()
    assert _guards_intact(bs) and _guards_intact(bd), "dif_decode_rows wrote outside its output rows"
    return sdf.cpu().numpy(), std.cpu().numpy()


def gpu_encode(model, x: np.ndarray):
    n = x.shape[0]
    rows = torch.from_numpy(np.ascontiguousarray(x, dtype=F32)).to(DEV)
    bo, out = _guarded(n * 29)
    w = model.packed.weights_struct(DEV)
    _lib.check(_lib.load().dif_encode_rows(w, _lib.ptr(rows), n, _lib.ptr(out), _lib.stream_ptr()), "dif_encode_rows")
    torch.cuda.synchronize()
    assert _guards_intact(bo), "dif_encode_rows wrote outside its output rows"
    return out.cpu().numpy().reshape(n, 29)


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _judge(label, out, e_gpu, e_ref, out_max, u, fails):
    limit = C.bar(e_ref, out_max, u)
    ok = e_gpu <= limit
    print(f"  {label:44s} {out:14s} e_gpu {e_gpu:.3e}  e_ref {e_ref:.3e}  e_gpu/e_ref {e_gpu / max(e_ref, 1e-300):6.2f}  bar {limit:.3e}{'' if ok else '   <-- OVER THE BAR'}")
    if not ok:
        fails.append(f"{label} {out}: e_gpu {e_gpu:.3e} > {limit:.3e} (e_ref {e_ref:.3e})")


# ---- explicit rows: values ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipe", PIPES)
@pytest.mark.parametrize("ws", C.WEIGHT_SETS)
def test_decoder_rows_values(ws, pipe, nets):
    b, model, fails = C.bundle(ws), nets(ws, pipe), []
    for case, x in b.dec.items():
        sdf, std = gpu_decode(model, x)
        r_sdf, r_std = b.dec64[case][0], b.dec64[case][1]
        e_sdf, e_std = b.dec_e_ref(case)
        label = f"{ws}/{pipe}/{case} [{_kernel('dec', pipe)}]"
        _judge(label, "sdf", C.max_err(sdf, r_sdf), e_sdf, np.abs(r_sdf).max(), C.U_SDF, fails)
        _judge(label, "std", C.max_err(std, r_std), e_std, np.abs(r_std).max(), C.U_STD, fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("pipe", PIPES)
@pytest.mark.parametrize("ws", C.WEIGHT_SETS)
def test_encoder_rows_values(ws, pipe, nets):
    b, model, fails = C.bundle(ws), nets(ws, pipe), []
    for case, x in b.enc.items():
        out, want, e_ref = gpu_encode(model, x), b.enc64[case], b.enc_e_ref(case)
        label = f"{ws}/{pipe}/{case} [{_kernel('enc', pipe)}]"
        for gi, g in enumerate(C.ENC_GROUPS):
            _judge(label, f"ch{4 * gi}-{g.stop - 1}", C.max_err(out[:, g], want[:, g]), e_ref[gi], np.abs(want[:, g]).max(), C.U_ENC, fails)
    assert not fails, "\n".join(fails)


# ---- explicit rows: shape -------------------------------------------------------------------------------------------------------
# dif_decode_rows / dif_encode_rows cap their grid at the CU count with 8 waves of 32 rows per workgroup: past (CUs * 256) rows a wave
# walks several tiles.  300,001 = 9,375 full tiles + 1 row is past that cap on any part with fewer than 1,172 CUs.
SHAPES = (1, 31, 32, 33, 255, 256, 257, 65535, 65536, 65537, 300001)


@pytest.mark.parametrize("pipe", PIPES)
def test_rows_shape(pipe, nets):
    """Every N: each output row equals, bit for bit, the same row's output in the 4,096-row launch that test_*_rows_values holds under
    the bar (rows repeat cyclically, so row i of any launch is base row i mod 4,096), and the guard bands come back untouched."""
    model, b = nets("shipped", pipe), C.bundle("shipped")
    assert 300001 > torch.cuda.get_device_properties(0).multi_processor_count * 256
    xd, xe = b.dec["N(0,1)"], b.enc["N(0,1)"]
    base_sdf, base_std = gpu_decode(model, xd)
    base_enc = gpu_encode(model, xe)
    for n in SHAPES:
        idx = np.arange(n) % C.N_ROWS
        sdf, std = gpu_decode(model, xd[idx])
        enc = gpu_encode(model, xe[idx])
        bad = np.nonzero((bits(sdf) != bits(base_sdf[idx])) | (bits(std) != bits(base_std[idx])))[0]
        assert bad.size == 0, f"N={n} [{_kernel('dec', pipe)}]: {bad.size} rows differ from the base launch, first {bad[:5]}"
        bad = np.nonzero((bits(enc) != bits(base_enc[idx])).any(axis=1))[0]
        assert bad.size == 0, f"N={n} [{_kernel('enc', pipe)}]: {bad.size} rows differ from the base launch, first {bad[:5]}"


# ---- explicit rows: position independence ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipe", PIPES)
@pytest.mark.parametrize("ws", ("shipped", "hostile_a"))
def test_rows_position_independence(ws, pipe, nets):
    """The arithmetic of a row does not depend on its lane, wave, workgroup or grid-stride step: no tolerance."""
    model, b = nets(ws, pipe), C.bundle(ws)
    g = np.random.default_rng(21)
    for case in ("N(0,0.3)", "N(0,16)", "pu(10,20]", "pu(88,250]"):
        x = b.dec[case]
        perm = g.permutation(x.shape[0])
        sdf, std = gpu_decode(model, x)
        psdf, pstd = gpu_decode(model, x[perm])
        assert np.array_equal(bits(psdf), bits(sdf[perm])) and np.array_equal(bits(pstd), bits(std[perm])), (case, _kernel("dec", pipe))
    for case in ("unit", "N(0,4)"):
        x = b.enc[case]
        perm = g.permutation(x.shape[0])
        assert np.array_equal(bits(gpu_encode(model, x[perm])), bits(gpu_encode(model, x)[perm])), (case, _kernel("enc", pipe))
    # one row in every position of a tile, a workgroup and two grid-stride steps
    n = 2 * torch.cuda.get_device_properties(0).multi_processor_count * 256 + 33
    for j in (0, 1777):
        sdf, std = gpu_decode(model, np.repeat(b.dec["N(0,1)"][j:j + 1], n, axis=0))
        assert np.unique(bits(sdf)).size == 1 and np.unique(bits(std)).size == 1, _kernel("dec", pipe)
        enc = gpu_encode(model, np.repeat(b.enc["nonunit"][j:j + 1], n, axis=0))
        assert (bits(enc) == bits(enc[0])).all(), _kernel("enc", pipe)


# ---- explicit rows: non-finite inputs -------------------------------------------------------------------------------------------
def _bad_values():
    return np.array([0x7FC00000, 0xFFC00000, 0x7F800000, 0xFF800000], dtype=np.uint32).view(F32)      # +NaN, -NaN (x86's inf - inf), +inf, -inf


@pytest.mark.parametrize("pipe", PIPES)
@pytest.mark.parametrize("ws", C.WEIGHT_SETS)
def test_rows_non_finite(ws, pipe, nets):
    """+NaN, -NaN (sign bit set: what x86 produces for inf - inf and 0 / 0), +inf and -inf in each feature position, scattered among
    finite rows of the same tiles.  (a) every finite row comes out bit for bit as in the run without the bad rows; (b) a bad row comes
    out as the float64 reference has it (NaN wherever the reference is NaN) — not as a finite, plausible value."""
    model, b = nets(ws, pipe), C.bundle(ws)
    vals = _bad_values()
    for net, x, width, run, ref in (("dec", b.dec["N(0,1)"], 32, lambda m, x: np.stack(gpu_decode(m, x), axis=1), lambda x: np.stack(b.ref.decoder(x)[:2], axis=1)),
                                    ("enc", b.enc["unit"], 6, gpu_encode, b.ref.encoder)):
        clean = run(model, x)
        dirty_x = x.copy()
        where = 5 + 29 * np.arange(4 * width)                  # 29 is odd: every lane position of a tile gets its turn
        for j, row in enumerate(where):
            dirty_x[row, j % width] = vals[j // width]
        dirty = run(model, dirty_x)
        finite = np.ones(x.shape[0], dtype=bool)
        finite[where] = False
        assert np.array_equal(bits(dirty[finite]), bits(clean[finite])), f"[{_kernel(net, pipe)}] a non-finite row changed a finite row of its launch"
        want = ref(dirty_x[where])
        got = dirty[where]
        lost = np.isnan(want) & ~np.isnan(got)
        names = ["+NaN", "-NaN", "+inf", "-inf"]
        report = [f"{names[j // width]} in feature {j % width} -> {got[j][:2]}" for j in np.nonzero(lost.any(axis=1))[0]]
        print(f"  {ws}/{pipe}/{net}: {len(report)} of {len(where)} non-finite rows came out finite")
        assert not report, f"[{_kernel(net, pipe)}] the float64 reference gives NaN, the kernel a finite value: " + "; ".join(report[:6])
        both = ~np.isnan(want)
        assert np.allclose(got[both], want[both], rtol=1e-5, atol=1e-5, equal_nan=True)


# ---- point queries --------------------------------------------------------------------------------------------------------------
from tests.test_gpu_map import CASES, run_sequence  # noqa: E402  (seq_small: the small fixture of the map tests)
SEQ = CASES["seq_small"]


def _planted_map(model, oracle, ws_seed, scale):
    """seq_small's frames through `model`, then every latent replaced by N(0, scale) (as test_decode_of_reference_latents_within_1e5
    replaces them by the reference's) and every count lifted over the decode gate -> (map, OracleMap with the same state, n_occupied)."""
    from di_fusion_amd.system.map import DenseIndexedMap
    om, n, lat, frames = C.planted_oracle_map(oracle, ws_seed, scale)
    m = DenseIndexedMap(model, SEQ[1].namespace(), 29, DEV, initial_capacity=1024)
    for xyz, nrm in frames:
        m.integrate_keyframe(torch.from_numpy(xyz).to(DEV), torch.from_numpy(nrm).to(DEV))
    assert n == m.n_occupied and np.array_equal(m.latent_vecs_pos[:n].cpu().numpy(), om.latent_vecs_pos[:n])
    m._latent[:n] = torch.from_numpy(lat).to(DEV)
    m._obs[:n] = 100.0
    return m, om, n


_query_rows = C.query_rows


@pytest.mark.parametrize("pipe", PIPES)
@pytest.mark.parametrize("ws", C.WEIGHT_SETS)
def test_point_queries(ws, pipe, nets):
    """get_sdf (forward-only tile) and get_sdf_with_gradient (the reverse chain) on maps with planted latents of scale 0.3, 4 and 16.
    Gradient: against ref64.decoder_xyz_grad / voxel_size.  The gradient is discontinuous where a hidden pre-activation changes sign, and
    a float32 evaluation cannot decide a sign inside its own error: points with a pre-activation closer to zero than
    mlp_cases.Bundle.grad_keep's margin (K_BAR times the oracle's own pre-activation error, per row and layer) are set aside, at most 1 % of them.
    Not only the first layer: with the hostile_b weights and latents N(0, 0.3) one query of 4,096 has a layer-2 pre-activation at
    9e-9 of its row's largest (float32 resolves 6e-8); both pipes take the other side there and land 4.1e-2 from the float64 gradient."""
    b, model, fails = C.bundle(ws), nets(ws, pipe), []
    reach = dict(pu20=0.0, sat=0.0)
    for scale in C.QUERY_SCALES:
        m, om, n = _planted_map(model, b.oracle, C.WEIGHT_SETS.index(ws), scale)
        xyz, rows = _query_rows(om, n, C.N_ROWS, C.QUERY_SEED)
        r_sdf, r_std, r_grad = b.ref.decoder_xyz_grad(rows)
        pu = b.ref.decoder(rows)[3]
        reach["pu20"], reach["sat"] = max(reach["pu20"], (pu > 20).mean()), max(reach["sat"], (np.abs(r_sdf) > 0.999).mean())
        o_sdf, o_std, o_grad = b.oracle.decoder_xyz_grad(rows)
        keep = b.grad_keep(rows)
        assert (~keep).mean() <= 0.01, f"the query set puts {(~keep).mean():.2%} of its points on a ReLU kink of some hidden layer"
        q = torch.from_numpy(xyz).to(DEV)
        sdf, std, mask = m.get_sdf(q)
        assert bool(mask.all())
        label = f"{ws}/{pipe}/queries N(0,{scale:g})"
        fwd = "k_decode_x6 / decoder_tile_x6" if pipe == "bf16x6" else "k_decode<false> / decoder_tile"
        _judge(f"{label} [{fwd}]", "sdf", C.max_err(sdf.cpu().numpy(), r_sdf), C.max_err(o_sdf, r_sdf), 1.0, C.U_SDF, fails)
        _judge(f"{label} [{fwd}]", "std", C.max_err(std.cpu().numpy(), r_std), C.max_err(o_std, r_std), np.abs(r_std).max(), C.U_STD, fails)
        s2, d2, m2, g2 = m.get_sdf_with_gradient(q)
        assert bool(m2.all())
        bwd = "k_decode_grad_x6 / decoder_tile_grad_x6" if pipe == "bf16x6" else "k_decode<true> / decoder_tile_grad"
        vs = om.voxel_size
        _judge(f"{label} [{bwd}]", "sdf", C.max_err(s2.cpu().numpy(), r_sdf), C.max_err(o_sdf, r_sdf), 1.0, C.U_SDF, fails)
        _judge(f"{label} [{bwd}]", "std", C.max_err(d2.cpu().numpy(), r_std), C.max_err(o_std, r_std), np.abs(r_std).max(), C.U_STD, fails)
        _judge(f"{label} [{bwd}]", "d sdf / d xyz", C.max_err(g2.cpu().numpy()[keep], r_grad[keep] / vs), C.max_err(o_grad[keep] / F32(vs), r_grad[keep] / vs),
               np.abs(r_grad[keep]).max() / vs, C.U_GRAD, fails)
    assert ws == "shipped" or reach["pu20"] >= 0.01, reach          # (the shipped weights reach pu > 20 on explicit rows only: the "pu(lo,hi]" cases)
    assert reach["sat"] >= 0.01, reach
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("pipe", PIPES)
def test_point_queries_past_the_grid_cap(pipe, nets):
    """The query kernels cap their grid at the CU count too: 8 waves per workgroup forward-only, 4 in the gradient kernels (256 threads),
    32 points per wave.  The 4,096 query points repeated cyclically past three grid-stride steps of either, with a ragged tail: every
    output equals, bit for bit, the same point's output in the 4,096-point call that test_point_queries holds under the bar."""
    b, model = C.bundle("shipped"), nets("shipped", pipe)
    m, om, n = _planted_map(model, b.oracle, 0, 4.0)
    xyz, _ = _query_rows(om, n, C.N_ROWS, C.QUERY_SEED)
    big = 3 * torch.cuda.get_device_properties(0).multi_processor_count * 256 + 17
    idx = np.arange(big) % C.N_ROWS
    q, qbig = torch.from_numpy(xyz).to(DEV), torch.from_numpy(xyz[idx]).to(DEV)
    sdf, std, mask = m.get_sdf(q)
    s2, d2, m2, g2 = m.get_sdf_with_gradient(q)
    bsdf, bstd, bmask = m.get_sdf(qbig)
    bs2, bd2, bm2, bg2 = m.get_sdf_with_gradient(qbig)
    assert bool(mask.all()) and bool(bmask.all()) and bool(m2.all()) and bool(bm2.all())
    tidx = torch.from_numpy(idx).to(DEV)
    assert torch.equal(bsdf.view(torch.int32), sdf[tidx].view(torch.int32)) and torch.equal(bstd.view(torch.int32), std[tidx].view(torch.int32))
    assert torch.equal(bs2.view(torch.int32), s2[tidx].view(torch.int32)) and torch.equal(bd2.view(torch.int32), d2[tidx].view(torch.int32))
    assert torch.equal(bg2.contiguous().view(torch.int32), g2[tidx].contiguous().view(torch.int32))


# ---- lattice decode and refine --------------------------------------------------------------------------------------------------
def _check_cubes(m, om, b, pipe, r, fast, label, fails):
    """One extract of map `m` against ref64.lattice_cubes on `om`'s latents (the two maps hold the same state)."""
    m.extract_mesh_arrays(r, int(4e6), fast=fast, max_std=0.15, no_cache=True, to_host=False)
    oa = om.extract_prepare(r, fast=fast, no_cache=True)
    B = m.last_counters["B"]
    tens = m._xbuf[1]
    slots = tens["occ_slot"][:B].cpu().numpy()
    assert B == len(oa["occupied_vec_id"]) and np.array_equal(slots, oa["occupied_vec_id"])
    want = b.ref.lattice_cubes(om.latent_vecs[slots], r, fast)
    cs, cd = tens["cube_sdf"][:B].cpu().numpy(), tens["cube_std"][:B].cpu().numpy()
    assert cs.shape == want["cube_sdf"].shape                       # stored negated, 2r samples per axis (map.py:640-687)
    folded = "decoder_tile_folded_x6" if pipe == "bf16x6" else "decoder_tile_folded"
    label = f"{label} B={B} r={r} fast={fast} [{folded if fast else _kernel('dec', pipe).split(' / ')[1]}]"
    aside = np.zeros(cs.shape, dtype=bool)
    if fast:
        # what decides a flip is the error of the LOW lattice's values: e_ref of those, from the float32 oracle on the same rows
        low = b.ref.samples(r, -(r // 2) * (1. / r), 1. + (r - 1) // 2 * (1. / r))
        x = np.concatenate([np.repeat(om.latent_vecs[slots], r ** 3, axis=0), np.tile(low, (B, 1)).astype(F32)], axis=1)
        margin = C.bar(C.max_err(b.oracle.decoder(x)[0][:, 0], want["low_sdf"].reshape(-1)), 1.0, C.U_SDF)
        aside = (want["margin"] < margin).reshape(cs.shape)
        assert aside.mean() <= 0.005, (label, aside.mean(), margin)
        vh, vh64 = m.last_counters["VH"], int(want["refine"].sum())
        assert abs(vh - vh64) <= int(aside.sum()), (label, vh, vh64, int(aside.sum()))
    keep = ~aside
    o_flip = np.zeros(cs.shape, dtype=bool).reshape(B, -1)
    if len(oa["near_threshold"]):
        o_flip[oa["near_threshold"][:, 0], oa["near_threshold"][:, 1]] = True
    ok = keep & ~o_flip.reshape(cs.shape)                           # e_ref: the oracle's own flips (its 1e-5 band) do not count against it
    e_sdf, e_std = C.max_err(oa["cube_sdf"][ok], want["cube_sdf"][ok]), C.max_err(oa["cube_std"][ok], want["cube_std"][ok])
    _judge(label, "cube_sdf", C.max_err(cs[keep], want["cube_sdf"][keep]), e_sdf, 1.0, C.U_SDF, fails)
    _judge(label, "cube_std", C.max_err(cd[keep], want["cube_std"][keep]), e_std, np.abs(want["cube_std"]).max(), C.U_STD, fails)
    print(f"      set aside {int(aside.sum())} of {aside.size} samples; VH {m.last_counters['VH']} (float64 {int(want['refine'].sum())})")
    return want


@pytest.mark.parametrize("pipe", PIPES)
@pytest.mark.parametrize("ws", C.WEIGHT_SETS)
def test_lattice_cubes(ws, pipe, nets):
    """extract_mesh_arrays at r in {2, 4, 8}, fast on and off, on maps with planted latents (scales 0.3 and 4): cube_sdf / cube_std against
    ref64.lattice_cubes.  A sample whose interpolated |sdf| lies within the case's own bar (K_BAR * e_ref of the low-lattice values + 1
    ulp) of 0.05 in float64 may flip between interpolated and re-decoded: set aside and counted, at most 0.5 % of the samples; VH (rows
    refined) equals the float64 count to within that number."""
    b, model, fails = C.bundle(ws), nets(ws, pipe), []
    reach = dict(pu20=0.0, sat=0.0, refined=0)
    for scale in (0.3, 4.0):
        m, om, n = _planted_map(model, b.oracle, C.WEIGHT_SETS.index(ws), scale)
        for r, fast in ((2, True), (2, False), (4, True), (4, False), (8, True), (8, False)):
            want = _check_cubes(m, om, b, pipe, r, fast, f"{ws}/{pipe}/lattice N(0,{scale:g})", fails)
            reach["pu20"] = max(reach["pu20"], float((want["cube_std"] > 0.05 + 0.5 * 20).mean()))
            reach["sat"] = max(reach["sat"], float((np.abs(want["cube_sdf"]) > 0.999).mean()))
            reach["refined"] += int(want["refine"].sum())
    print(f"  {ws}/{pipe}: reached {reach}")
    assert reach["sat"] >= 0.01 and reach["refined"] > 0, reach
    assert ws == "shipped" or reach["pu20"] >= 0.01, reach          # (the shipped weights reach pu > 20 on explicit rows only: the "pu(lo,hi]" cases)
    assert not fails, "\n".join(fails)


def _allocated_map(model, oracle, n_voxels, scale, seed):
    """A 16^3 map with exactly `n_voxels` voxels allocated (allocate_block, map.py:310-319), latents N(0, scale) and counts planted:
    with no_cache every allocated voxel is decoded, so the batch size B of the lattice kernel is n_voxels."""
    from di_fusion_amd.system.map import DenseIndexedMap
    from oracle import difusion_oracle as O
    _, cfg, _ = CASES["seq_room16"]
    g = np.random.default_rng([seed, n_voxels])
    m = DenseIndexedMap(model, cfg.namespace(), 29, DEV, initial_capacity=1024)
    om = O.OracleMap(oracle, cfg.bound_min, cfg.bound_max, cfg.voxel_size)
    ids = np.sort(g.choice(int(np.prod(om.n_xyz)), size=n_voxels, replace=False)).astype(np.int64)
    m.allocate_block(torch.from_numpy(ids).to(DEV))
    om.allocate_block(ids)
    assert m.n_occupied == om.n_occupied == n_voxels and np.array_equal(m.latent_vecs_pos[:n_voxels].cpu().numpy(), om.latent_vecs_pos[:n_voxels])
    lat = (g.standard_normal((n_voxels, 29)) * scale).astype(F32)
    m._latent[:n_voxels] = torch.from_numpy(lat).to(DEV)
    om.latent_vecs[:n_voxels] = lat
    m._obs[:n_voxels] = 100.0
    om.voxel_obs_count[:n_voxels] = 100.0
    return m, om


@pytest.mark.parametrize("pipe", PIPES)
@pytest.mark.parametrize("ws", ("shipped", "hostile_a"))
def test_lattice_rounds(ws, pipe, nets):
    """The round structure of k_decode_voxels: a launch of min(ceil(max_voxels / 4), CUs) workgroups deals one voxel to each of its four
    wave pairs per round (decode_voxels_body), so one full round is 4 * CUs voxels.  B = 1, a handful, and just below, at and just above
    one full round."""
    b, model, fails = C.bundle(ws), nets(ws, pipe), []
    full = 4 * torch.cuda.get_device_properties(0).multi_processor_count
    assert full + 1 <= 16 ** 3
    for n_voxels in (1, 5, full - 1, full, full + 1):
        m, om = _allocated_map(model, b.oracle, n_voxels, 1.0, C.WEIGHT_SETS.index(ws))
        _check_cubes(m, om, b, pipe, 4, True, f"{ws}/{pipe}/rounds", fails)
        assert m.last_counters["B"] == n_voxels
    assert not fails, "\n".join(fails)


# ---- the whole path on foreign weights ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipe", PIPES)
@pytest.mark.parametrize("ws", ("hostile_a+zc", "hostile_b+zc", "bf16+zc"))
def test_sequence_on_foreign_weights(ws, pipe, nets):
    """seq_small's frames (integrate, extract, marching cubes, get_sdf) with another model: test_gpu_map's sequence test against
    OracleMap(OracleNetworks(weight set)): integer state bit for bit, latents, cubes and triangles under that test's own bars.  The
    "+zc" sets are the hostile ones with the sdf head's bias moved so that the surface passes through the scene (a random decoder keeps
    one sign everywhere: no refinement rows, no triangles); every frame refines more than a thousand rows and all but one frame mesh."""
    from oracle import difusion_oracle as O
    run_sequence("seq_small", nets(ws, pipe), O.OracleNetworks(C.weight_set(ws)), golden=False)
