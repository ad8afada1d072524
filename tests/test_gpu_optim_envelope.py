"""The latent optimiser (dif_optimize_latents: csrc/kernels_optimize.hip.h and the two nll tiles of csrc/mlp.hip.h) against a float64
reference, step by step, on both matrix pipes.

The reference is tests/ref64.py (Ref64.decoder_nll_grad, adam_update64, code_reg_grad64; pinned by tests/test_ref64_cpu.py against float64
autograd and torch.optim.Adam); maps, the NumPy restatement of the gather, the cases and THE BAR are in tests/optim_cases.py.  The calls go
through ctypes on planted 16^3 maps; the optimiser's state (rows, voxel list, z, m, v) is read through dif_test_optimize_views.

After n_iters = 1 the workspace holds m = (1 - 0.9f) * g and v = ((1 - 0.999f) * g) * g: the per-voxel gradient g is read back to one ulp.

WHICH TILE IS REACHED WHERE (every test prints e_gpu / e_ref per case):
  decoder_tile_nll_grad_x6   test_*[bf16x6]   (k_optim_grad<true>)
  decoder_tile_nll_grad      test_*[f32]      (k_optim_grad<false>)
  k_optim_focus, the ordered gather, the unique scan (both branches of either scan)        test_gather_bit_for_bit, test_no_rows_and_second_call
  the epilogue (clamps, logf, pu > 20 twice, the two-headed upstream gradient), inv_n       test_one_step_gradient (asserts its reach on float64 values)
  the segmented fixed-point sums, the second grid-stride step                               test_segmented_sums
  k_optim_adam (moments, bias corrections, regulariser), k_optim_writeback, loss_out        test_steps
"""
import ctypes

import numpy as np
import pytest
import torch

from di_fusion_amd import _lib
from di_fusion_amd.network import utility as net_util
from tests import mlp_cases as C
from tests import optim_cases as OC
from tests.ref64 import adam_update64, code_reg_grad64

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PIPES = ("bf16x6", "f32")
F32 = np.float32
GUARD = 1024                                   # 4-byte words kept behind and in front of every buffer the call writes
SENTINEL = 0x7FC0DEAD
# the constants k_optim_adam states, as float32 evaluates them (1 - 0.9f and 1 - 0.999f are exact subtractions)
B1, B2 = float(F32(0.9)), float(F32(0.999))
C1, C2 = float(F32(1) - F32(0.9)), float(F32(1) - F32(0.999))
LR, EPS = float(F32(1e-2)), float(F32(1e-8))
U = 2.0 ** -24                                 # the relative error bound of one correctly rounded float32 operation
LAMBDA = 0.01                                  # tests/golden/seq_optim.npz: code_reg_lambda


@pytest.fixture(scope="module")
def nets():
    cache = {}

    def get(ws, pipe):
        if (ws, pipe) not in cache:
            cache[ws, pipe] = net_util.networks_from_arrays(C.weight_set(ws), x6=(pipe == "bf16x6"))
        return cache[ws, pipe]
    return get


def _kernel(pipe):
    return "k_optim_grad<true> / decoder_tile_nll_grad_x6" if pipe == "bf16x6" else "k_optim_grad<false> / decoder_tile_nll_grad"


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _guarded(n, dtype):
    """n elements of `dtype` with GUARD sentinel words on either side -> (whole buffer as int32, the view)"""
    size = torch.empty((), dtype=dtype).element_size()
    words = (n * size + 3) // 4
    buf = torch.full((words + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
    return buf, buf[GUARD:GUARD + words].view(torch.uint8)[:n * size].view(dtype)


def _guards_intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all() and (buf[-GUARD:] == SENTINEL).all())


class Device:
    """A Planted map on the GPU (every buffer the call writes is guarded) and calls of dif_optimize_latents on it."""

    def __init__(self, pm: OC.Planted, model):
        self.pm, self.model, cap = pm, model, pm.capacity
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        self.indexer, self.pos, self.obs = t(pm.indexer), t(pm.pos), t(pm.obs)
        self.g_lat, self.latent = _guarded(cap * 29, torch.float32)
        self.g_dirty, self.dirty = _guarded(cap, torch.uint8)
        self.g_opt, self.optimized = _guarded(cap, torch.uint8)
        self.g_loss, self.loss = _guarded(64, torch.float32)
        self.latent.copy_(t(pm.latent).reshape(-1))
        self.dirty.zero_()
        self.optimized.copy_(t(pm.optimized))
        self.loss.zero_()
        self.counters = torch.zeros((_lib.C_COUNT,), dtype=torch.int32, device=DEV)
        self.counters[_lib.C_N_OCCUPIED] = pm.n
        m = _lib.DifMap()
        m.nx = m.ny = m.nz = OC.GRID
        m.bound_min = (ctypes.c_float * 3)(*[float(v) for v in pm.bound_min])
        m.voxel_size = float(pm.voxel_size)
        m.prune_min_vox_obs, m.ignore_count_th, m.encoder_count_th, m.capacity = 16, 16.0, OC.ENC_TH, cap
        m.indexer, m.latent_vecs, m.latent_vecs_pos, m.voxel_obs_count = _lib.ptr(self.indexer), _lib.ptr(self.latent), _lib.ptr(self.pos), _lib.ptr(self.obs)
        m.dirty, m.voxel_optimized, m.counters = _lib.ptr(self.dirty), _lib.ptr(self.optimized), _lib.ptr(self.counters)
        self.cmap = m

    def call(self, xyz, normal, mask, noise, n_iters, lam=0.0, with_loss=True):
        """-> a namespace of everything the call left behind, as NumPy arrays"""
        lib, N, cap = _lib.load(), int(xyz.shape[0]), self.pm.capacity
        t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(DEV)
        d_xyz, d_nrm, d_mask = t(xyz, F32), t(normal, F32), t(mask, np.uint8)
        d_noise = torch.zeros((8 * N,), dtype=torch.float32, device=DEV)
        d_noise[:min(8 * N, noise.size)] = t(noise[:8 * N], F32)
        nb = int(lib.dif_optimize_workspace_bytes(N, cap))
        assert nb > 0
        g_ws, ws = _guarded(nb, torch.uint8)
        ws.fill_(0xA5)                                     # stale workspace contents must not matter
        self.loss.zero_()
        w = self.model.packed.weights_struct(DEV)
        _lib.check(lib.dif_optimize_latents(ctypes.byref(self.cmap), ctypes.byref(w), _lib.ptr(d_xyz), _lib.ptr(d_nrm), N, _lib.ptr(d_mask), _lib.ptr(d_noise),
                                            int(n_iters), 1.0e-2, float(lam), _lib.ptr(self.loss) if with_loss else None, _lib.ptr(ws), nb, _lib.stream_ptr()),
                   "dif_optimize_latents")
        torch.cuda.synchronize()
        for name, buf in (("workspace", g_ws), ("latents", self.g_lat), ("dirty", self.g_dirty), ("voxel_optimized", self.g_opt), ("loss_out", self.g_loss)):
            assert _guards_intact(buf), f"dif_optimize_latents wrote outside its {name}"
        views = _lib.DifOptimizeViews()
        _lib.check(lib.dif_test_optimize_views(N, cap, _lib.ptr(ws), ctypes.byref(views)), "dif_test_optimize_views")

        def view(name, count, dtype):
            off = getattr(views, name) - ws.data_ptr()
            size = torch.empty((), dtype=dtype).element_size()
            assert 0 <= off and off + count * size <= nb, name
            return ws[off:off + count * size].view(dtype).cpu().numpy()

        c = self.counters.cpu().numpy()
        r = type("Result", (), {})()
        r.rows, r.voxels = int(c[_lib.C_OPT_ROWS]), int(c[_lib.C_OPT_VOXELS])
        if n_iters > 0 and N > 0:
            assert 0 <= r.rows <= 8 * N and 0 <= r.voxels <= cap
            r.row_slot, r.row_xyz, r.row_sdf = view("row_slot", r.rows, torch.int32), view("row_xyz", r.rows * 3, torch.float32).reshape(-1, 3), view("row_sdf", r.rows, torch.float32)
            r.uniq_slot, r.slot_u, r.slot_flag = view("uniq_slot", r.voxels, torch.int32), view("slot_u", cap, torch.int32), view("slot_flag", cap, torch.int32)
            r.z, r.m, r.v = (view(k, r.voxels * 32, torch.float32).reshape(-1, 32)[:, :29] for k in ("z", "m", "v"))
        r.latent, r.dirty, r.optimized = self.latent.cpu().numpy().reshape(cap, 29), self.dirty.cpu().numpy(), self.optimized.cpu().numpy()
        r.loss = self.loss.cpu().numpy()
        return r


def _judge(label, out, err, limit, e_ref, fails):
    """err, limit: arrays of one shape; prints the worst element's figures"""
    ratio = err / limit
    j = np.unravel_index(np.argmax(np.where(np.isnan(ratio), np.inf, ratio)), ratio.shape) if ratio.size else ()
    e_gpu = float(np.nan_to_num(err, nan=np.inf).max()) if err.size else 0.0
    ok = bool((err <= limit).all())
    print(f"  {label:58s} {out:10s} e_gpu {e_gpu:.3e}  e_ref {e_ref:.3e}  e_gpu/e_ref {(e_gpu / e_ref) if e_ref > 0 else float('nan'):6.2f}  worst err/bar {float(ratio[j]) if ratio.size else 0.0:5.2f}"
          f"{'' if ok else '   <-- OVER THE BAR'}")
    if not ok:
        fails.append(f"{label} {out}: err {float(err[j]):.3e} > bar {float(limit[j]):.3e} at {j} (e_ref {e_ref:.3e})")


# ---- the gather, bit for bit --------------------------------------------------------------------------------------------------------
def _check_gather(r, pm, xyz, normal, mask, noise, label):
    slot, rxyz, rsdf = OC.gather_rows(pm, xyz, normal, mask, noise)
    assert r.rows == slot.size, (label, r.rows, slot.size)
    assert np.array_equal(r.row_slot, slot), label
    assert np.array_equal(bits(r.row_xyz), bits(rxyz)) and np.array_equal(bits(r.row_sdf), bits(rsdf)), label
    uniq = np.unique(slot)
    assert r.voxels == uniq.size and np.array_equal(r.uniq_slot, uniq), label
    assert np.array_equal(r.slot_u[uniq], np.arange(uniq.size)), label
    return uniq


def _check_bookkeeping(r, pm, uniq, label):
    """voxel_optimized and dirty set exactly for uniq_slot, slot_flag back to 0, no other latent touched"""
    want_opt = pm.optimized.copy()
    want_opt[uniq] = 1
    want_dirty = np.zeros(pm.capacity, dtype=np.uint8)
    want_dirty[uniq] = 1
    assert np.array_equal(r.optimized, want_opt) and np.array_equal(r.dirty, want_dirty), label
    assert not r.slot_flag.any(), label
    other = np.ones(pm.capacity, dtype=bool)
    other[uniq] = False
    assert np.array_equal(bits(r.latent[other]), bits(pm.latent[other])), label
    assert np.array_equal(bits(r.latent[uniq]), bits(r.z)), label


@pytest.mark.parametrize("pipe", PIPES)
def test_gather_bit_for_bit(pipe, nets):
    """row_slot, row_xyz, row_sdf, DIF_C_OPT_ROWS, DIF_C_OPT_VOXELS and uniq_slot (ascending) against optim_cases.gather_rows.
    Isolated voxels with one-octant points give row counts 1 (N = 1), 31, 32, 33; the messy scenes (optim_cases.messy_scene) at N = 1,
    511 and 513 (8 N crosses 4,096: the ordered scan goes from one workgroup to two passes) and 2,000; capacity 1,024 and 8,192 are the
    unique scan's two branches."""
    model = nets("shipped", pipe)
    for capacity in (1024, 8192):
        for n in (1, 31, 32, 33):
            pm, xyz, nrm, mask, noise, _ = OC.isolated_scene(n, capacity, 0)
            r = Device(pm, model).call(xyz, nrm, mask, noise, 1)
            assert r.rows == n
            uniq = _check_gather(r, pm, xyz, nrm, mask, noise, f"isolated N={n} capacity={capacity}")
            _check_bookkeeping(r, pm, uniq, f"isolated N={n}")
        for n in (1, 511, 513, 2000):
            pm, xyz, nrm, mask, noise = OC.messy_scene(n, capacity, 0)
            r = Device(pm, model).call(xyz, nrm, mask, noise, 1)
            uniq = _check_gather(r, pm, xyz, nrm, mask, noise, f"messy N={n} capacity={capacity}")
            _check_bookkeeping(r, pm, uniq, f"messy N={n}")
            assert pm.indexer[0] >= 0 and pm.indexer[0] not in uniq            # lin id 0 is allocated and never optimised
            print(f"  {pipe} messy N={n} capacity={capacity}: {r.rows} rows, {r.voxels} voxels")
            if n >= 511:
                assert r.rows > 0 and 0 < r.voxels < int(pm.in_set().sum()) + 1


@pytest.mark.parametrize("pipe", PIPES)
def test_no_rows_and_second_call(pipe, nets):
    """No rows at all (every voxel optimised before, or every point masked) leaves latents and flags unchanged and loss_out all zero; a
    second call right after a first finds nothing to do."""
    model = nets("shipped", pipe)
    pm, xyz, nrm, mask, noise = OC.messy_scene(513, 1024, 1)
    for what in ("all optimised", "all masked"):
        q = OC.Planted(pm.pos[:pm.n], 1024, latents=pm.latent[:pm.n], obs=pm.obs[:pm.n], optimized=np.ones(pm.n, dtype=np.uint8) if what == "all optimised" else pm.optimized[:pm.n])
        r = Device(q, model).call(xyz, nrm, mask if what == "all optimised" else np.zeros_like(mask), noise, 5, lam=LAMBDA)
        assert r.rows == 0 and r.voxels == 0, what
        assert np.array_equal(bits(r.latent), bits(q.latent)) and np.array_equal(r.optimized, q.optimized) and not r.dirty.any() and not r.slot_flag.any(), what
        assert not r.loss.view(np.uint32).any(), what
    dev = Device(pm, model)
    r1 = dev.call(xyz, nrm, mask, noise, 2, lam=LAMBDA)
    assert r1.rows > 0 and r1.voxels > 0
    r2 = dev.call(xyz, nrm, mask, noise, 2, lam=LAMBDA)
    assert r2.rows == 0 and r2.voxels == 0
    assert np.array_equal(bits(r2.latent), bits(r1.latent)) and np.array_equal(r2.optimized, r1.optimized) and np.array_equal(r2.dirty, r1.dirty)
    assert not r2.slot_flag.any() and not r2.loss.view(np.uint32).any()


# ---- one step: the gradient ---------------------------------------------------------------------------------------------------------
def _one_step(case, model, pipe, fails, reach, k=None):
    """n_iters = 1, lambda = 0: g from m per voxel under the bar, v against g^2 under the matching bar -> the result"""
    r = Device(case.pm, model).call(case.xyz, case.normal, case.mask, case.noise, 1)
    assert r.rows == case.n_rows and np.array_equal(r.uniq_slot, case.uniq) and np.array_equal(r.row_slot, case.row_slot), case.label
    assert np.array_equal(bits(r.row_xyz), bits(case.row_xyz)) and np.array_equal(bits(r.row_sdf), bits(case.row_sdf)), case.label
    ref = case.grad64()
    G, S, rr = ref["G"], ref["S"], ref["r"]
    e_ref = C.max_err(case.grad32()[0], G)
    limit = OC.nll_bar(e_ref, case.rows_u, G, S, k) + U * np.abs(G)                 # (+ half an ulp: g is read back from m = fl(C1 * g))
    g_gpu = r.m.astype(np.float64) / C1
    label = f"{case.label}/{pipe} rows {case.n_rows} [{_kernel(pipe)}]"
    _judge(label, "g (from m)", np.abs(g_gpu - G), limit, e_ref, fails)
    v_lim = C2 * (2.0 * np.abs(G) * limit + limit * limit) + 2.0 * OC.spacing32(C2 * G * G)
    _judge(label, "v", np.abs(r.v.astype(np.float64) - C2 * G * G), v_lim, e_ref, fails)
    # v is formed from the very g that m holds: two roundings of its own and g's read-back
    assert (np.abs(r.v.astype(np.float64) - C2 * g_gpu * g_gpu) <= 6.0 * U * C2 * g_gpu * g_gpu + 2.0 ** -149).all(), label
    for key, frac in (("in", (np.abs(rr["sdf"]) <= 0.2).mean()), ("out", (np.abs(rr["sdf"]) > 0.2).mean()), ("gt", (np.abs(case.row_sdf) > F32(0.2)).mean()),
                      ("pu20", (rr["pu"] > 20).mean())):
        reach[key] = max(reach.get(key, 0.0), float(frac))
    print(f"      dropped {case.dropped:.2%} of the candidate points; |sdf| <= 0.2 {(np.abs(rr['sdf']) <= 0.2).mean():.2%}, |gt| > 0.2 "
          f"{(np.abs(case.row_sdf) > F32(0.2)).mean():.2%}, pu > 20 {(rr['pu'] > 20).mean():.2%}; largest unscaled row gradient {np.abs(rr['grad']).max() * case.n_rows:.3g}")
    return r


@pytest.mark.parametrize("pipe", PIPES)
@pytest.mark.parametrize("ws", C.WEIGHT_SETS + ("large_pu",))
def test_one_step_gradient(ws, pipe, nets):
    """The per-voxel gradient after one step under optim_cases' bar, at latent scales 0.3 and 4 with noise of which about 1 % lies
    beyond 4 sigma; "large_pu": the shipped weights on latents taken from decoder_rows_large_pu's rows (pu > 20 at the actual rows is
    asserted), with its own e_ref; every weight set also on latents whose pu lies just above 10 (optim_cases.near_switch_case: the
    hostile_a rows put a `pu > 20` switch moved to 10 seven bars out); with the shipped weights also n_rows = 1, the largest 1 / n.  Candidate points with a row inside a
    kink margin were dropped by the float64 reference beforehand (at most 5 % per case, asserted where the case is built)."""
    fails, reach = [], {}
    if ws == "large_pu":
        case = OC.one_step_case("large_pu", 0.0)
        _one_step(case, nets("shipped", pipe), pipe, fails, reach)
        assert reach["pu20"] >= 0.01, reach
    else:
        model = nets(ws, pipe)
        for scale in (0.3, 4.0):
            case = OC.one_step_case(ws, scale)
            _one_step(case, model, pipe, fails, reach)
            if scale == 4.0 and ws != "shipped":
                r4 = case.grad64()["r"]
                assert (r4["pu"] > 20).mean() >= 0.01, (ws, (r4["pu"] > 20).mean())
        assert reach["in"] >= 0.01 and reach["out"] >= 0.01 and reach["gt"] >= 0.005, reach
        near = OC.one_step_case(ws, OC.NEAR_SWITCH)               # pu just above 10: softplus' is not yet 1 to float32
        pu = near.grad64()["r"]["pu"]
        assert ((pu > 10) & (pu <= 12)).mean() >= 0.01, (ws, pu.min(), pu.max())
        _one_step(near, model, pipe, fails, {})
        if ws == "shipped":
            one = None
            for seed in range(64):           # one row: the first seed whose single point is not on a kink and lies inside the clamp (a gradient of size)
                pm, xyz, nrm, mask, noise, _ = OC.isolated_scene(1, 1024, seed, n_voxels=1)
                cand = OC.Case(C.bundle(ws), pm, xyz, nrm, noise[:8].reshape(1, 8), f"{ws}/one row", cap=1.0)
                if cand.n_rows == 1 and abs(cand.grad64()["r"]["sdf"][0]) <= 0.19:
                    one = cand
                    break
            assert one is not None and one.n_rows == 1
            _one_step(one, model, pipe, fails, {})
    print(f"  {ws}/{pipe}: reached {reach}")
    assert not fails, "\n".join(fails)


# ---- segmented sums -----------------------------------------------------------------------------------------------------------------
def _isolated_case(ws, n_voxels, vox_of_point, seed, scale=0.3, filter_points=True, zero_voxel=None, capacity=1024):
    """Isolated set voxels with latents N(0, scale) and one point per entry of vox_of_point (one octant): rows equal points"""
    b = C.bundle(ws)
    g = np.random.default_rng([59, seed, n_voxels])
    ijk = OC.isolated_voxels(n_voxels, g)
    lat = (g.standard_normal((n_voxels, 29)) * scale).astype(F32)
    if zero_voxel is not None:
        lat[zero_voxel] = 0.0
    pm = OC.Planted(OC.lin_of(ijk), capacity, latents=lat)
    n = len(vox_of_point)
    xyz = OC.one_octant_points(ijk[vox_of_point], 0.02 + 0.43 * g.random((n, 3)))
    return OC.Case(b, pm, xyz, OC.unit_normals(g, n), OC.planted_noise(g, (n, 8)), f"{ws}/isolated", filter_points=filter_points)


CRAFTED_RUNS = [(0, 1), (1, 15), (0, 16),                      # voxel 0 twice in tile 0, its second run from lane 16
                (2, 17), (3, 15),                              # a run over lanes 0..16
                (4, 31), (5, 32), (6, 33), (7, 70),            # runs that straddle one and two tile boundaries
                (2, 5), (3, 4), (2, 6), (1, 1), (8, 16), (1, 17)]


@pytest.mark.parametrize("pipe", PIPES)
def test_segmented_sums(pipe, nets):
    """The same multiset of rows per voxel three ways: sorted by voxel (long runs), shuffled (runs of about one row), and in crafted
    runs of 1, 15, 16, 17, 31, 32, 33 and 70 rows (straddling lane 15 / 16 and tile boundaries, one voxel recurring in separate runs of a
    tile): m and v bit for bit the same, since the per-voxel sums are exact integers.  And one case past the grid's first stride
    (more than 32 * 4 * CUs + 17 rows) under the bar of the one-step test."""
    model = nets("shipped", pipe)
    crafted = np.concatenate([np.full(n, v) for v, n in CRAFTED_RUNS])
    case = _isolated_case("shipped", 9, crafted, 0, filter_points=False)
    assert np.array_equal(case.uniq[case.inv], case.row_slot) and case.n_rows == crafted.size
    g = np.random.default_rng(61)
    out = {}
    for name, perm in (("crafted", np.arange(crafted.size)), ("sorted", np.argsort(crafted, kind="stable")), ("shuffled", g.permutation(crafted.size))):
        noise = np.zeros(8 * crafted.size, dtype=F32)
        noise[:crafted.size] = case.noise[:crafted.size][perm]                   # rows equal points: the sample travels with its point
        r = Device(case.pm, model).call(case.xyz[perm], case.normal[perm], case.mask, noise, 1)
        assert r.rows == crafted.size and np.array_equal(r.row_slot, case.row_slot[perm])
        out[name] = r
        runs = 1 + int((np.diff(r.row_slot) != 0).sum())
        print(f"  {pipe} {name}: {runs} runs over {r.rows} rows")
    for name in ("sorted", "shuffled"):
        assert np.array_equal(bits(out[name].m), bits(out["crafted"].m)) and np.array_equal(bits(out[name].v), bits(out["crafted"].v)), f"{name} [{_kernel(pipe)}]"
    assert np.abs(out["crafted"].m).max() > 0
    # past the first grid-stride step
    first = 32 * 4 * torch.cuda.get_device_properties(0).multi_processor_count
    n = int((first + 18) / 0.97) + 1
    big = _isolated_case("shipped", 300, np.random.default_rng(67).integers(0, 300, size=n), 1)
    assert big.n_rows > first + 17, (big.n_rows, first)
    fails = []
    _one_step(big, model, pipe, fails, {})
    assert not fails, "\n".join(fails)


# ---- steps, each judged from the GPU's own previous state ---------------------------------------------------------------------------------
def _z_tolerance(z64, delta, k):
    """|z_gpu - float64 Adam on the GPU's own m_k, v_k|.  k_optim_adam evaluates  z - step * (m / (sqrtf(v) / bc2 + eps)),  step = lr / (1 -
    powf(0.9f, k)),  bc2 = sqrtf(1 - powf(0.999f, k)).  With u = 2^-24 per correctly rounded operation and powf within 1 ulp (<= 2 u p
    absolute, HIP math API):  1 - p  is off by u (2 p / (1 - p) + 1) relative;  step: + 1 (the division);  bc2: half of that + 1 (sqrtf);
    then the five operations sqrtf(v), / bc2, + eps, m / ., step * . add u each.  Relative error of the update delta:
        u * (8.5 + 2 p1 / (1 - p1) + p2 / (1 - p2)),     p1 = 0.9^k, p2 = 0.999^k        (1,027 u at k = 1: the cancellation in 1 - 0.999^k)
    and the final subtraction rounds once: 1 ulp of z (half an ulp, a whole one across a binade edge)."""
    p1, p2 = B1 ** k, B2 ** k
    return np.abs(delta) * U * (8.5 + 2.0 * p1 / (1.0 - p1) + p2 / (1.0 - p2)) + OC.spacing32(z64)


STEPS = (1, 2, 5, 70)


@pytest.mark.parametrize("lam", (0.0, LAMBDA))
@pytest.mark.parametrize("pipe", PIPES)
@pytest.mark.parametrize("ws", ("shipped", "hostile_b"))
def test_steps(ws, pipe, lam, nets):
    """For k in 1, 2, 5, 70: n_iters = k - 1 (twice: same bits) and k from the same planted state; the float64 gradient at the GPU's own
    z_{k-1}; m_k against 0.9 m_{k-1} + 0.1 g under 0.1 * the gradient bar + 2 ulp (of the larger term), v_k likewise, z_k against float64
    Adam on the GPU's own m_k, v_k (_z_tolerance).  256 isolated voxels of 8 rows, one of them with an all-zero latent (its regulariser
    term is exactly 0); a voxel with a row inside a kink margin at z_{k-1} is set aside (at most 10 %).  The regulariser's float32
    evaluation (29 squares, a five-level butterfly, sqrtf, a division, two products, inv_n) adds 8 u of its own size.  Then the
    write-back and the flags; and loss_out[i] for i < min(k, 64) against the float64 likelihood at z_i."""
    model, b = nets(ws, pipe), C.bundle(ws)
    case = _isolated_case(ws, 256, np.repeat(np.arange(256), 8), 2, filter_points=False, zero_voxel=5)
    assert case.n_rows == 2048 and (case.rows_u == 8).all() and not case.pm.latent[case.uniq[5]].any()
    n, fails = case.n_rows, []

    def run(k):
        return Device(case.pm, model).call(case.xyz, case.normal, case.mask, case.noise, k, lam=lam)

    z0 = case.pm.latent[case.uniq]
    state = {0: (z0, np.zeros_like(z0), np.zeros_like(z0))}
    losses64 = {}
    final = None
    for k in STEPS + (64,):                                       # 64: z_63, for slot 63 of loss_out
        if k > 1:
            a, a2 = run(k - 1), run(k - 1)
            # (loss_out is summed with float atomics in whatever order the tiles finish: it is under a bar below, not under this)
            differ = {f: int((bits(getattr(a, f)) != bits(getattr(a2, f))).sum()) for f in ("z", "m", "v", "latent")}
            assert not any(differ.values()), f"two runs of {k - 1} steps differ in {differ} elements"
            state[k - 1] = (a.z, a.m, a.v)
        zp, mp, vp = (x.astype(np.float64) for x in state[k - 1])
        ref = case.grad64(zp)
        losses64[k - 1] = (ref["loss"], ref["loss_abs"], case.grad32(state[k - 1][0])[1])
        if k == 64:
            break
        r = run(k)
        assert np.array_equal(r.uniq_slot, case.uniq)
        aside = case.sums(OC.Case.rows_on_a_kink(b, case.rows_at(state[k - 1][0]).astype(F32)).astype(np.int64)) > 0
        assert aside.mean() <= 0.10, (k, aside.mean())
        keep = ~aside
        reg = code_reg_grad64(zp, lam, n) if lam > 0 else np.zeros_like(zp)
        g = ref["G"] + reg
        e_ref = C.max_err(case.grad32(state[k - 1][0])[0][keep], ref["G"][keep])
        d = OC.nll_bar(e_ref, case.rows_u, ref["G"], ref["S"]) + 8.0 * U * np.abs(reg) + OC.spacing32(g)
        label = f"{ws}/{pipe}/lambda {lam:g}/step {k} (set aside {aside.mean():.1%})"
        m_ref, v_ref = B1 * mp + C1 * g, B2 * vp + C2 * g * g
        _judge(label, "m", np.abs(r.m - m_ref)[keep], (C1 * d + 2.0 * OC.spacing32(np.maximum(np.abs(B1 * mp), np.abs(C1 * g))))[keep], e_ref, fails)
        _judge(label, "v", np.abs(r.v - v_ref)[keep], (C2 * (2.0 * np.abs(g) * d + d * d) + 2.0 * OC.spacing32(np.maximum(B2 * vp, C2 * g * g)))[keep], e_ref, fails)
        z64 = adam_update64(zp, r.m.astype(np.float64), r.v.astype(np.float64), k, LR, B1, B2, EPS)
        _judge(label, "z", np.abs(r.z - z64), _z_tolerance(z64, z64 - zp, k), 0.0, fails)      # (rounding only: no e_ref)
        if k == 1:                                               # the all-zero latent: judged above on the likelihood gradient alone
            assert keep[5] and (reg[5] == 0).all() and r.m[5].all()
        _check_bookkeeping(r, case.pm, case.uniq, label)
        final = r
    # the loss: slot i holds the likelihood at z_i for i < min(k, 64); with 70 steps slot 63 is step 64's value alone
    assert final.loss.shape == (64,)
    tiles = (n + 31) // 32
    for i in (0, 1, 4, 63):
        want, want_abs, oracle = losses64[i]
        limit = OC.K_NLL * abs(oracle - want) + (tiles + 6) * U * want_abs
        err = abs(float(final.loss[i]) - want)
        print(f"  {ws}/{pipe}/lambda {lam:g} loss_out[{i}] {final.loss[i]:.7g}  float64 {want:.7g}  err {err:.2e}  bar {limit:.2e}  e_gpu/e_ref {err / max(abs(oracle - want), 1e-300):.2f}")
        if err > limit:
            fails.append(f"loss_out[{i}] = {final.loss[i]!r}, float64 {want!r}: err {err:.3e} > {limit:.3e}")
    r5 = run(5)
    assert not r5.loss[5:].view(np.uint32).any() and r5.loss[:5].all()
    assert not fails, "\n".join(fails)
