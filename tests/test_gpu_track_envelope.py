"""GPU: the tracker's SDF term (`dif_sdf_hg`) stage by stage against tests/track_ref.py — the dense query rows the decoder leaves in the
workspace (the DENSE instantiations of csrc/kernels_extract.hip.h, read through the test hook dif_test_sdf_hg_views), then the reduction
(`hg_accumulate` and the loop of k_sdf_hg_reduce, csrc/kernels_track.hip.h; alone through dif_test_sdf_hg_reduce).

WHICH ORACLE JUDGES WHAT.
  the valid set            track_ref.dense_rows: the float32 rule in the kernel's op order, EXACT (std == 0 marks a row that is not valid)
  sdf, std, grad of a row  tests/ref64.py (float64) under the bar of tests/mlp_cases.py: K_BAR * e_ref + U ulp, e_ref the float32 oracle's error
                           on the same rows; and bit for bit the rows `get_sdf` / `get_sdf_with_gradient` give for the host-posed cloud
  the 44 numbers           track_ref.sums_of_flat(flat_terms(the GPU's own rows)): M exact, every entry within SUM_SLACK x S
Maps: seq_small (8^3 voxels) with planted latents, counts in six voxels on the decode gate (tests/track_cases.py); what the generated
cloud promises is asserted without a GPU by tests/test_track_cpu.py.  Every test prints its worst figures (`TRACK_ENV` lines)."""
import ctypes

import numpy as np
import pytest
import torch

from di_fusion_amd import _lib
from di_fusion_amd.network import utility as net_util
from oracle import difusion_oracle as O
from tests import mlp_cases as C
from tests import track_cases as K
from tests import track_ref as T
from tests.test_gpu_mlp_envelope import SEQ, _judge, bits

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PIPES = ("bf16x6", "f32")
F32 = np.float32
SUM_SLACK = 1e-10          # as tests/test_gpu_photo.py: two float64 summation orders of N terms differ by at most N * 2^-53 * S, below this up to 9e5 points
HG_BLOCKS, HG_TERMS = 256, 29
DENSE_KERNEL = {("bf16x6", False): "k_decode_x6<true>", ("bf16x6", True): "k_decode_grad_x6<PF,true>",
                ("f32", False): "k_decode<false,true>", ("f32", True): "k_decode<true,true>"}


@pytest.fixture(scope="module")
def nets():
    """One Networks per (weight set, pipe), built on first use."""
    cache = {}

    def get(ws, pipe):
        if (ws, pipe) not in cache:
            cache[ws, pipe] = net_util.networks_from_arrays(C.weight_set(ws), x6=(pipe == "bf16x6"))
        return cache[ws, pipe]
    return get


@pytest.fixture(scope="module")
def maps(nets):
    """(weight set, pipe, latent scale) -> (map, OracleMap with the same state, n_occupied); shared by the cases with and without derivatives."""
    cache = {}

    def get(ws, pipe, scale):
        if (ws, pipe, scale) not in cache:
            from di_fusion_amd.system.map import DenseIndexedMap
            om, n, lat, frames, _ = K.track_map(C.bundle(ws).oracle, C.WEIGHT_SETS.index(ws), scale)
            m = DenseIndexedMap(nets(ws, pipe), SEQ[1].namespace(), 29, DEV, initial_capacity=1024)
            for xyz, nrm in frames:
                m.integrate_keyframe(torch.from_numpy(xyz).to(DEV), torch.from_numpy(nrm).to(DEV))
            assert n == m.n_occupied and np.array_equal(m.latent_vecs_pos[:n].cpu().numpy(), om.latent_vecs_pos[:n])
            m._latent[:n] = torch.from_numpy(lat).to(DEV)
            m._obs[:n] = torch.from_numpy(om.voxel_obs_count[:n]).to(DEV)              # 100, and the six voxels on the gate
            cache[ws, pipe, scale] = (m, om, n)
        return cache[ws, pipe, scale]
    return get


_REF = {}


def reference(ws, scale, pose_name, om):
    """Per (weight set, scale, pose), computed once: the valid set, the decoder rows, their float64 values, the float32 oracle's and grad_keep."""
    key = (ws, scale, pose_name)
    if key not in _REF:
        b = C.bundle(ws)
        valid, rows = T.dense_rows(om, K.cloud()[0], POSES[pose_name][0])
        _REF[key] = dict(valid=valid, rows=rows, r64=b.ref.decoder_xyz_grad(rows), o32=b.oracle.decoder_xyz_grad(rows), keep=b.grad_keep(rows))
    return _REF[key]


# pose name -> (T_cur = last . delta as (R, t), last, delta)
POSES = {"identity": (K.IDENTITY, K.IDENTITY, K.IDENTITY), "posed": (K.pose(), *K.split_pose())}


class Workspace:
    """A dif_sdf_hg workspace for N points filled with `fill` bytes, and where its views are (dif_test_sdf_hg_views)."""

    def __init__(self, N, fill=0xFF, capacity=None):
        lib = _lib.load()
        self.N = N
        self.bytes = int(lib.dif_sdf_hg_workspace_bytes(N))
        size = max(self.bytes, int(lib.dif_sdf_hg_workspace_bytes(capacity)) if capacity else 0)
        self.buf = torch.full((size + 256,), fill, dtype=torch.uint8, device=DEV)
        self.skip = (-self.buf.data_ptr()) % 256
        self.base = self.buf.data_ptr() + self.skip
        self.size = size
        self.relayout(N)

    def relayout(self, N):
        lib = _lib.load()
        v = _lib.DifSdfHgViews()
        assert lib.dif_test_sdf_hg_views(N, ctypes.c_void_p(self.base), ctypes.byref(v)) == 0
        self.N, self.bytes = N, int(lib.dif_sdf_hg_workspace_bytes(N))
        self.sdf, self.std, self.grad = v.sdf - self.base, v.std - self.base, v.grad - self.base
        self.partial, self.ticket = int(v.partial_offset), int(v.ticket_offset)
        up = lambda x: (x + 255) // 256 * 256   # noqa: E731
        assert (self.sdf, self.std, self.grad) == (0, up(4 * N), 2 * up(4 * N)) and self.partial == self.grad + up(12 * N)
        assert self.ticket == self.partial + up(HG_BLOCKS * HG_TERMS * 8) and self.bytes == self.ticket + 256 <= self.size

    def host(self):
        return self.buf[self.skip:self.skip + self.bytes].cpu().numpy()

    def put(self, offset, a):
        a = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(DEV)
        self.buf[self.skip + offset:self.skip + offset + a.numel()] = a

    def rows(self, with_grad=True):
        """-> (sdf (N,), std (N,), grad (N,3) or None, padding bytes of the three views) from the device"""
        h, N = self.host(), self.N
        f = lambda off, n: h[off:off + 4 * n].view(F32).copy()   # noqa: E731
        pad = np.concatenate([h[self.sdf + 4 * N:self.std], h[self.std + 4 * N:self.grad], h[self.grad + 12 * N:self.partial]])
        return f(self.sdf, N), f(self.std, N), f(self.grad, 3 * N).reshape(N, 3), pad, h


def hg_args(T_cur, delta, last, kernel, k, no_grad):
    a = _lib.DifSdfHg()
    a.T_cur[:] = T.rows34(*T_cur).tolist()
    a.T_delta[:] = T.rows34(*delta).tolist()
    a.last_Rt[:] = np.asarray(last[0], dtype=np.float64).astype(F32).T.reshape(9).tolist()
    a.robust_kernel, a.robust_k, a.no_grad = T.ROBUST_ID[kernel], float(k), 1 if no_grad else 0
    return a


def sdf_hg(m, cloud_t, a, ws):
    """dif_sdf_hg through ctypes, no host hand-back: the 44 numbers after a synchronize."""
    out = torch.full((44,), float("nan"), dtype=torch.float64, device=DEV)
    w = m.model.packed.weights_struct(DEV)
    _lib.check(_lib.load().dif_sdf_hg(ctypes.byref(m._cmap), ctypes.byref(w), _lib.ptr(cloud_t), int(cloud_t.size(0)), ctypes.byref(a),
                                      ctypes.c_void_p(ws.base), ws.bytes, _lib.ptr(out), None, 0, _lib.stream_ptr()), "dif_sdf_hg")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def reduce_only(obs_t, N, a, ws):
    out = torch.full((44,), float("nan"), dtype=torch.float64, device=DEV)
    _lib.check(_lib.load().dif_test_sdf_hg_reduce(_lib.ptr(obs_t), N, ctypes.byref(a), ctypes.c_void_p(ws.base), ws.bytes, _lib.ptr(out),
                                                  _lib.stream_ptr()), "dif_test_sdf_hg_reduce")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def check_sums(out, sdf, std, grad, cloud, delta, last, kernel, k, what):
    """The 44 numbers against the float64 sums of the flat terms of these rows -> the worst error in units of S."""
    s, w, wf, J = T.flat_terms(sdf, std, grad, cloud, delta, np.asarray(last[0]).T, kernel, k)
    want, S = T.sums_of_flat(s, w, wf, J)
    assert int(out[43]) == int(want[43]) and out[43] == float(int(out[43])), f"{what}: M {out[43]} != {want[43]}"
    assert not np.isnan(out).any(), f"{what}: NaN in the result"
    worst = T.within(out[:43], want[:43], S, SUM_SLACK, what)
    H = out[:36].reshape(6, 6)
    assert np.array_equal(H.view(np.uint64), H.T.copy().view(np.uint64)), f"{what}: H is not symmetric bit for bit"
    if grad is None:
        assert not out[:42].any(), f"{what}: a value-only call wrote H or g"
    return worst


# ---- a. dense rows ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grad", (True, False), ids=("grad", "values"))
@pytest.mark.parametrize("pipe", PIPES)
@pytest.mark.parametrize("ws", C.WEIGHT_SETS)
def test_dense_rows(ws, pipe, grad, maps):
    """The ~2k-point cloud of track_cases.cloud() under the identity and under a 0.27 rad / 0.17 m pose, latents N(0, 0.3) and N(0, 4), the
    workspace filled with 0xFF bytes before every call."""
    xyz, kind, _, _ = K.cloud()
    N = len(xyz)
    cloud_t = torch.from_numpy(xyz).to(DEV)
    label0, fails, worst_sum = f"{ws}/{pipe} [{DENSE_KERNEL[pipe, grad]}]", [], 0.0
    n_call = 0
    for scale in K.SCALES:
        m, om, n = maps(ws, pipe, scale)
        vs = om.voxel_size
        for pose_name, (Tc, last, delta) in POSES.items():
            kernel, k = T.KERNELS[n_call % 3]
            n_call += 1
            label = f"{label0} N(0,{scale:g}) {pose_name}"
            ref = reference(ws, scale, pose_name, om)
            valid, keep = ref["valid"], ref["keep"]
            a = hg_args(Tc, delta, last, kernel, k, not grad)
            wsp = Workspace(N, 0xFF)
            out = sdf_hg(m, cloud_t, a, wsp)
            sdf, std, g3, pad, h = wsp.rows()
            # the valid set: exact
            wrong = np.nonzero((std == 0) != ~valid)[0]
            assert wrong.size == 0, f"{label}: {wrong.size} rows with the wrong verdict, first {wrong[:6].tolist()} of kinds {kind[wrong[:6]].tolist()}"
            # nothing but std = 0 is written for a row that is not valid; nothing behind row N - 1; nothing in grad without derivatives
            assert (bits(sdf[~valid]) == 0xFFFFFFFF).all() and (bits(g3[~valid]) == 0xFFFFFFFF).all(), f"{label}: a row that is not valid was written"
            assert pad.size > 0 and (pad == 0xFF).all(), f"{label}: bytes behind the last row of a view were written"
            if not grad:
                assert (h[wsp.grad:wsp.partial] == 0xFF).all(), f"{label}: the value-only call wrote the gradient view"
            assert h[wsp.ticket:wsp.ticket + 4].view(np.int32)[0] == 0, f"{label}: the ticket is not left at 0"
            # the rows under the bar
            r_sdf, r_std, r_grad = ref["r64"]
            o_sdf, o_std, o_grad = ref["o32"]
            _judge(label, "sdf", C.max_err(sdf[valid], r_sdf), C.max_err(o_sdf, r_sdf), 1.0, C.U_SDF, fails)
            _judge(label, "std", C.max_err(std[valid], r_std), C.max_err(o_std, r_std), np.abs(r_std).max(), C.U_STD, fails)
            if grad:
                _judge(label, "d sdf / d xyz", C.max_err(g3[valid][keep], r_grad[keep] / vs), C.max_err(o_grad[keep] / F32(vs), r_grad[keep] / vs),
                       np.abs(r_grad[keep]).max() / vs, C.U_GRAD, fails)
            # the same rows from the compacting query on the host-posed cloud: bit for bit
            with np.errstate(all="ignore"):
                q = torch.from_numpy(O._rigid32(Tc[0], Tc[1], xyz)).to(DEV)
            if grad:
                q_sdf, q_std, q_mask, q_grad = m.get_sdf_with_gradient(q)
                assert np.array_equal(bits(q_grad.cpu().numpy()), bits(g3[valid])), f"{label}: gradient rows differ from get_sdf_with_gradient's"
            else:
                q_sdf, q_std, q_mask = m.get_sdf(q)
            assert np.array_equal(q_mask.cpu().numpy(), valid), f"{label}: get_sdf's mask differs"
            assert np.array_equal(bits(q_sdf.cpu().numpy()), bits(sdf[valid])) and np.array_equal(bits(q_std.cpu().numpy()), bits(std[valid])), \
                f"{label}: rows differ from the compacting query's"
            # the 44 numbers from the GPU's own rows
            assert int(out[43]) == int(valid.sum())
            worst_sum = max(worst_sum, check_sums(out, sdf, std, g3 if grad else None, xyz, delta, last, kernel, k, f"{label} {kernel}"))
            # a poisoned ticket (-1 from the fill) and a zeroed workspace: the same bits
            again = sdf_hg(m, cloud_t, a, Workspace(N, 0x00))
            assert np.array_equal(out.view(np.uint64), again.view(np.uint64)), f"{label}: the result depends on what the workspace held"
            if not grad:                                     # the value-only kernel and the gradient kernel agree on M
                full = sdf_hg(m, cloud_t, hg_args(Tc, delta, last, kernel, k, False), Workspace(N, 0xFF))
                assert full[43] == out[43], f"{label}: M {out[43]} without derivatives, {full[43]} with"
    print(f"  TRACK_ENV dense {label0}: worst sum error {worst_sum:.2e} S")
    assert not fails, "\n".join(fails)


# ---- b. tails and the decoder's grid cap -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grad", (True, False), ids=("grad", "values"))
@pytest.mark.parametrize("pipe", PIPES)
def test_dense_rows_tails_and_grid_cap(pipe, grad, maps):
    """N in {1, 31, 32, 33, 63, 65} and 3 * CUs * 256 + 17 points (three grid-stride steps of either kernel and a ragged tail), the cloud
    repeated cyclically: every row equals, bit for bit, the same point's row in a 4,096-point call; nothing behind row N - 1 is written."""
    m, om, n = maps("shipped", pipe, 4.0)
    xyz = K.cloud()[0]
    xyz = xyz[np.arange(4096) % len(xyz)]
    Tc, last, delta = POSES["posed"]
    a = hg_args(Tc, delta, last, "huber", 0.75, not grad)

    def run(N):
        idx = np.arange(N) % 4096
        wsp = Workspace(N, 0xFF)
        out = sdf_hg(m, torch.from_numpy(xyz[idx]).to(DEV), a, wsp)
        sdf, std, g3, pad, _ = wsp.rows()
        assert (pad == 0xFF).all() and int(out[43]) == int((std != 0).sum()), (N, DENSE_KERNEL[pipe, grad])
        return np.concatenate([sdf[:, None], std[:, None], g3], axis=1), idx

    base, _ = run(4096)
    assert 1000 < int((base[:, 1] != 0).sum()) < 4096
    big = 3 * torch.cuda.get_device_properties(0).multi_processor_count * 256 + 17
    for N in (1, 31, 32, 33, 63, 65, big):
        rows, idx = run(N)
        bad = np.nonzero((bits(rows) != bits(base[idx])).any(axis=1))[0]
        assert bad.size == 0, f"N={N} [{DENSE_KERNEL[pipe, grad]}]: {bad.size} rows differ from the 4,096-point call, first {bad[:5].tolist()}"


# ---- c. the reduction alone -----------------------------------------------------------------------------------------------------------------
# grid = min(ceil(N / 512), 256) workgroups of 256 threads, two points per thread and trip: one, two, three workgroups; the cap (131072) and the
# first point of a second trip whose partner falls off the end (131073: m1 == m); a partial third trip (262401 = 4 * 65536 + 257)
REDUCE_N = (0, 1, 255, 256, 257, 511, 512, 513, 1023, 1025, 131072, 131073, 262401)
REDUCE_POSE = K.split_pose()


def _reduce_case(N, fill=0xFF, capacity=None, wsp=None):
    sdf, std, grad, obs = K.reduce_rows(N)
    if wsp is None:
        wsp = Workspace(N, fill, capacity)
    else:
        wsp.relayout(N)
    wsp.put(wsp.sdf, sdf); wsp.put(wsp.std, std); wsp.put(wsp.grad, grad)
    obs_t = torch.from_numpy(obs if N else np.zeros((1, 3), dtype=F32)).to(DEV)
    return (sdf, std, grad, obs), obs_t, wsp


@pytest.mark.parametrize("N", REDUCE_N)
def test_reduction_alone(N):
    """k_sdf_hg_reduce on random per-point rows (30 % of them std == 0 with NaN in sdf and grad) and the rows crafted onto the robust kernels'
    thresholds, every robust kernel, with and without derivatives, in a workspace whose other bytes are 0xFF (NaN partial rows, ticket -1)."""
    last, delta = REDUCE_POSE
    (sdf, std, grad, obs), obs_t, wsp = _reduce_case(N)
    worst = 0.0
    for kernel, k in T.KERNELS:
        for no_grad in (False, True):
            a = hg_args(K.pose(), delta, last, kernel, k, no_grad)
            out = reduce_only(obs_t, N, a, wsp)
            what = f"reduction N={N} {kernel} {'values' if no_grad else 'grad'}"
            worst = max(worst, check_sums(out, sdf, std, None if no_grad else grad, obs, delta, last, kernel, k, what))
            assert int(out[43]) == int((std != 0).sum())
            again = reduce_only(obs_t, N, a, wsp)
            assert np.array_equal(out.view(np.uint64), again.view(np.uint64)), f"{what}: two calls, two results"
            if N == 0:
                assert not out.any()
    print(f"  TRACK_ENV reduce N={N}: worst sum error {worst:.2e} S")


def test_reduction_after_a_larger_one_in_the_same_workspace():
    """N = 513 (two workgroups) directly after N = 262401 (256 workgroups) in the same workspace equals, bit for bit, N = 513 in a fresh one:
    no partial row of the larger launch is read."""
    last, delta = REDUCE_POSE
    a = hg_args(K.pose(), delta, last, "tukey", 1.5, False)
    _, obs_small, fresh = _reduce_case(513, 0x00)
    want = reduce_only(obs_small, 513, a, fresh)
    _, obs_big, wsp = _reduce_case(262401, 0xFF)
    big = reduce_only(obs_big, 262401, a, wsp)
    assert int(big[43]) > 150000
    rows, obs_small, wsp = _reduce_case(513, wsp=wsp)
    got = reduce_only(obs_small, 513, a, wsp)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    check_sums(got, *rows[:3], rows[3], delta, last, "tukey", 1.5, "N=513 after N=262401")


def test_hooks_refuse_what_dif_sdf_hg_refuses():
    lib = _lib.load()
    (_, _, _, _), obs_t, wsp = _reduce_case(513)
    a = hg_args(K.pose(), REDUCE_POSE[1], REDUCE_POSE[0], None, 0.0, False)
    out = torch.zeros((44,), dtype=torch.float64, device=DEV)

    def call(obs=obs_t, N=513, base=wsp.base, nbytes=wsp.bytes, out_ptr=_lib.ptr(out)):
        return int(lib.dif_test_sdf_hg_reduce(_lib.ptr(obs), N, ctypes.byref(a), ctypes.c_void_p(base), nbytes, out_ptr, _lib.stream_ptr()))

    assert call() == 0
    torch.cuda.synchronize()
    assert call(nbytes=wsp.bytes - 1) == -1 and call(base=wsp.base + 64) == -1 and call(base=0) == -1 and call(out_ptr=None) == -1
    assert call(obs=None) == -1 and call(N=-1) == -1
    a.robust_kernel = 3
    assert call() == -1
    v = _lib.DifSdfHgViews()
    assert lib.dif_test_sdf_hg_views(-1, ctypes.c_void_p(wsp.base), ctypes.byref(v)) == -1
    assert lib.dif_test_sdf_hg_views(4, None, ctypes.byref(v)) == -1
