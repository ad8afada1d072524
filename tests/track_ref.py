"""Numpy restatement of the tracker's SDF term (csrc/kernels_track.hip.h, the DENSE row fetch of csrc/kernels_extract.hip.h; reference
tracker.py:174-218, map.py:559-579), stage by stage: which points of a posed cloud are valid and what decoder rows they give, the per-point
terms s, w, wf, J from the decoder's outputs, and the 44 numbers from those.

Per-point quantities are float32 in the kernels' op order (numpy's elementwise float32 operations are correctly rounded and never fused), so
the valid set and the flat terms are reproduced exactly; the sums are float64.  The valid set can ONLY be judged in float32: a float64
evaluation of the pose puts a point that sits on a voxel face on the other side about as often as not (tests/test_track_cpu.py).
Test helper, like tests/photo_ref.py; no GPU, no torch."""
import numpy as np

from oracle import difusion_oracle as O
from tests import photo_ref as P

F = np.float32
KERNELS = [(None, 0.0), ("huber", 0.75), ("tukey", 1.5)]
ROBUST_ID = {None: 0, "huber": 1, "tukey": 2}


def rows34(R, t):
    """The twelve floats the library takes for a pose: rows of [R | t], float32 of the float64 entries."""
    return np.concatenate([np.asarray(R, dtype=np.float64).astype(F), np.asarray(t, dtype=np.float64).astype(F)[:, None]], axis=1).reshape(12)


# ---- the dense row fetch (decode_row_input<DENSE>: pose_row, voxel_of, indexer, count gate) -----------------------------------------------
def posed_xn(om, cloud, T_cur):
    """pose_row then normalize1, float32: (posed (N,3), xn (N,3)).  T_cur = (R, t)."""
    with np.errstate(all="ignore"):
        cur = O._rigid32(T_cur[0], T_cur[1], np.asarray(cloud, dtype=F))
        xn = ((cur - om.bound_min[None, :].astype(F)) / F(om.voxel_size)).astype(F)
    return cur, xn


def dense_rows(om, cloud, T_cur):
    """-> (valid (N,) bool, rows (M,32) float32 = [latent | rel] of the valid points in cloud order).  A point is valid when, per axis,
    1 <= ceil(xn) <= n (NaN and infinities fail), its voxel ceil(xn) - 1 is allocated, and the voxel's count is > ignore_count_th."""
    _, xn = posed_xn(om, cloud, T_cur)
    with np.errstate(all="ignore"):
        c = np.ceil(xn)
        ok = np.all((c >= F(1)) & (c <= np.asarray(om.n_xyz, dtype=F)[None, :]), axis=1)
    ix = np.where(ok[:, None], c, F(1)).astype(np.int64) - 1
    slot = np.where(ok, om.indexer[om._linearize_id(ix)], -1)
    ok = slot >= 0
    ok[ok] = om.voxel_obs_count[slot[ok]] > F(om.ignore_count_th)
    rel = ((xn[ok] - ix[ok].astype(F)).astype(F) - F(0.5)).astype(F)
    return ok, np.concatenate([om.latent_vecs[slot[ok]].astype(F), rel], axis=1)


# ---- hg_accumulate: the per-point terms -------------------------------------------------------------------------------------------------
def flat_terms(sdf, std, grad, obs, T_delta, Lt, kernel, k):
    """The terms of the rows with std != 0, in row order: s = sdf / std, w = robust(s), wf = s w (float32, (M,)) and
    J (M,6) = [d Lt | (T_delta obs) x (d Lt)] with d = grad / std (None when `grad` is None: the value-only call).
    Lt (3,3) = last_R^T; T_delta = (R, t).  Division by std, three-term products left to right, Huber ab > k, Tukey |s| <= k."""
    sdf, std = np.asarray(sdf, dtype=F), np.asarray(std, dtype=F)
    keep = ~(std == F(0))
    sd = std[keep]
    with np.errstate(all="ignore"):
        s = (sdf[keep] / sd).astype(F)
        w = P.robust_weight(s, kernel, F(k))
        wf = (s * w).astype(F)
        if grad is None:
            return s, w, wf, None
        d = (np.asarray(grad, dtype=F)[keep] / sd[:, None]).astype(F)
        Lt = np.asarray(Lt, dtype=np.float64).astype(F)
        Ja = np.stack([(d[:, 0] * Lt[0, j] + d[:, 1] * Lt[1, j]) + d[:, 2] * Lt[2, j] for j in range(3)], axis=1).astype(F)
        c = O._rigid32(T_delta[0], T_delta[1], np.asarray(obs, dtype=F)[keep])
        Jb = np.stack([c[:, 1] * Ja[:, 2] - c[:, 2] * Ja[:, 1], c[:, 2] * Ja[:, 0] - c[:, 0] * Ja[:, 2], c[:, 0] * Ja[:, 1] - c[:, 1] * Ja[:, 0]],
                      axis=1).astype(F)
    return s, w, wf, np.concatenate([Ja, Jb], axis=1)


# ---- the sums -----------------------------------------------------------------------------------------------------------------------------
def sums_of_flat(s, w, wf, J):
    """-> (out (44,) float64 = H row-major | g | e | M, S (43,) float64 = the sum of the ABSOLUTE values of every entry's terms on the same
    scale).  Products of two float32 factors in double (exact), summed over the M rows in float64, then / M.  J None: e and M only."""
    M = int(np.asarray(s).size)
    out, S = np.zeros(44), np.zeros(43)
    out[43] = M
    if M == 0:
        return out, S
    s64, wf64 = np.asarray(s, dtype=F).astype(np.float64), np.asarray(wf, dtype=F).astype(np.float64)
    te = s64 * wf64
    out[42], S[42] = te.sum() / M, np.abs(te).sum() / M
    if J is not None:
        J = np.asarray(J, dtype=F)
        JW = (J * np.asarray(w, dtype=F)[:, None]).astype(F).astype(np.float64)
        J64 = J.astype(np.float64)
        for r in range(6):
            for c in range(6):
                tt = JW[:, min(r, c)] * J64[:, max(r, c)]
                out[r * 6 + c], S[r * 6 + c] = tt.sum() / M, np.abs(tt).sum() / M
            tg = J64[:, r] * wf64
            out[36 + r], S[36 + r] = tg.sum() / M, np.abs(tg).sum() / M
    return out, S


def within(x, x_ref, S, slack, what):
    """|x - x_ref| <= slack * S, entry by entry (S: the sum of the absolute values of the entry's terms)."""
    err = np.abs(np.asarray(x, dtype=np.float64) - np.asarray(x_ref, dtype=np.float64))
    bar = slack * np.asarray(S)
    bad = np.nonzero(~(err <= bar))[0]
    assert bad.size == 0, f"{what}: entries {bad[:6].tolist()} off by {err[bad][:6]} (bar {bar[bad][:6]})"
    pos = np.asarray(S) > 0
    return float((err[pos] / np.asarray(S)[pos]).max()) if pos.any() else 0.0          # the worst error in units of S


def compute_sdf_hg(om, obs_xyz, last_R, last_t, delta_R, delta_t, kernel=None, k=0.0, no_grad=False):
    """The whole term on an OracleMap through the three stages above, the decoder being the float32 oracle's: (out (44,), S (43,), valid)."""
    last_R, delta_R = np.asarray(last_R, dtype=np.float64), np.asarray(delta_R, dtype=np.float64)
    cur = (last_R @ delta_R, last_R @ np.asarray(delta_t, dtype=np.float64) + np.asarray(last_t, dtype=np.float64))
    obs_xyz = np.asarray(obs_xyz, dtype=F)
    valid, rows = dense_rows(om, obs_xyz, cur)
    sdf, std, grad = np.zeros(valid.size, dtype=F), np.zeros(valid.size, dtype=F), np.zeros((valid.size, 3), dtype=F)
    if rows.shape[0]:
        sdf[valid], std[valid], g = om.net.decoder_xyz_grad(rows)
        grad[valid] = (g / F(om.voxel_size)).astype(F)
    s, w, wf, J = flat_terms(sdf, std, None if no_grad else grad, obs_xyz, (delta_R, delta_t), last_R.T, kernel, k)
    return (*sums_of_flat(s, w, wf, J), valid)
