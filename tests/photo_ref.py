"""Numpy restatement of the tracker's photometric term: the reference's image kernels (ext/imgproc/photometric.cu: gradient_xy_kernel,
evaluate_fJ), its pyramid (tracker.py:41-56) and the Python of `compute_rgb_Hg` (tracker.py:131-172).

Per-pixel quantities are float32 in the op order of csrc/kernels_photo.hip.h (numpy's elementwise float32 operations are correctly rounded and
never fused), so the flat operators are reproduced bit for bit; the sums are float64.  Test helper, like tests/ref64.py; no GPU, no torch."""
import hashlib

import numpy as np

F = np.float32
SHIPPED_RGB = dict(weight=500.0, robust_kernel=None, robust_k=0.01, min_grad_scale=0.0, max_depth_delta=0.2)      # configs/fusion-lr-kt.yaml:51-56
SHIPPED_ITERS = [{"n": 10, "type": [["rgb", 2]]}, {"n": 10, "type": [["sdf"], ["rgb", 1]]}, {"n": 50, "type": [["sdf"], ["rgb", 0]]}]
KERNELS = [(None, 0.0), ("huber", 0.01), ("tukey", 0.05)]


def sha(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# ---- the image kernels ----------------------------------------------------------------------------------------------------------------
def gradient_xy(I):
    """photometric.cu:3-22: (H,W) -> (H,W,2), (d1 + 2 d2 + d3) / 8 left to right, NaN on the one-pixel border."""
    I = np.asarray(I, dtype=F)
    H, W = I.shape
    G = np.full((H, W, 2), np.nan, dtype=F)
    if H < 3 or W < 3:
        return G
    n = lambda i, j: I[i:H - 2 + i, j:W - 2 + j]   # noqa: E731   n(i, j) = I[v - 1 + i][u - 1 + j] over the interior
    u1, u2, u3 = n(0, 2) - n(0, 0), n(1, 2) - n(1, 0), n(2, 2) - n(2, 0)
    G[1:-1, 1:-1, 0] = ((u1 + F(2) * u2) + u3) / F(8)
    v1, v2, v3 = n(2, 0) - n(0, 0), n(2, 1) - n(0, 1), n(2, 2) - n(0, 2)
    G[1:-1, 1:-1, 1] = ((v1 + F(2) * v2) + v3) / F(8)
    return G


def intensity_of(rgb):
    """torch.mean(rgb, -1) on three elements: ((r + g) + b) / 3."""
    rgb = np.asarray(rgb, dtype=F)
    return ((rgb[..., 0] + rgb[..., 1]) + rgb[..., 2]) / F(3)


def _src(n_in, n_out):
    """torch's bilinear source index (align_corners=False): i0, i1, lambda (float32)."""
    scale = F(n_in) / F(n_out)
    f = np.maximum(scale * (np.arange(n_out, dtype=F) + F(0.5)) - F(0.5), F(0))
    i0 = np.minimum(f.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    lam = np.minimum(np.maximum(f - i0.astype(F), F(0)), F(1))
    return i0, i1, lam


def resize_bilinear(I, h, w):
    I = np.asarray(I, dtype=F)
    y0, y1, ly = _src(I.shape[0], h)
    x0, x1, lx = _src(I.shape[1], w)
    my, mx = (F(1) - ly)[:, None], (F(1) - lx)[None, :]
    ly, lx = ly[:, None], lx[None, :]
    a00, a01, a10, a11 = I[y0][:, x0], I[y0][:, x1], I[y1][:, x0], I[y1][:, x1]
    return my * (mx * a00 + lx * a01) + ly * (mx * a10 + lx * a11)


def resize_nearest(D, h, w):
    D = np.asarray(D, dtype=F)
    ys = np.minimum(np.floor(np.arange(h, dtype=F) * (F(D.shape[0]) / F(h))).astype(np.int64), D.shape[0] - 1)
    xs = np.minimum(np.floor(np.arange(w, dtype=F) * (F(D.shape[1]) / F(w))).astype(np.int64), D.shape[1] - 1)
    return D[ys][:, xs]


def pyramid(intensity, depth):
    """tracker.py:41-56: three lists of three levels."""
    Is, Ds = [np.asarray(intensity, dtype=F)], [np.asarray(depth, dtype=F)]
    for _ in range(2):
        h, w = Is[-1].shape[0] // 2, Is[-1].shape[1] // 2
        Is.append(resize_bilinear(Is[-1], h, w))
        Ds.append(resize_nearest(Ds[-1], h, w))
    return Is, Ds, [gradient_xy(i) for i in Is]


def _rn(q):
    """CUDA's __float2int_rn: round half to even; NaN -> 0; beyond the int range -> the nearest int."""
    q = np.asarray(q, dtype=F)
    with np.errstate(invalid="ignore"):
        r = np.clip(np.rint(q).astype(np.float64), -2147483648.0, 2147483647.0)
    return np.where(np.isnan(q), 0.0, r).astype(np.int64)


def rgb_odometry(prev_I, prev_D, cur_I, cur_D, cur_G, intr, krkinv, kt, min_grad_scale, max_depth_delta, compute_J=True):
    """photometric.cu:24-77 over the whole image: f (H,W) NaN where invalid, J (H,W,6) NaN where f is (None without `compute_J`)."""
    prev_I, prev_D, cur_I, cur_D, cur_G = (np.asarray(a, dtype=F) for a in (prev_I, prev_D, cur_I, cur_D, cur_G))
    H, W = cur_I.shape
    k = [F(x) for x in krkinv]
    t = [F(x) for x in kt]
    fx, fy, cx, cy = (F(x) for x in intr)
    fu = np.arange(W, dtype=F)[None, :] + np.zeros((H, 1), dtype=F)
    fv = np.arange(H, dtype=F)[:, None] + np.zeros((1, W), dtype=F)
    with np.errstate(all="ignore"):
        gx, gy = cur_G[..., 0], cur_G[..., 1]
        m2 = (gx * gx) + (gy * gy)
        ok = ~((m2 < F(min_grad_scale)) | np.isnan(m2)) & ~np.isnan(cur_D)
        d1 = cur_D
        wd = d1 * ((k[6] * fu + k[7] * fv) + k[8]) + t[2]
        u0 = _rn((d1 * ((k[0] * fu + k[1] * fv) + k[2]) + t[0]) / wd)
        v0 = _rn((d1 * ((k[3] * fu + k[4] * fv) + k[5]) + t[1]) / wd)
        ok &= (u0 >= 0) & (u0 < W) & (v0 >= 0) & (v0 < H)
        uc, vc = np.where(ok, u0, 0), np.where(ok, v0, 0)
        d0, pi = prev_D[vc, uc], prev_I[vc, uc]
        ok &= ~np.isnan(d0) & (np.abs(wd - d0) <= F(max_depth_delta)) & (d0 > F(0))
        f = np.where(ok, cur_I - pi, F(np.nan)).astype(F)
        if not compute_J:
            return f, None
        Gx, Gy, Gz = d0 * (u0.astype(F) - cx) / fx, d0 * (v0.astype(F) - cy) / fy, d0
        p0, p1 = gx * fx / Gz, gy * fy / Gz
        p2 = -(p0 * Gx + p1 * Gy) / Gz
        J = np.stack([p0, p1, p2, (-Gz) * p1 + Gy * p2, Gz * p0 - Gx * p2, (-Gy) * p0 + Gx * p1], axis=-1).astype(F)
        J[np.isnan(f)] = np.nan
    return f, J


# ---- compute_rgb_Hg's Python (tracker.py:146-172) with float64 sums ------------------------------------------------------------------------
def robust_weight(f, kernel, k):
    f = np.asarray(f, dtype=F)
    if kernel is None:
        return np.ones_like(f)
    k = F(k)
    if kernel == "huber":
        ab = np.abs(f)
        return np.where(ab > k, k / np.where(ab > k, ab, F(1)), F(1)).astype(F)
    if kernel == "tukey":
        r = f / k
        u = F(1) - r * r
        return np.where(np.abs(f) <= k, u * u, F(0)).astype(F)
    raise NotImplementedError(kernel)


def sums_of_flat(f_img, J_img, weight, kernel=None, k=0.0):
    """The term from the flat operator's outputs: (out (44,) float64 = H | g | e | M, S (43,) float64 = the sum of the ABSOLUTE values of every
    entry's terms with the same scale).  Products of float32 factors in double, like the fused kernel; J_img None: energy only."""
    f_img = np.asarray(f_img, dtype=F)
    mask = ~np.isnan(f_img)
    f = f_img[mask]
    M = int(f.size)
    out, S = np.zeros(44), np.zeros(43)
    out[43] = M
    if M == 0:
        return out, S, mask
    w = robust_weight(f, kernel, k)
    wf = (f * w).astype(F)
    scale = 1.0 / M * float(F(weight))
    te = f.astype(np.float64) * wf.astype(np.float64)
    out[42], S[42] = te.sum() * scale, np.abs(te).sum() * scale
    if J_img is not None:
        J = (-np.asarray(J_img, dtype=F)[mask]).astype(F)
        JW = (J * w[:, None]).astype(F).astype(np.float64)
        J64 = J.astype(np.float64)
        for r in range(6):
            for c in range(6):
                tt = JW[:, min(r, c)] * J64[:, max(r, c)]
                out[r * 6 + c], S[r * 6 + c] = tt.sum() * scale, np.abs(tt).sum() * scale
            tg = J64[:, r] * wf.astype(np.float64)
            out[36 + r], S[36 + r] = tg.sum() * scale, np.abs(tg).sum() * scale
    return out, S, mask


def warp_of(intr, R, t):
    """tracker.py:133-137: K R K^-1 and K t in float64, flattened."""
    K = np.array([[intr[0], 0.0, intr[2]], [0.0, intr[1], intr[3]], [0.0, 0.0, 1.0]])
    return (K @ np.asarray(R, dtype=np.float64) @ np.linalg.inv(K)).flatten(), (K @ np.asarray(t, dtype=np.float64)).flatten()


def compute_rgb_hg(prev_pyr, cur_pyr, level, intr, R, t, rgb_args, no_grad=False):
    """`SDFTracker.compute_rgb_Hg` on the restatement: (out, S, mask) of `sums_of_flat`.  prev_pyr / cur_pyr = (Is, Ds, Gs); `intr` is used
    as given at every level (the reference passes the full-resolution calib, tracker.py:135-142)."""
    krkinv, kt = warp_of(intr, R, t)
    f, J = rgb_odometry(prev_pyr[0][level], prev_pyr[1][level], cur_pyr[0][level], cur_pyr[1][level], cur_pyr[2][level], intr, krkinv, kt,
                        rgb_args["min_grad_scale"], rgb_args["max_depth_delta"], not no_grad)
    return sums_of_flat(f, J, rgb_args["weight"], rgb_args["robust_kernel"], rgb_args["robust_k"])
