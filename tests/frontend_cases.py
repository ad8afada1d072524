"""The depth front end (csrc/kernels_points.hip.h: k_depth_frontend, k_normal_weight, k_unproject) and point_box_filter, stated twice
without the product and without oracle/: once in float64 (the statement) and once in float32, operation for operation in the kernel's
order (the restatement), and the cases both run on.  Everything here is NumPy (torch only for the third float32 evaluation that K_FE is
measured with); tests/test_frontend_cpu.py pins it, tests/test_gpu_frontend_envelope.py holds the kernels to it.

WHAT IS STATED (reference: ext/imgproc/imgproc.cu:5-160, system/tracker.py:13-23)
  filter_depth           5x5 bilateral filter on the interior (2 <= v < H-2, 2 <= u < W-2), the border untouched; z < 1e-6 -> 0; neighbours
                         below 1e-6 carry no weight; w = exp(-0.5 ((|i|+|j|) L^2 + (nz-z)^2 sigma_z^2)), sigma_z = 1 / (noise model at z)
  unproject_depth        ((u - cx) / fx * d, (v - cy) / fy * d, d); a NaN depth gives a NaN point (all three components here)
  compute_normal_weight  1 <= v <= H-2, 1 <= u <= W-2; centre z <= 1e-6 or a neighbour z < 1e-6 -> invalid (weight -1, normal unwritten);
                         n = cross(p(v+1) - p(v-1), p(u+1) - p(u-1)), |n| < 1e-6 -> invalid; theta = acos(n_z / |n|),
                         weight = 1 / (0.0012 + 0.0019 (z - 0.4)^2 + 0.0001 / sqrt(z) (theta / (0.5 * 3.14159 - theta))^2)
  frame pair             frame_depth / frame_normal carry the filtered depth and the normal where the pixel is valid, its weight > 0, and
                         neither the normal nor the depth is NaN; NaN elsewhere (the project's own rule: what dif_frame_t takes)
  point_box_filter       boxes of voxel_size on the grid of tracker.py:15-19 (float32: which box a point falls into is a decision),
                         mean point and mean normal per box, boxes in ascending linear id
THRESHOLDS compare the float32 VALUE in double (`z < 1e-6` with a float z and a double literal): float32(1e-6) is below 1e-6.  The
constants are the float32 ones (0.0012f ...), widened; NaN compares false everywhere, so a NaN depth is filtered to NaN, not to 0.

THE CAMERA of a case is a centred H x W crop of a 640 x 480 sensor: the focal length stays (525, 525.5), the principal point follows the
size ((W-1)/2 + 0.25, (H-1)/2 - 0.25).  With that focal length a plane at 0.1 m has |n| = 4 z^2 / (fx fy) = 1.5e-7 < 1e-6 at every stencil.
"""
from __future__ import annotations

import functools

import numpy as np

F32, F64 = np.float32, np.float64
# the float32 constants of imgproc.cu
C_A, C_B, C_Z0, C_C, C_Q, C_HALF, C_PI, C_L = F32(0.0012), F32(0.0019), F32(0.4), F32(0.0001), F32(0.25), F32(0.5), F32(3.14159), F32(1.2232)
TH = 1e-6                       # a double, as in the reference
TH32 = F32(1e-6)                # 9.99999997e-07: below TH

SIZES = [(1, 1), (1, 7), (2, 2), (3, 3), (4, 9), (5, 5), (5, 40), (40, 5), (16, 16), (17, 17), (15, 33), (22, 22), (33, 19), (48, 64)]
SCENES = ["plane", "sphere", "near", "noisy"]
PLANT_VALUES = [F32(np.nan), F32(0.0), F32(-1.0), TH32, np.nextafter(TH32, F32(0)), np.nextafter(TH32, F32(1)), F32(1e-40), F32(np.inf)]
UPPER = np.nextafter(TH32, F32(1))          # the only planted value the thresholds keep as a depth
MARGIN = 1e-3


def spacing32(x):
    return np.spacing(np.abs(np.asarray(x, F64)).astype(F32)).astype(F64)


class Intr:
    def __init__(self, H, W):
        self.fx, self.fy, self.cx, self.cy = 525.0, 525.5, (W - 1) / 2 + 0.25, (H - 1) / 2 - 0.25

    def tuple(self):
        return self.fx, self.fy, self.cx, self.cy


# ---- scenes ------------------------------------------------------------------------------------------------------------------------------
def _rays(H, W, K):
    u, v = np.meshgrid(np.arange(W, dtype=F64), np.arange(H, dtype=F64))
    return (u - K.cx) / K.fx, (v - K.cy) / K.fy


def plane_depth(H, W, K, n, d):
    """depth of the plane n . p = d seen along the rays ((u-cx)/fx, (v-cy)/fy, 1), float64"""
    a, b = _rays(H, W, K)
    return d / (n[0] * a + n[1] * b + n[2])


PLANE_N = np.array([0.35, -0.2, 1.0]) / np.linalg.norm([0.35, -0.2, 1.0])


def scene_depth(scene, H, W, K, seed):
    g = np.random.default_rng(seed)
    if scene == "plane":                                  # tilted plane, ~1.2 m
        z = plane_depth(H, W, K, PLANE_N, 1.2 * PLANE_N[2])
    elif scene == "sphere":                               # a sphere at 1.5 m, about 0.3 max(H, W) pixels in radius, over a wall at 2.5 m: a 1 m depth step
        a, b = _rays(H, W, K)
        wall = plane_depth(H, W, K, np.array([0.1, 0.05, 1.0]) / np.linalg.norm([0.1, 0.05, 1.0]), 2.5)
        c, r = np.array([0.0, 0.0, 1.5]), 1.5 * 0.3 * max(H, W) / K.fx
        d = np.stack([a, b, np.ones_like(a)], -1)
        dd, dc = (d * d).sum(-1), d @ c
        disc = dc * dc - dd * (c @ c - r * r)
        z = np.where(disc > 0, (dc - np.sqrt(np.maximum(disc, 0))) / dd, wall)
    elif scene == "near":                                 # every stencil has |n| ~ 1.5e-7: no pixel is valid
        z = plane_depth(H, W, K, np.array([0.02, 0.01, 1.0]) / np.linalg.norm([0.02, 0.01, 1.0]), 0.1)
    elif scene == "noisy":                                # a slanted wall with the sensor's own noise (sigma of the noise model at z, i.e. ~3 mm at 1.5 m)
        z = plane_depth(H, W, K, np.array([-0.25, 0.3, 1.0]) / np.linalg.norm([-0.25, 0.3, 1.0]), 1.5)
        z = z + g.standard_normal(z.shape) * (0.0012 + 0.0019 * (z - 0.4) ** 2)
    else:
        raise KeyError(scene)
    return z.astype(F32)


def plant_positions(H, W):
    """Where values are planted, in a fixed order: the four corners; one pixel in five on rings 0, 1, H-2, H-1 (rows and columns); on rows
    and columns 13..18 (the seam between tiles 0 and 1 with its 3-pixel apron) one pixel per row of the 6 x 6 crossing, each column once,
    and one pixel in seven along the rest of those rows and columns."""
    pos = []

    def add(v, u):
        if 0 <= v < H and 0 <= u < W and (v, u) not in pos:
            pos.append((v, u))
    for v, u in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        add(v, u)
    for k, r in enumerate((0, 1, H - 2, H - 1)):
        for u in range(2 + k, W, 5):
            add(r, u)
    for k, c in enumerate((0, 1, W - 2, W - 1)):
        for v in range(3 + k, H, 5):
            add(v, c)
    for i in range(6):
        add(13 + i, 13 + (5 * i + 2) % 6)
    for i, r in enumerate(range(13, 19)):
        for u in range(20 + i, W - 2, 7):
            add(r, u)
        for v in range(21 + i, H - 2, 7):
            add(v, r)
    return pos


def plant(depth, shift):
    """-> (depth with the values planted, bool mask of the planted pixels).  The values cycle over the positions, starting at `shift`.
    UPPER (the one value that survives the thresholds) is never planted within two pixels of another UPPER: a filter window that
    holds two of them would average equal values, and the rounding of that average, not the input, would decide `z <= 1e-6`."""
    d, mask = depth.copy(), np.zeros(depth.shape, bool)
    uppers = []
    for k, (v, u) in enumerate(plant_positions(*depth.shape)):
        val = PLANT_VALUES[(k + shift) % len(PLANT_VALUES)]
        if val == UPPER:
            if any(max(abs(v - a), abs(u - b)) <= 2 for a, b in uppers):
                val = TH32
            else:
                uppers.append((v, u))
        d[v, u] = val
        mask[v, u] = True
    return d, mask


class Case:
    def __init__(self, scene, H, W):
        self.scene, self.H, self.W = scene, H, W
        self.K = Intr(H, W)
        self.name = f"{scene}-{H}x{W}"
        si = SCENES.index(scene)
        self.clean = scene_depth(scene, H, W, self.K, 1000 * si + 37 * H + W)
        self.depth, self.planted = plant(self.clean, 3 * si + H + W)


@functools.lru_cache(maxsize=None)
def cases():
    return [Case(s, H, W) for s in SCENES for (H, W) in SIZES]


# ---- the float64 statement ---------------------------------------------------------------------------------------------------------------
def _noise64(z):
    return F64(C_A) + F64(C_B) * (z - F64(C_Z0)) ** 2


def filter64(depth32):
    """filter_depth: float64 arithmetic on the float32 input.  A copy of the input (widened) with the interior filtered."""
    H, W = depth32.shape
    d = depth32.astype(F64)
    out = d.copy()
    ii, jj = np.meshgrid(np.arange(-2, 3), np.arange(-2, 3), indexing="ij")
    dist = (np.abs(ii) + np.abs(jj)).astype(F64) * (F64(C_L) * F64(C_L))
    for v in range(2, H - 2):
        for u in range(2, W - 2):
            z = d[v, u]
            if z < TH:
                out[v, u] = 0.0
                continue
            with np.errstate(all="ignore"):
                sigma_z = 1.0 / (_noise64(z) + F64(C_C) / np.sqrt(z) * F64(C_Q))
                win = d[v - 2:v + 3, u - 2:u + 3]
                w = np.exp(-0.5 * (dist + (win - z) ** 2 * sigma_z * sigma_z))
                keep = ~(win < TH)                          # a NaN neighbour is kept (and poisons the pixel), as in the reference
                out[v, u] = (w[keep] * win[keep]).sum() / w[keep].sum()
    return out


def unproject64(d, K):
    H, W = d.shape
    a, b = _rays(H, W, K)
    with np.errstate(all="ignore"):
        pc = np.stack([a * d, b * d, d], -1)
    pc[np.isnan(d)] = np.nan
    return pc


def normal_weight64(pc):
    """compute_normal_weight -> dict(valid (H,W) bool, normal (H,W,3), weight (H,W), len (H,W)).  weight is -1 and normal 0 where invalid; len is the
    un-normalised normal's length wherever the stencil was evaluated (NaN elsewhere): the quantity the `< 1e-6` test decides on."""
    H, W, _ = pc.shape
    valid = np.zeros((H, W), bool)
    normal, weight, ln = np.zeros((H, W, 3)), np.full((H, W), -1.0), np.full((H, W), np.nan)
    for v in range(1, H - 1):
        for u in range(1, W - 1):
            c, xp, xm, yp, ym = pc[v, u], pc[v, u + 1], pc[v, u - 1], pc[v + 1, u], pc[v - 1, u]
            if c[2] <= TH or xp[2] < TH or xm[2] < TH or yp[2] < TH or ym[2] < TH:
                continue
            with np.errstate(all="ignore"):
                n = np.cross(yp - ym, xp - xm)
                length = np.sqrt((n * n).sum())
                ln[v, u] = length
                if length < TH:
                    continue
                n = n / length
                theta = np.arccos(n[2])
                td = theta / (F64(C_HALF) * F64(C_PI) - theta)
                wgt = _noise64(c[2]) + F64(C_C) / np.sqrt(c[2]) * td * td
                valid[v, u], normal[v, u], weight[v, u] = True, n, 1.0 / wgt
    return dict(valid=valid, normal=normal, weight=weight, len=ln)


def frame_rule(depth, nw):
    with np.errstate(all="ignore"):
        use = nw["valid"] & (nw["weight"] > 0) & ~np.isnan(nw["normal"][..., 0]) & ~np.isnan(depth)
    fd = np.where(use, depth, np.nan)
    fn = np.where(use[..., None], nw["normal"], np.nan)
    return use, fd, fn


def _compose(depth32, K, filt, filter_fn, unproject_fn, nw_fn):
    d = filter_fn(depth32) if filt else depth32.astype(filter_fn.dtype)
    pc = unproject_fn(d, K)
    nw = nw_fn(pc)
    use, fd, fn = frame_rule(d, nw)
    return dict(depth=d, pc=pc, use=use, frame_depth=fd, frame_normal=fn, **nw)


filter64.dtype = F64


def statement(depth32, K, filt):
    """The whole front end in float64: filter (or not) -> unproject -> normal + weight -> frame pair."""
    return _compose(depth32, K, filt, filter64, unproject64, normal_weight64)


# ---- the float32 restatement: the kernel's operations in the kernel's order -------------------------------------------------------------
class _Lib:
    """How a float32 evaluation takes exp / acos / sqrt.  `once`: in float64, rounded once to float32 (the restatement)."""
    def __init__(self, kind):
        self.kind = kind

    def _f(self, name, x):
        x = np.asarray(x, F32)
        with np.errstate(all="ignore"):
            if self.kind == "once":
                return getattr(np, name)(x.astype(F64)).astype(F32)
            if self.kind == "numpy":
                return getattr(np, name)(x)
        import torch
        return getattr(torch, {"arccos": "acos"}.get(name, name))(torch.from_numpy(np.ascontiguousarray(x))).numpy()

    def exp(self, x): return self._f("exp", x)
    def acos(self, x): return self._f("arccos", x)
    def sqrt(self, x): return self._f("sqrt", x)


ONCE = _Lib("once")


def _lt(x, th=TH):
    """`x < 1e-6` as the kernel takes it: the float32 value against the double constant"""
    with np.errstate(all="ignore"):
        return np.asarray(x, F32).astype(F64) < th


def filter32(depth32, lib=ONCE, sequential=True):
    """k_depth_frontend's filter stage: per interior pixel, the 25 neighbours in row-major order, `w_sum += w; acc += w * nz`, every
    operation rounded to float32.  L^2 is the precomputed float32 product.  `sequential=False`: the window sums are taken by the
    library's own reduction instead (an honest float32 evaluation in another order, for K_FE)."""
    H, W = depth32.shape
    out = depth32.astype(F32).copy()
    if H < 5 or W < 5:
        return out
    sl2 = C_L * C_L
    z = depth32[2:H - 2, 2:W - 2].astype(F32)
    with np.errstate(all="ignore"):
        dzc = z - C_Z0
        sigma_z = F32(1.0) / (C_A + C_B * dzc * dzc + C_C / lib.sqrt(z) * C_Q)
        w_sum, acc = np.zeros_like(z), np.zeros_like(z)
        ws, ps = [], []
        for di in range(-2, 3):
            for dj in range(-2, 3):
                nz = depth32[2 + di:H - 2 + di, 2 + dj:W - 2 + dj].astype(F32)
                skip = _lt(nz)
                dz = (nz - z) * (nz - z)
                w = lib.exp(F32(-0.5) * (F32(abs(di) + abs(dj)) * sl2 + dz * sigma_z * sigma_z))
                if sequential:
                    w_sum = np.where(skip, w_sum, w_sum + w)
                    acc = np.where(skip, acc, acc + w * nz)
                else:
                    ws.append(np.where(skip, F32(0), w)); ps.append(np.where(skip, F32(0), w * nz))
        if not sequential:
            if lib.kind == "torch":
                import torch
                w_sum, acc = torch.from_numpy(np.stack(ws, -1)).sum(-1).numpy(), torch.from_numpy(np.stack(ps, -1)).sum(-1).numpy()
            else:
                w_sum, acc = np.stack(ws, -1).sum(-1, dtype=F32), np.stack(ps, -1).sum(-1, dtype=F32)
        out[2:H - 2, 2:W - 2] = np.where(_lt(z), F32(0), acc / w_sum)
    return out


filter32.dtype = F32


def unproject32(d, K):
    """k_unproject / backproject: ((float)u - cx) / fx * d, every operation rounded"""
    H, W = d.shape
    fx, fy, cx, cy = (F32(x) for x in K.tuple())
    u, v = np.arange(W, dtype=F32)[None, :], np.arange(H, dtype=F32)[:, None]
    d = d.astype(F32)
    with np.errstate(all="ignore"):
        pc = np.stack([np.broadcast_to((u - cx) / fx, d.shape) * d, np.broadcast_to((v - cy) / fy, d.shape) * d, d], -1).astype(F32)
    pc[np.isnan(d)] = np.nan
    return pc


def normal_weight32(pc, lib=ONCE):
    """normal_weight_of on every pixel with a stencil; same dict as normal_weight64, float32 values"""
    H, W, _ = pc.shape
    valid = np.zeros((H, W), bool)
    normal, weight, ln = np.zeros((H, W, 3), F32), np.full((H, W), F32(-1)), np.full((H, W), F32(np.nan))
    if H < 3 or W < 3:
        return dict(valid=valid, normal=normal, weight=weight, len=ln)
    pc = pc.astype(F32)
    c, xp, xm, yp, ym = pc[1:-1, 1:-1], pc[1:-1, 2:], pc[1:-1, :-2], pc[2:, 1:-1], pc[:-2, 1:-1]
    with np.errstate(all="ignore"):
        ok = ~(c[..., 2].astype(F64) <= TH) & ~(_lt(xp[..., 2]) | _lt(xm[..., 2]) | _lt(yp[..., 2]) | _lt(ym[..., 2]))
        dxx, dxy, dxz = (xp[..., k] - xm[..., k] for k in range(3))
        dyx, dyy, dyz = (yp[..., k] - ym[..., k] for k in range(3))
        nx, ny, nz = dyy * dxz - dyz * dxy, dyz * dxx - dyx * dxz, dyx * dxy - dyy * dxx          # cross(diff_y, diff_x)
        length = lib.sqrt(nx * nx + ny * ny + nz * nz)
        ln[1:-1, 1:-1] = np.where(ok, length, F32(np.nan))
        ok &= ~_lt(length)
        nx, ny, nz = nx / length, ny / length, nz / length
        theta = lib.acos(nz)
        td = theta / (C_HALF * C_PI - theta)
        cz = c[..., 2]
        wgt = C_A + C_B * (cz - C_Z0) * (cz - C_Z0) + C_C / lib.sqrt(cz) * td * td
        valid[1:-1, 1:-1] = ok
        normal[1:-1, 1:-1] = np.where(ok[..., None], np.stack([nx, ny, nz], -1), F32(0))
        weight[1:-1, 1:-1] = np.where(ok, F32(1.0) / wgt, F32(-1))
    return dict(valid=valid, normal=normal, weight=weight, len=ln)


def restatement(depth32, K, filt, lib=ONCE, sequential=True):
    f = lambda d: filter32(d, lib, sequential)
    f.dtype = F32
    return _compose(depth32, K, filt, f, unproject32, lambda pc: normal_weight32(pc, lib))


@functools.lru_cache(maxsize=None)
def results(i, filt):
    """(statement, restatement) of case i, computed once and shared; callers do not modify them"""
    c = cases()[i]
    return statement(c.depth, c.K, filt), restatement(c.depth, c.K, filt)


# ---- errors and the bar ------------------------------------------------------------------------------------------------------------------
OUTPUTS = ("depth", "normal", "weight")
U_ULP = dict(depth=1.0, normal=0.0, weight=0.0)       # ulps granted for device functions: expf is documented at 1 ulp; nothing else is behind one
# K_FE: twice the largest ratio between the errors of three honest float32 evaluations of the same case and output (the restatement; NumPy
# float32 with its libm and its own window sums; torch CPU float32 likewise), re-measured by test_frontend_cpu.py::test_k_fe and tabulated in
# profiles/frontend_envelope_k.md.  Largest ratios measured: weight 5.61 (near-16x16, filter off: 3.8e-7 / 2.1e-6 / 3.8e-7, nine valid pixels
# next to planted values), normal 4.56 (near-5x40, filter on), depth 3.02 (noisy-40x5).  The worst error of a handful of pixels is partly a
# draw, which is what makes the small cases the largest ratios; the constant is taken over all of them all the same.
K_FE = 11.5


def errors(got, want64):
    """Worst absolute error per output of a float32 evaluation `got` against the statement, over the pixels where the statement has a
    number: depth wherever it is finite, normal and weight on the statement's valid pixels with finite values.  -> (dict output -> error,
    dict output -> largest |value| there)"""
    e, m = {}, {}
    with np.errstate(all="ignore"):
        fin = np.isfinite(want64["depth"])
        e["depth"] = float(np.abs(got["depth"].astype(F64) - want64["depth"])[fin].max()) if fin.any() else 0.0
        m["depth"] = float(np.abs(want64["depth"])[fin].max()) if fin.any() else 0.0
        ok = want64["valid"] & np.isfinite(want64["weight"]) & np.isfinite(want64["normal"]).all(-1)
        e["normal"] = float(np.abs(got["normal"].astype(F64) - want64["normal"])[ok].max()) if ok.any() else 0.0
        m["normal"] = 1.0
        e["weight"] = float(np.abs(got["weight"].astype(F64) - want64["weight"])[ok].max()) if ok.any() else 0.0
        m["weight"] = float(np.abs(want64["weight"])[ok].max()) if ok.any() else 0.0
    return e, m


def bar(e_ref, out_max, output):
    return K_FE * e_ref + U_ULP[output] * float(np.spacing(F32(out_max)))


def in_margin(st):
    """Pixels whose decisions float32 cannot be held to: in the float64 statement `st`, |n| or the filtered z within 1e-3 (relative) of 1e-6,
    or the weight of a valid pixel within the same distance (1e-9) of 0.  (A weight is 1 / (a positive sum): it reaches 0 only when the
    sum overflows, and it falls below 1e-9 only where theta is within a float32 spacing of 0.5f * 3.14159f, where theta / (that - theta)
    has no stable value.  A weight that is merely small, 1e-3 at a grazing normal, is decided as safely as any other.)"""
    with np.errstate(all="ignore"):
        near = lambda x: np.abs(x - TH) <= MARGIN * TH
        return near(st["len"]) | near(st["depth"]) | (st["valid"] & (np.abs(st["weight"]) <= MARGIN * TH))


# ---- point_box_filter -------------------------------------------------------------------------------------------------------------------
def box_ids(points32, voxel_size):
    """tracker.py:15-19 in float32 (the arithmetic that decides a point's box): -> (linear id per point, grid counts)"""
    p, vs = points32.astype(F32), F32(voxel_size)
    mn = p.min(axis=0) - vs * F32(0.5)
    mx = p.max(axis=0) + vs * F32(0.5)
    n = np.floor((mx - mn) / vs).astype(np.int64) + 16
    c = np.floor((p - mn[None]) / vs).astype(np.int64)
    return c[:, 0] + c[:, 1] * n[0] + c[:, 2] * n[0] * n[1], n


def box_filter64(points32, normals32, voxel_size):
    """-> (mean point, mean normal, count) per box in ascending id, float64 means"""
    lin, _ = box_ids(points32, voxel_size)
    ids, inv = np.unique(lin, return_inverse=True)
    cnt = np.bincount(inv, minlength=len(ids))
    sp, sn = np.zeros((len(ids), 3)), np.zeros((len(ids), 3))
    np.add.at(sp, inv, points32.astype(F64)); np.add.at(sn, inv, normals32.astype(F64))
    return sp / cnt[:, None], sn / cnt[:, None], cnt


def box_filter32(points32, normals32, voxel_size):
    """k_pbf_accumulate / k_pbf_finish: every coordinate rounded to the 2^-24 fixed point (round to nearest even), exact integer sums,
    then float32(sum * 2^-24) / float32(count).  -> (mean point, mean normal) float32, boxes in ascending id"""
    lin, _ = box_ids(points32, voxel_size)
    ids, inv = np.unique(lin, return_inverse=True)
    cnt = np.bincount(inv, minlength=len(ids))
    out = []
    for a in (points32, normals32):
        q = np.rint(a.astype(F64) * 16777216.0).astype(np.int64)          # a float32 times 2^24 is exact in double; rint rounds half to even
        s = np.zeros((len(ids), 3), np.int64)
        np.add.at(s, inv, q)
        out.append((s.astype(F64) * (1.0 / 16777216.0)).astype(F32) / cnt[:, None].astype(F32))
    return out[0], out[1]


def box_mean_bound(mean64):
    """2^-25 (each point's rounding to the fixed point; a mean of errors is no larger) + one rounding of the sum to float32 and one
    float32 division: 2^-24 |m| each, compounded"""
    return 2.0 ** -25 + 2.0 ** -23 * np.abs(mean64) * (1.0 + 2.0 ** -24)


def box_cloud(n, seed, voxel_size=0.05, boxes=200):
    """n points on at most `boxes` boxes: box centres on a lattice of 2 * voxel_size (negative coordinates included), points jittered by
    less than a third of a voxel around them; unit normals"""
    g = np.random.default_rng(seed)
    centres = (g.integers(-6, 7, (min(boxes, max(n, 1)), 3)) * 2 + 0.5).astype(F64) * voxel_size
    which = g.integers(0, len(centres), n)
    p = centres[which] + g.uniform(-0.3, 0.3, (n, 3)) * voxel_size
    nr = g.standard_normal((n, 3))
    nr /= np.linalg.norm(nr, axis=1, keepdims=True) + 1e-30
    return p.astype(F32), nr.astype(F32)


def box_cloud_cells_31_32(voxel_size=0.05):
    """Two boxes whose ids are 31 and 32: the last bit of bitmap word 0 and the first of word 1.  The grid's x count is >= 33 + 16, so
    ids 31 and 32 are x cells 31 and 32 of the first row: points at x = 31.5 and 32.5 voxels from the minimum, and one at the far end."""
    vs = voxel_size
    p = np.array([[0.0, 0.0, 0.0], [31.0 * vs, 0.0, 0.0], [31.0 * vs + 0.01 * vs, 0.0, 0.0], [32.0 * vs, 0.0, 0.0], [40.0 * vs, 0.0, 0.0]], F32)
    n = np.tile(np.array([[0.0, 0.6, 0.8]], F32), (len(p), 1))
    return p, n
