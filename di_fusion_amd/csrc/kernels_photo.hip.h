// The photometric term of the tracker's Gauss-Newton step — reference ext/imgproc/photometric.cu (gradient_xy_kernel, evaluate_fJ),
// tracker.py:41-56 (_make_image_pyramid), tracker.py:131-172 (SDFTracker.compute_rgb_Hg)
//
//   I_l, D_l, G_l = pyramid(mean(rgb), depth)                      tracker.py:83-85, 41-56       k_photo_level (one launch per level)
//   f, J = rgb_odometry(prev_I, prev_D, cur_I, cur_D, cur_G, ...)     tracker.py:139-145            k_rgb_odometry (the flat operator)
//   mask = !isnan(f) ; J = -J[mask] ; w = robust(f) ; Wf = f w ; JW = J w       tracker.py:152-163
//   H = sum JW (x) J s ; g = sum J Wf s ; e = sum f Wf s ; s = weight / M       tracker.py:165-172
//
// The reference spends one kernel that writes an (H, W) residual image and an (H, W, 6) Jacobian image, a boolean compaction of both, about a
// dozen torch launches and three host round trips per evaluation.  k_rgb_hg is the whole term in ONE launch: nothing per pixel is stored,
// the 44 numbers come back through pinned host memory (the reduction tree and the hand-back of k_sdf_hg_reduce: hg_finish).
//
// Every per-pixel quantity is float32 in the order written here (the library is built with -ffp-contract=off; the divisions are __fdiv_rn),
// shared between the flat operator and the fused kernel: tests/photo_ref.py restates it in numpy and reproduces it bit for bit.
#pragma once

struct PhotoArgs {
    float k[9];          // K R K^-1, row-major
    float kt[3];         // K t
    float fx, fy, cx, cy;
    float min_grad, max_dd;
    int robust;          // 0 none, 1 huber, 2 tukey (on f)
    float rk;
    int no_grad;
    double weight;       // the term's weight (tracker.py:165)
};

// ---- gradient_xy (photometric.cu:3-22) ---------------------------------------------------------------------------------------------------
// (d1 + 2 d2 + d3) / 8, left to right; rows of the 3x3 neighbourhood: n[i][j] = I[v - 1 + i][u - 1 + j]
__device__ __forceinline__ void sobel_of(const float (&n)[3][3], float& gx, float& gy) {
    const float u1 = n[0][2] - n[0][0], u2 = n[1][2] - n[1][0], u3 = n[2][2] - n[2][0];
    gx = __fdiv_rn((u1 + 2.0f * u2) + u3, 8.0f);
    const float v1 = n[2][0] - n[0][0], v2 = n[2][1] - n[0][1], v3 = n[2][2] - n[0][2];
    gy = __fdiv_rn((v1 + 2.0f * v2) + v3, 8.0f);
}

__global__ void __launch_bounds__(DIF_BLOCK) k_gradient_xy(const float* __restrict__ I, float* __restrict__ G, int H, int W) {
    const int64_t n = (int64_t)H * W;
    for (int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; m < n; m += (int64_t)gridDim.x * blockDim.x) {
        const int v = (int)(m / W), u = (int)(m % W);
        float gx = __builtin_nanf(""), gy = gx;
        if (!(v < 1 || v > H - 2 || u < 1 || u > W - 2)) {
            float nb[3][3];
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) nb[i][j] = I[(int64_t)(v - 1 + i) * W + (u - 1 + j)];
            sobel_of(nb, gx, gy);
        }
        G[m * 2] = gx; G[m * 2 + 1] = gy;
    }
}

// ---- the pyramid (tracker.py:41-56, 83) ------------------------------------------------------------------------------------------------------
// One launch per level: level 0 reads the colour image (intensity = ((r + g) + b) / 3: torch.mean's order on three elements) and copies the
// depth; level l + 1 reads level l (bilinear intensity, nearest depth: torch.nn.functional.interpolate, align_corners = False).  The 16 x 16
// intensity tile and its 1-pixel apron go through LDS, the Sobel stencil reads them there: the gradient is that of the intensities this
// launch writes, bit for bit.
struct PhotoLevelArgs {
    const float* rgb;            // level 0: (H, W, 3); nullptr on the other levels, and on level 0 when the caller brings the intensity (src_I == I)
    const float* src_I;          // level l > 0: level l - 1's intensity (Hs, Ws)
    const float* src_D;          // the depth to copy (level 0, Hs == H) or to resize
    int Hs, Ws, H, W;
    float sh, sw;                // (float)Hs / H, (float)Ws / W: torch's area_pixel_compute_scale
    float* I; float* D; float* G;
};

__device__ __forceinline__ float photo_level_intensity(const PhotoLevelArgs& a, int y, int x) {
    if (a.rgb) {
        const float* p = a.rgb + ((int64_t)y * a.W + x) * 3;
        return __fdiv_rn((p[0] + p[1]) + p[2], 3.0f);
    }
    if (a.src_I == a.I) return a.src_I[(int64_t)y * a.W + x];
    // source index max(scale (dst + 0.5) - 0.5, 0), weights 1 - l and l, rows of (columns of): with scale == 2 both weights are exactly 0.5
    const float fy = fmaxf(a.sh * ((float)y + 0.5f) - 0.5f, 0.0f), fx = fmaxf(a.sw * ((float)x + 0.5f) - 0.5f, 0.0f);
    const int y0 = min((int)fy, a.Hs - 1), x0 = min((int)fx, a.Ws - 1);
    const int y1 = y0 + (y0 < a.Hs - 1 ? 1 : 0), x1 = x0 + (x0 < a.Ws - 1 ? 1 : 0);
    const float ly = fminf(fmaxf(fy - (float)y0, 0.0f), 1.0f), lx = fminf(fmaxf(fx - (float)x0, 0.0f), 1.0f), my = 1.0f - ly, mx = 1.0f - lx;
    const float a00 = a.src_I[(int64_t)y0 * a.Ws + x0], a01 = a.src_I[(int64_t)y0 * a.Ws + x1];
    const float a10 = a.src_I[(int64_t)y1 * a.Ws + x0], a11 = a.src_I[(int64_t)y1 * a.Ws + x1];
    return my * (mx * a00 + lx * a01) + ly * (mx * a10 + lx * a11);
}

__global__ void __launch_bounds__(FE_TILE * FE_TILE) k_photo_level(PhotoLevelArgs a) {
    __shared__ float tile[FE_FIL][FE_FIL + 1];
    const int u0 = (int)blockIdx.x * FE_TILE, v0 = (int)blockIdx.y * FE_TILE, t = (int)threadIdx.x;
    const float qnan = __builtin_nanf("");
    for (int k = t; k < FE_FIL * FE_FIL; k += FE_TILE * FE_TILE) {
        const int i = k / FE_FIL, j = k % FE_FIL, v = v0 - 1 + i, u = u0 - 1 + j;
        tile[i][j] = (v >= 0 && v < a.H && u >= 0 && u < a.W) ? photo_level_intensity(a, v, u) : qnan;
    }
    __syncthreads();
    const int lx = t & (FE_TILE - 1), ly = t / FE_TILE, u = u0 + lx, v = v0 + ly;
    if (u >= a.W || v >= a.H) return;
    const int64_t px = (int64_t)v * a.W + u;
    if (a.src_I != a.I) a.I[px] = tile[ly + 1][lx + 1];
    // nearest: source index floor(dst * scale), clamped (level 0: scale == 1, a copy)
    const int ys = min((int)floorf((float)v * a.sh), a.Hs - 1), xs = min((int)floorf((float)u * a.sw), a.Ws - 1);
    a.D[px] = a.src_D[(int64_t)ys * a.Ws + xs];
    float gx = qnan, gy = qnan;
    if (!(v < 1 || v > a.H - 2 || u < 1 || u > a.W - 2)) {
        float nb[3][3];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) nb[i][j] = tile[ly + i][lx + j];
        sobel_of(nb, gx, gy);
    }
    a.G[px * 2] = gx; a.G[px * 2 + 1] = gy;
}

// ---- evaluate_fJ (photometric.cu:24-77), in three steps so that the fused kernel can issue the loads of two pixels together ------------------
// The reference rounds the warp target with CUDA's __float2int_rn, whose result for a non-finite argument is DEFINED there: NaN -> 0, beyond
// the int range -> the nearest int.  A warped depth of 0 makes the quotient +-inf (target outside the image: the pixel is invalid) or NaN
// (0 / 0: target column / row 0, a pixel like any other — it then has to pass the depth test against a warped depth of 0).  The same here,
// written out, because a float -> int conversion of such a value is undefined in C++.
__device__ __forceinline__ int photo_rn(float q) {
    if (q != q) return 0;
    if (q >= 2147483648.0f) return 2147483647;
    if (q <= -2147483648.0f) return -2147483647 - 1;
    return (int)rintf(q);
}

struct PhotoPix {
    float gx, gy, d1, ci;        // streamed: the current frame at (v, u)
    float wd;                    // warped depth
    int u0, v0;                  // warp target in the previous frame (u0: column, v0: row)
    bool cand;                   // the target is inside the image
    float d0, pi;                // gathered: the previous frame at (v0, u0)

    __device__ __forceinline__ void stream(int64_t m, const float* __restrict__ cur_I, const float* __restrict__ cur_D, const float* __restrict__ cur_G) {
        const float2 g = ((const float2*)cur_G)[m];
        gx = g.x; gy = g.y; d1 = cur_D[m]; ci = cur_I[m];
    }
    __device__ __forceinline__ void target(const PhotoArgs& a, int u, int v, int H, int W) {
        cand = false;
        const float mTwo = (gx * gx) + (gy * gy);
        if (mTwo < a.min_grad || mTwo != mTwo) return;
        if (d1 != d1) return;
        const float fu = (float)(unsigned)u, fv = (float)(unsigned)v;
        wd = d1 * ((a.k[6] * fu + a.k[7] * fv) + a.k[8]) + a.kt[2];
        u0 = photo_rn(__fdiv_rn(d1 * ((a.k[0] * fu + a.k[1] * fv) + a.k[2]) + a.kt[0], wd));
        v0 = photo_rn(__fdiv_rn(d1 * ((a.k[3] * fu + a.k[4] * fv) + a.k[5]) + a.kt[1], wd));
        cand = u0 >= 0 && u0 < W && v0 >= 0 && v0 < H;
    }
    __device__ __forceinline__ void gather(const float* __restrict__ prev_I, const float* __restrict__ prev_D, int W) {
        d0 = 0.0f; pi = 0.0f;
        if (cand) { const int64_t p = (int64_t)v0 * W + u0; d0 = prev_D[p]; pi = prev_I[p]; }
    }
    // the residual; NaN: not a valid pair (a NaN intensity on either side too: the reference's mask is !isnan(f), tracker.py:152)
    __device__ __forceinline__ float residual(const PhotoArgs& a) const {
        if (!cand || d0 != d0 || !(fabsf(wd - d0) <= a.max_dd) || !(d0 > 0.0f)) return __builtin_nanf("");
        return ci - pi;
    }
    // d f / d xi as the reference's kernel writes it (tracker.py:157 negates it)
    __device__ __forceinline__ void jacobian(const PhotoArgs& a, float (&J)[6]) const {
        const float Gx = __fdiv_rn(d0 * ((float)u0 - a.cx), a.fx), Gy = __fdiv_rn(d0 * ((float)v0 - a.cy), a.fy), Gz = d0;
        const float p0 = __fdiv_rn(gx * a.fx, Gz), p1 = __fdiv_rn(gy * a.fy, Gz);
        const float p2 = __fdiv_rn(-(p0 * Gx + p1 * Gy), Gz);
        J[0] = p0; J[1] = p1; J[2] = p2;
        J[3] = (-Gz) * p1 + Gy * p2;
        J[4] = Gz * p0 - Gx * p2;
        J[5] = (-Gy) * p0 + Gx * p1;
    }
};

// the flat operator: f_img (H, W), NaN where invalid; J_img (H, W, 6) if asked, NaN where f is (the reference leaves those rows unwritten)
__global__ void __launch_bounds__(DIF_BLOCK) k_rgb_odometry(int H, int W, const float* __restrict__ prev_I, const float* __restrict__ prev_D,
                                                          const float* __restrict__ cur_I, const float* __restrict__ cur_D,
                                                          const float* __restrict__ cur_G, PhotoArgs a, float* __restrict__ f_img, float* __restrict__ J_img) {
    const int64_t n = (int64_t)H * W;
    for (int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; m < n; m += (int64_t)gridDim.x * blockDim.x) {
        PhotoPix p;
        p.stream(m, cur_I, cur_D, cur_G);
        p.target(a, (int)(m % W), (int)(m / W), H, W);
        p.gather(prev_I, prev_D, W);
        const float f = p.residual(a);
        f_img[m] = f;
        if (!J_img) continue;
        float J[6];
        if (f == f) p.jacobian(a, J);
        else {
#pragma unroll
            for (int j = 0; j < 6; ++j) J[j] = f;
        }
#pragma unroll
        for (int j = 0; j < 6; ++j) J_img[m * 6 + j] = J[j];
    }
}

__device__ __forceinline__ void photo_accumulate(double* acc, const PhotoArgs& a, const PhotoPix& p) {
    const float f = p.residual(a);
    if (f != f) return;
    acc[28] += 1.0;
    float w = 1.0f;
    if (a.robust == 1) {
        const float ab = fabsf(f);
        if (ab > a.rk) w = __fdiv_rn(a.rk, ab);
    } else if (a.robust == 2) {
        w = 0.0f;
        if (fabsf(f) <= a.rk) {
            const float r = __fdiv_rn(f, a.rk), u = 1.0f - r * r;
            w = u * u;
        }
    }
    const float wf = f * w;
    acc[27] += (double)f * (double)wf;
    if (a.no_grad) return;
    float J[6];
    p.jacobian(a, J);
#pragma unroll
    for (int r = 0; r < 6; ++r) J[r] = -J[r];
    int t = 0;
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        const double jw = (double)(J[r] * w);
#pragma unroll
        for (int c = r; c < 6; ++c) acc[t++] += jw * (double)J[c];
    }
#pragma unroll
    for (int r = 0; r < 6; ++r) acc[21 + r] += (double)J[r] * (double)wf;
}

// The whole term.  Reads per pixel: cur_I, cur_D, cur_G streamed (16 bytes), prev_D and prev_I gathered at the warp target (neighbouring pixels
// land on neighbouring targets for the small motions of a tracker).  Two pixels per thread and trip, the streamed loads of both issued
// together, then both gathers.  Sums in double in the fixed tree of k_sdf_hg_reduce, scaled by weight / M.
__global__ void __launch_bounds__(DIF_BLOCK) k_rgb_hg(int H, int W, const float* __restrict__ prev_I, const float* __restrict__ prev_D,
                                                    const float* __restrict__ cur_I, const float* __restrict__ cur_D, const float* __restrict__ cur_G,
                                                    PhotoArgs a, double* partial, int* ticket, double* out, double* out_host, int64_t seq) {
    double acc[HG_TERMS];
#pragma unroll
    for (int t = 0; t < HG_TERMS; ++t) acc[t] = 0.0;
    const int N = H * W, stride = (int)(gridDim.x * blockDim.x);
    for (int m = (int)(blockIdx.x * blockDim.x + threadIdx.x); m < N; m += 2 * stride) {
        const int m1 = m + stride < N ? m + stride : m;
        PhotoPix p0, p1;
        p0.stream(m, cur_I, cur_D, cur_G);
        p1.stream(m1, cur_I, cur_D, cur_G);
        p0.target(a, m % W, m / W, H, W);
        p1.target(a, m1 % W, m1 / W, H, W);
        p0.gather(prev_I, prev_D, W);
        p1.gather(prev_I, prev_D, W);
        photo_accumulate(acc, a, p0);
        if (m1 != m) photo_accumulate(acc, a, p1);
    }
    hg_finish<true>(acc, partial, ticket, out, out_host, seq, a.weight);
}
