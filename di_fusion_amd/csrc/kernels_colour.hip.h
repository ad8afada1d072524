// Vertex colours of an indexed mesh from RGB keyframes (dif_mesh_colour_view, dif_mesh_colour_resolve).  DESIGN.md "Colouring an indexed mesh".
// No reference counterpart: the reference keeps no colour in its map.
//
// Visibility is the rasteriser's own (kernels_raster.hip.h: projection, the two walks, the 64-bit atomicMin z-buffer); behind it ONE new kernel
// splats every pixel's colour onto the three vertices of the triangle that won the pixel, weighted by the perspective-correct barycentrics of
// k_raster_resolve times cos^2 of the angle between the blended normal and the view ray.  The weights are rounded to 1/65536 and the colours to
// 8 bits BEFORE they are summed, so the sums are integers: the order of pixels, views and waves cannot show, and tests/colour_ref.py restates
// the result in numpy bit for bit.  The float arithmetic is written out operation by operation (-ffp-contract=off), in double.
//
// Every pixel falls into exactly one class, tested in this order: NO_HIT, BAD_COLOUR, DEPTH, EDGE, GRAZING, USED (difusion.h).
// House rules as in kernels_raster.hip.h: bounded launches, nothing spins, no LDS, no early return before the wave votes.
//   k_colour_splat    per pixel: class, then up to twelve 64-bit atomicAdd (three vertices x (w r, w g, w b, w)); counts the classes
//   k_colour_resolve  per vertex: round-to-nearest integer division of the sums, weight; counts the vertices coloured
#pragma once

#define COLOUR_WEIGHT_ONE 65536.0                 // fixed point of a weight: b_k cos^2 <= 1 -> w_k <= 2^16, w_k q <= 2^16 * 255 < 2^24

struct ColourGates { float depth_tol, min_cos2; int edge; };

// Is the z-buffer word of the neighbour (i, j) — inside the image — empty, or its depth further than tol from d?
__device__ __forceinline__ bool colour_step(const unsigned long long* __restrict__ zbuf, int i, int j, int W, float d, float tol) {
    const unsigned long long w = zbuf[(size_t)j * W + i];
    if (w == RASTER_EMPTY) return true;
    const float dn = __uint_as_float((unsigned)(w >> 32));
    return fabsf(dn - d) > tol;
}

// One thread per pixel, no early return (the votes).  Behind the kernel boundary nobody writes the z-buffer: plain loads.
__global__ void __launch_bounds__(DIF_BLOCK) k_colour_splat(const unsigned long long* __restrict__ zbuf, const int* __restrict__ tri, int K, int V,
                                                           const RasterVertex* __restrict__ pv, const float* __restrict__ normals,
                                                           const float* __restrict__ rgb, const float* __restrict__ depth_in, RasterCam cam,
                                                           ColourGates g, const int* __restrict__ raster_counts, unsigned long long* accum,
                                                           int* __restrict__ counts) {
    const long long p = (long long)blockIdx.x * DIF_BLOCK + threadIdx.x;
    const long long npix = (long long)cam.H * cam.W;
    int cls = -1;
    if (p < npix) {
        cls = DIF_COLOUR_NO_HIT;
        const unsigned long long word = zbuf[p];
        const unsigned t = (unsigned)word;
        if (word != RASTER_EMPTY && t < (unsigned)K) {
            const int a = tri[3 * (size_t)t], b = tri[3 * (size_t)t + 1], c = tri[3 * (size_t)t + 2];
            RasterSetup s;
            if (comp_in_range(a, b, c, V) && raster_setup(pv, a, b, c, cam.H, cam.W, cam.cull != 0, s) == RASTER_OK) {
                const int j = (int)(p / cam.W), i = (int)(p - (long long)j * cam.W);
                const float d = __uint_as_float((unsigned)(word >> 32));
                const float cr = rgb[p * 3], cg = rgb[p * 3 + 1], cb = rgb[p * 3 + 2];
                bool stop = false;
                if (!(isfinite(cr) && isfinite(cg) && isfinite(cb))) { cls = DIF_COLOUR_BAD_COLOUR; stop = true; }
                if (!stop && depth_in) {
                    const float din = depth_in[p];
                    if (!isfinite(din) || fabsf(din - d) > g.depth_tol) { cls = DIF_COLOUR_DEPTH; stop = true; }
                }
                if (!stop && g.edge) {
                    bool e = false;
                    if (i > 0) e = e || colour_step(zbuf, i - 1, j, cam.W, d, g.depth_tol);
                    if (i + 1 < cam.W) e = e || colour_step(zbuf, i + 1, j, cam.W, d, g.depth_tol);
                    if (j > 0) e = e || colour_step(zbuf, i, j - 1, cam.W, d, g.depth_tol);
                    if (j + 1 < cam.H) e = e || colour_step(zbuf, i, j + 1, cam.W, d, g.depth_tol);
                    if (e) { cls = DIF_COLOUR_EDGE; stop = true; }
                }
                if (!stop) {
                    long long E[3];
                    raster_cover(s, i, j, E);
                    const double sum = raster_s(s, E);
                    const double bk[3] = {((double)E[0] * s.iz[0]) / sum, ((double)E[1] * s.iz[1]) / sum, ((double)E[2] * s.iz[2]) / sum};
                    const int vk[3] = {a, s.swapped ? c : b, s.swapped ? b : c};
                    const float* n0 = normals + (size_t)vk[0] * 3; const float* n1 = normals + (size_t)vk[1] * 3; const float* n2 = normals + (size_t)vk[2] * 3;
                    const double nx = (bk[0] * (double)n0[0] + bk[1] * (double)n1[0]) + bk[2] * (double)n2[0];
                    const double ny = (bk[0] * (double)n0[1] + bk[1] * (double)n1[1]) + bk[2] * (double)n2[1];
                    const double nz = (bk[0] * (double)n0[2] + bk[1] * (double)n1[2]) + bk[2] * (double)n2[2];
                    // the view ray through the pixel centre, turned into the mesh's frame: R^T (rx, ry, 1), column k of the world-to-camera rotation
                    const double rx = ((double)i - (double)cam.cx) / (double)cam.fx, ry = ((double)j - (double)cam.cy) / (double)cam.fy;
                    const double dx = ((double)cam.r[0] * rx + (double)cam.r[4] * ry) + (double)cam.r[8];
                    const double dy = ((double)cam.r[1] * rx + (double)cam.r[5] * ry) + (double)cam.r[9];
                    const double dz = ((double)cam.r[2] * rx + (double)cam.r[6] * ry) + (double)cam.r[10];
                    const double nd = (nx * dx + ny * dy) + nz * dz;
                    const double nn = (nx * nx + ny * ny) + nz * nz;
                    const double dd = (dx * dx + dy * dy) + dz * dz;
                    const double cos2 = (nd * nd) / (nn * dd);                  // no sign: the normals are not turned towards the camera
                    if (!(nn > 0.0) || !isfinite(cos2) || cos2 < (double)g.min_cos2) {
                        cls = DIF_COLOUR_GRAZING;
                    } else {
                        cls = DIF_COLOUR_USED;
                        const unsigned long long qr = (unsigned long long)rint(fmin(fmax((double)cr, 0.0), 1.0) * 255.0);
                        const unsigned long long qg = (unsigned long long)rint(fmin(fmax((double)cg, 0.0), 1.0) * 255.0);
                        const unsigned long long qb = (unsigned long long)rint(fmin(fmax((double)cb, 0.0), 1.0) * 255.0);
#pragma unroll
                        for (int k = 0; k < 3; ++k) {
                            const unsigned long long w = (unsigned long long)rint((bk[k] * cos2) * COLOUR_WEIGHT_ONE);
                            if (w == 0) continue;
                            unsigned long long* o = accum + (size_t)vk[k] * 4;
                            atomicAdd(o, w * qr); atomicAdd(o + 1, w * qg); atomicAdd(o + 2, w * qb); atomicAdd(o + 3, w);
                        }
                    }
                }
            }
        }
    }
    const int lane = lane_id();
#pragma unroll
    for (int k = DIF_COLOUR_USED; k <= DIF_COLOUR_GRAZING; ++k) {
        const unsigned long long vote = __ballot(cls == k);
        if (lane == 0 && vote) atomicAdd(counts + k, __popcll(vote));
    }
    if (p == 0) counts[DIF_COLOUR_STATUS] = raster_counts[RASTER_STATUS];       // (k_raster_triangles raised it; nobody else writes this word)
}

// One thread per vertex, no early return (the vote).
__global__ void __launch_bounds__(DIF_BLOCK) k_colour_resolve(const unsigned long long* __restrict__ accum, int V, unsigned long long min_weight,
                                                             unsigned char* __restrict__ rgb8, float* __restrict__ weight, int* __restrict__ counts) {
    const long long v = (long long)blockIdx.x * DIF_BLOCK + threadIdx.x;
    bool coloured = false;
    if (v < V) {
        const unsigned long long* a = accum + (size_t)v * 4;
        const unsigned long long S = a[3];
        unsigned char r = 128, g = 128, b = 128;
        coloured = S >= (min_weight > 1ull ? min_weight : 1ull);
        if (coloured) {
            r = (unsigned char)((2ull * a[0] + S) / (2ull * S));
            g = (unsigned char)((2ull * a[1] + S) / (2ull * S));
            b = (unsigned char)((2ull * a[2] + S) / (2ull * S));
        }
        rgb8[v * 3] = r; rgb8[v * 3 + 1] = g; rgb8[v * 3 + 2] = b;
        weight[v] = (float)((double)S / COLOUR_WEIGHT_ONE);
    }
    const unsigned long long vote = __ballot(coloured);
    if (lane_id() == 0 && vote) atomicAdd(counts, __popcll(vote));
}
