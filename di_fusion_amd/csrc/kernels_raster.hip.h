// Depth, normal, std and triangle-index images of an indexed mesh seen from a camera pose (dif_mesh_render).
// No reference counterpart: the reference shows its mesh through Open3D.  DESIGN.md "Rendering an indexed mesh".
//
// Coverage is decided in INTEGERS on a 1/256-pixel grid, the z-buffer is a 64-bit atomicMin of (depth bits, triangle index): every output is a pure
// function of the input, whatever the schedule, and tests/raster_ref.py restates it in numpy bit for bit.  The float arithmetic is written out
// operation by operation (the library is built with -ffp-contract=off): float32 for the projection, double for the depth and the attributes.
//
// Pixel convention = k_unproject (kernels_points.hip.h): pixel (u, v) is column and row, its centre sits at integer coordinates, x = (u - cx) / fx * z.
// No near-plane clipping: a triangle with a vertex at or behind z_near (or a non-finite one, or one that projects beyond 2^22 sub-pixels) vanishes
// as a whole.  Normals stay in the mesh's frame and are not turned towards the camera.
//
// House rules as in kernels_weld.hip.h: every launch is bounded, nothing spins, nothing waits for another workgroup, no host round trip.
// Chain:
//   k_raster_project    per vertex: camera point, snapped screen position, 1 / z in double; the same launch resets the z-buffer to all-ones
//   k_raster_triangles  per triangle: drops (bad index, clipped, degenerate, culled, off screen), then walks a box of at most
//                       RASTER_THREAD_PIXELS pixels itself, or appends the triangle to the list of large ones
//   k_raster_large      fixed grid, one workgroup per list entry (grid-stride; the length is read on the device), the threads stride the box
//   k_raster_resolve    per pixel: winning word -> depth, barycentric std and normal, triangle index; counts the pixels hit
#pragma once

#define RASTER_SUB 256                            // sub-pixel positions per pixel
#define RASTER_GUARD 4194304.0f                   // 2^22: snapped coordinates stay below it, so every edge function fits 2^47
#define RASTER_EMPTY 0xFFFFFFFFFFFFFFFFull
#define RASTER_THREAD_PIXELS DIF_RASTER_THREAD_PIXELS     // the largest box a single thread walks (difusion.h; _lib.RASTER_THREAD_PIXELS)
#define RASTER_LARGE_BLOCKS 2048                  // grid of k_raster_large
enum { RASTER_PIXELS_HIT = 0, RASTER_DRAWN = 1, RASTER_CLIPPED = 2, RASTER_DEGENERATE = 3, RASTER_CULLED = 4, RASTER_OFFSCREEN = 5, RASTER_LARGE = 6,
       RASTER_STATUS = 7 };

struct RasterCam { float r[12]; float fx, fy, cx, cy, z_near; int H, W, cull; };

// A projected vertex.  iz = 1 / z > 0 for a valid vertex; iz = 0 IS the invalid flag (X, Y are 0 then).
struct __attribute__((aligned(16))) RasterVertex { int X, Y; double iz; };

// A triangle ready to be walked: oriented so that area2 > 0 (vertices 1 and 2 swapped if need be: `swapped`), pixel box clipped to the image.
struct RasterSetup {
    int X[3], Y[3];
    double iz[3];
    long long area2;
    int i0, i1, j0, j1;       // columns i0..i1, rows j0..j1 (may be empty)
    bool swapped;
};

enum { RASTER_OK = 0, RASTER_DROP_CLIPPED = 1, RASTER_DROP_DEGENERATE = 2, RASTER_DROP_CULLED = 3 };

// Orientation and box of a triangle whose three indices are in range.  The ONE setup of all three consumers (thread walk, large walk, resolve).
__device__ __forceinline__ int raster_setup(const RasterVertex* __restrict__ pv, int a, int b, int c, int H, int W, bool cull, RasterSetup& s) {
    const RasterVertex v0 = pv[a], v1 = pv[b], v2 = pv[c];
    if (!(v0.iz > 0.0 && v1.iz > 0.0 && v2.iz > 0.0)) return RASTER_DROP_CLIPPED;
    const long long area2 = (long long)(v1.X - v0.X) * (long long)(v2.Y - v0.Y) - (long long)(v2.X - v0.X) * (long long)(v1.Y - v0.Y);
    if (area2 == 0) return RASTER_DROP_DEGENERATE;
    // area2 > 0  <=>  cross(p1 - p0, p2 - p0) . p0 > 0 in the camera frame (z > 0 for all three): that normal points away from the camera
    if (cull && area2 > 0) return RASTER_DROP_CULLED;
    s.swapped = area2 < 0;
    s.area2 = s.swapped ? -area2 : area2;
    s.X[0] = v0.X; s.Y[0] = v0.Y; s.iz[0] = v0.iz;
    s.X[1] = s.swapped ? v2.X : v1.X; s.Y[1] = s.swapped ? v2.Y : v1.Y; s.iz[1] = s.swapped ? v2.iz : v1.iz;
    s.X[2] = s.swapped ? v1.X : v2.X; s.Y[2] = s.swapped ? v1.Y : v2.Y; s.iz[2] = s.swapped ? v1.iz : v2.iz;
    const int xmin = min(v0.X, min(v1.X, v2.X)), xmax = max(v0.X, max(v1.X, v2.X));
    const int ymin = min(v0.Y, min(v1.Y, v2.Y)), ymax = max(v0.Y, max(v1.Y, v2.Y));
    // pixel centres 256 i inside [min, max]: ceil and floor by arithmetic shifts (|X| < 2^22: no overflow)
    s.i0 = max((xmin + (RASTER_SUB - 1)) >> 8, 0); s.i1 = min(xmax >> 8, W - 1);
    s.j0 = max((ymin + (RASTER_SUB - 1)) >> 8, 0); s.j1 = min(ymax >> 8, H - 1);
    return RASTER_OK;
}

// Edge function of the directed edge p -> q at the pixel centre (px, py), and whether the pixel passes it (top-left rule).
__device__ __forceinline__ bool raster_edge(int Xp, int Yp, int Xq, int Yq, long long px, long long py, long long& E) {
    const long long dx = (long long)Xq - Xp, dy = (long long)Yq - Yp;
    E = dx * (py - Yp) - dy * (px - Xp);
    return E >= ((dy < 0 || (dy == 0 && dx > 0)) ? 0 : 1);
}

// Coverage of pixel (i, j); E[k] belongs to vertex k (the edge opposite to it): v1->v2, v2->v0, v0->v1.  E0 + E1 + E2 == area2.
__device__ __forceinline__ bool raster_cover(const RasterSetup& s, int i, int j, long long (&E)[3]) {
    const long long px = (long long)RASTER_SUB * i, py = (long long)RASTER_SUB * j;
    const bool c0 = raster_edge(s.X[1], s.Y[1], s.X[2], s.Y[2], px, py, E[0]);
    const bool c1 = raster_edge(s.X[2], s.Y[2], s.X[0], s.Y[0], px, py, E[1]);
    const bool c2 = raster_edge(s.X[0], s.Y[0], s.X[1], s.Y[1], px, py, E[2]);
    return c0 && c1 && c2;
}

// sum of E_k / z_k: area2 / s is the perspective-correct z
__device__ __forceinline__ double raster_s(const RasterSetup& s, const long long (&E)[3]) {
    return ((double)E[0] * s.iz[0] + (double)E[1] * s.iz[1]) + (double)E[2] * s.iz[2];
}

// One pixel of one triangle: coverage, depth, z-buffer.  The thread walk and the large walk both go through here.
// The word only ever goes down: a pixel that cannot lower it sends no atomic (a surface behind another costs loads).
__device__ __forceinline__ void raster_pixel(const RasterSetup& s, int i, int j, int W, unsigned t, unsigned long long* zbuf) {
    long long E[3];
    if (!raster_cover(s, i, j, E)) return;
    const float d = (float)((double)s.area2 / raster_s(s, E));
    const unsigned long long word = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned long long)t;
    unsigned long long* z = zbuf + ((size_t)j * W + i);
    if (__hip_atomic_load(z, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > word) atomicMin(z, word);
}

// One thread per vertex, and per z-buffer word (the grid covers the larger of the two).
__global__ void __launch_bounds__(DIF_BLOCK) k_raster_project(const float* __restrict__ vertices, int V, RasterCam cam, RasterVertex* __restrict__ pv,
                                                             unsigned long long* __restrict__ zbuf, int npix) {
    const long long i = (long long)blockIdx.x * DIF_BLOCK + threadIdx.x;
    if (i < npix) zbuf[i] = RASTER_EMPTY;
    if (i >= V) return;
    const float x = vertices[i * 3], y = vertices[i * 3 + 1], z = vertices[i * 3 + 2];
    const float pcx = ((cam.r[0] * x + cam.r[1] * y) + cam.r[2] * z) + cam.r[3];
    const float pcy = ((cam.r[4] * x + cam.r[5] * y) + cam.r[6] * z) + cam.r[7];
    const float pcz = ((cam.r[8] * x + cam.r[9] * y) + cam.r[10] * z) + cam.r[11];
    RasterVertex o{0, 0, 0.0};
    if (isfinite(pcx) && isfinite(pcy) && isfinite(pcz) && pcz > cam.z_near) {
        const float sx = rintf((cam.fx * (pcx / pcz) + cam.cx) * (float)RASTER_SUB);
        const float sy = rintf((cam.fy * (pcy / pcz) + cam.cy) * (float)RASTER_SUB);
        if (fabsf(sx) < RASTER_GUARD && fabsf(sy) < RASTER_GUARD) {           // (NaN fails; the casts below are exact)
            o.X = (int)sx; o.Y = (int)sy; o.iz = 1.0 / (double)pcz;
        }
    }
    pv[i] = o;
}

// One thread per triangle, no early return (the wave votes need every lane).
__global__ void __launch_bounds__(DIF_BLOCK) k_raster_triangles(const int* __restrict__ tri, int K, int V, const RasterVertex* __restrict__ pv, int H, int W,
                                                               int cull, unsigned long long* zbuf, int* __restrict__ large_list, int* __restrict__ counts) {
    const long long t = (long long)blockIdx.x * DIF_BLOCK + threadIdx.x;
    bool bad = false, clipped = false, degenerate = false, culled = false, offscreen = false, drawn = false, large = false;
    if (t < K) {
        const int a = tri[3 * (size_t)t], b = tri[3 * (size_t)t + 1], c = tri[3 * (size_t)t + 2];
        if (!comp_in_range(a, b, c, V)) {
            bad = true;                                                         // never dereferenced
        } else {
            RasterSetup s;
            const int r = raster_setup(pv, a, b, c, H, W, cull != 0, s);
            clipped = r == RASTER_DROP_CLIPPED; degenerate = r == RASTER_DROP_DEGENERATE; culled = r == RASTER_DROP_CULLED;
            if (r == RASTER_OK) {
                offscreen = s.i0 > s.i1 || s.j0 > s.j1;
                drawn = !offscreen;
                if (drawn) {
                    large = (long long)(s.i1 - s.i0 + 1) * (long long)(s.j1 - s.j0 + 1) > RASTER_THREAD_PIXELS;
                    if (!large)
                        for (int j = s.j0; j <= s.j1; ++j)
                            for (int i = s.i0; i <= s.i1; ++i) raster_pixel(s, i, j, W, (unsigned)t, zbuf);
                }
            }
        }
    }
    const int lane = lane_id();
    const bool flags[5] = {drawn, clipped, degenerate, culled, offscreen};
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const unsigned long long vote = __ballot(flags[k]);
        if (lane == 0 && vote) atomicAdd(counts + RASTER_DRAWN + k, __popcll(vote));
    }
    // one reservation per wave; the list's order does not matter (the result is a minimum); at most K entries: each triangle appends once
    const unsigned long long vl = __ballot(large);
    if (vl) {
        const int leader = __builtin_ctzll(vl);
        int base = 0;
        if (lane == leader) base = atomicAdd(counts + RASTER_LARGE, __popcll(vl));
        base = __shfl(base, leader);
        if (large) large_list[base + __popcll(vl & ((1ull << lane) - 1ull))] = (int)t;
    }
    if (bad) atomicOr(counts + RASTER_STATUS, MESH_STATUS_BAD_INDEX);
}

// Fixed grid; workgroup g takes list entries g, g + gridDim.x, ...  (block-uniform loop: no barrier inside, nothing waits).
__global__ void __launch_bounds__(DIF_BLOCK) k_raster_large(const int* __restrict__ tri, int K, int V, const RasterVertex* __restrict__ pv, int H, int W, int cull,
                                                           unsigned long long* zbuf, const int* __restrict__ large_list, const int* __restrict__ counts) {
    const int n = min(counts[RASTER_LARGE], K);
    for (int e = (int)blockIdx.x; e < n; e += (int)gridDim.x) {
        const int t = large_list[e];
        if ((unsigned)t >= (unsigned)K) continue;
        const int a = tri[3 * (size_t)t], b = tri[3 * (size_t)t + 1], c = tri[3 * (size_t)t + 2];
        if (!comp_in_range(a, b, c, V)) continue;                               // (k_raster_triangles lists no such triangle)
        RasterSetup s;
        if (raster_setup(pv, a, b, c, H, W, cull != 0, s) != RASTER_OK || s.i0 > s.i1 || s.j0 > s.j1) continue;
        const long long bw = s.i1 - s.i0 + 1, npx = bw * (long long)(s.j1 - s.j0 + 1);          // <= H W < 2^31
        for (long long p = threadIdx.x; p < npx; p += DIF_BLOCK) {
            const int dj = (int)(p / bw);
            raster_pixel(s, s.i0 + (int)(p - dj * bw), s.j0 + dj, W, (unsigned)t, zbuf);
        }
    }
}

// One thread per pixel, no early return (the vote).  Behind the kernel boundary nobody writes the z-buffer: plain loads.
__global__ void __launch_bounds__(DIF_BLOCK) k_raster_resolve(const unsigned long long* __restrict__ zbuf, const int* __restrict__ tri, int K, int V,
                                                             const RasterVertex* __restrict__ pv, const float* __restrict__ normals,
                                                             const float* __restrict__ vertex_std, int H, int W, int cull, float* __restrict__ depth,
                                                             float* __restrict__ normal, float* __restrict__ std_out, int* __restrict__ triangle,
                                                             int* __restrict__ counts) {
    const long long p = (long long)blockIdx.x * DIF_BLOCK + threadIdx.x;
    const long long npix = (long long)H * W;
    bool hit = false;
    if (p < npix) {
        const float qnan = __builtin_nanf("");
        float d = qnan, sd = qnan, nx = 0.0f, ny = 0.0f, nz = 0.0f;
        int tid = -1;
        const unsigned long long word = zbuf[p];
        const unsigned t = (unsigned)word;
        if (word != RASTER_EMPTY && t < (unsigned)K) {
            const int a = tri[3 * (size_t)t], b = tri[3 * (size_t)t + 1], c = tri[3 * (size_t)t + 2];
            RasterSetup s;
            if (comp_in_range(a, b, c, V) && raster_setup(pv, a, b, c, H, W, cull != 0, s) == RASTER_OK) {
                const int j = (int)(p / W), i = (int)(p - (long long)j * W);
                long long E[3];
                raster_cover(s, i, j, E);
                const double sum = raster_s(s, E);
                const double b0 = ((double)E[0] * s.iz[0]) / sum, b1 = ((double)E[1] * s.iz[1]) / sum, b2 = ((double)E[2] * s.iz[2]) / sum;
                const int v0 = a, v1 = s.swapped ? c : b, v2 = s.swapped ? b : c;
                hit = true;
                tid = (int)t;
                d = __uint_as_float((unsigned)(word >> 32));
                sd = (float)((b0 * (double)vertex_std[v0] + b1 * (double)vertex_std[v1]) + b2 * (double)vertex_std[v2]);
                const float* n0 = normals + (size_t)v0 * 3; const float* n1 = normals + (size_t)v1 * 3; const float* n2 = normals + (size_t)v2 * 3;
                const double x = (b0 * (double)n0[0] + b1 * (double)n1[0]) + b2 * (double)n2[0];
                const double y = (b0 * (double)n0[1] + b1 * (double)n1[1]) + b2 * (double)n2[1];
                const double z = (b0 * (double)n0[2] + b1 * (double)n1[2]) + b2 * (double)n2[2];
                const double len = sqrt((x * x + y * y) + z * z);
                if (len > 0.0 && isfinite(len)) { nx = (float)(x / len); ny = (float)(y / len); nz = (float)(z / len); }
            }
        }
        depth[p] = d; std_out[p] = sd; triangle[p] = tid;
        normal[p * 3] = nx; normal[p * 3 + 1] = ny; normal[p * 3 + 2] = nz;
    }
    const unsigned long long vote = __ballot(hit);
    if (lane_id() == 0 && vote) atomicAdd(counts + RASTER_PIXELS_HIT, __popcll(vote));
}
