// Indexed mesh from the triangle soup of the mesh cache (dif_mesh_weld): weld by LATTICE EDGE, area-weighted vertex normals.
// No reference counterpart: the reference leaves this to Open3D (merge_close_vertices / compute_vertex_normals, commented out in its main loop).
//
// Why not by position: one lattice edge is edge 0 of one cell and edge 2 of its neighbour, its end points come in reversed order, and
// w2 / 1 - w2 round differently (mc_interp / mc_vertex, kernels_mesh.hip.h) — the copies of a vertex differ in the last bit, and a weld on a
// quantisation grid straddles grid lines.  The blended corner values are the same on both sides of a voxel face (mc_corner), so WHICH lattice
// edge carries a vertex is a global name for it: the key is (lattice point of the edge's low end, axis), or (lattice point, 3) for a vertex
// that sits on a lattice corner (the early-outs of mc_interp).  DESIGN.md "Indexed mesh".
//
// Chain (every launch is bounded, nothing spins, nothing waits for another workgroup):
//   k_weld_insert    corner -> key -> open-addressing table (64-bit CAS, probe loop bounded by the capacity), atomicMin of the corner index per slot
//   scan 1           representatives (lowest corner index of a class) in soup order -> vertex ids; copies position and std; clears the normal sums
//   k_weld_triangles corner -> vertex id
//   scan 2           triangles without a repeated index, in soup order; their fixed-point area normals go to the three vertices (64-bit atomics:
//                    integer sums, so the result does not depend on the order)
//   k_weld_normals   sum -> unit vector, in double
#pragma once

#define WELD_EMPTY 0xFFFFFFFFFFFFFFFFull          // (a key uses 62 bits)
#define WELD_TOL 0.0009765625f                    // 2^-10 of a cell
#define WELD_KEY_LIMIT 1048576.0f                 // 2^20: lattice coordinates are packed in 20 bits each
#define WELD_FIXED 1073741824.0                   // 2^30, the fixed point of k_groupby_sum
enum { WELD_N_VERTICES = 0, WELD_N_KEPT = 1, WELD_N_DROPPED = 2, WELD_N_UNKEYED = 3, WELD_STATUS = 4 };
enum { WELD_STATUS_TABLE_FULL = 1 };

struct WeldTable {
    unsigned long long* key;    // [cap]  WELD_EMPTY = free
    unsigned* min_corner;       // [cap]  lowest soup corner of the class (cleared to all-ones)
    int* vertex;                // [cap]  the class's output vertex (written by scan 1)
    unsigned mask;              // cap - 1
    int shift;                  // 64 - log2(cap)
};

struct WeldGeo { float bx, by, bz, vs, r; };

// lattice coordinate of one axis: L, its nearest integer and the distance to it
__device__ __forceinline__ void weld_axis(float p, float b, float vs, float r, float& L, float& q, float& f) {
    L = normalize1(p, b, vs) * r;
    q = rintf(L);
    f = fabsf(L - q);
}

// Key of a soup corner, or false: not on the lattice (another resolution, NaN / inf, outside the 20-bit range) — such a corner is welded to nothing.
__device__ __forceinline__ bool weld_key(const WeldGeo& g, float x, float y, float z, unsigned long long& key) {
    float Lx, Ly, Lz, qx, qy, qz, fx, fy, fz;
    weld_axis(x, g.bx, g.vs, g.r, Lx, qx, fx);
    weld_axis(y, g.by, g.vs, g.r, Ly, qy, fy);
    weld_axis(z, g.bz, g.vs, g.r, Lz, qz, fz);
    int a = 0;                                                   // the axis with the largest distance; ties go to the lowest axis
    float fa = fx;
    if (fy > fa) { a = 1; fa = fy; }
    if (fz > fa) { a = 2; fa = fz; }
    const float o1 = a == 0 ? fy : fx, o2 = a == 2 ? fy : fz;    // the other two
    if (!(o1 < WELD_TOL && o2 < WELD_TOL)) return false;         // (NaN fails)
    const bool corner = fa < WELD_TOL;
    if (!corner) {
        if (a == 0) qx = floorf(Lx);
        else if (a == 1) qy = floorf(Ly);
        else qz = floorf(Lz);
    }
    if (!(qx >= 0.0f && qx < WELD_KEY_LIMIT && qy >= 0.0f && qy < WELD_KEY_LIMIT && qz >= 0.0f && qz < WELD_KEY_LIMIT)) return false;
    key = ((unsigned long long)(unsigned)(int)qx << 42) | ((unsigned long long)(unsigned)(int)qy << 22) | ((unsigned long long)(unsigned)(int)qz << 2) |
          (unsigned long long)(corner ? 3 : a);
    return true;
}

// One thread per soup corner (no grid-stride loop: the wave votes below need every lane).  slot[i] = the class's table slot, or -1: own vertex.
// Neighbouring corners of a soup are neighbouring lattice edges, and the hash scatters them over the whole table on purpose: a table of 6 T
// slots is at most half full, so a probe sequence is 1.5 slots long on average, and the CAS / atomicMin are resolved in L2 (one 64-byte line per
// probe whatever the hash is — there is no locality to win inside a line of eight keys that would be worth clustering for).
__global__ void __launch_bounds__(DIF_BLOCK) k_weld_insert(WeldTable t, WeldGeo g, const float* __restrict__ tri, int n, int* __restrict__ slot,
                                                          int* __restrict__ counts) {
    const int i = (int)(blockIdx.x * DIF_BLOCK + threadIdx.x);
    bool unkeyed = false, full = false;
    if (i < n) {
        const float* p = tri + (size_t)i * 3;
        unsigned long long key;
        int s = -1;
        if (weld_key(g, p[0], p[1], p[2], key)) {
            unsigned h = (unsigned)((key * 0x9E3779B97F4A7C15ull) >> t.shift);
            // bounded by the capacity: a full table (it cannot be: capacity >= 2 x corners) ends the loop and is reported, it never spins
            for (unsigned probe = 0; probe <= t.mask; ++probe) {
                unsigned long long prev = __hip_atomic_load(t.key + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (prev == WELD_EMPTY) prev = atomicCAS(t.key + h, WELD_EMPTY, key);
                if (prev == WELD_EMPTY || prev == key) { s = (int)h; break; }
                h = (h + 1) & t.mask;
            }
            full = s < 0;
            // the minimum only ever goes down: a corner that cannot lower it need not touch it (a class of thousands — every corner the same
            // point — would otherwise queue thousands of atomics on one address)
            if (s >= 0 && __hip_atomic_load(t.min_corner + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > (unsigned)i) atomicMin(t.min_corner + s, (unsigned)i);
        } else {
            unkeyed = true;
        }
        slot[i] = s;
    }
    const unsigned long long vote = __ballot(unkeyed);
    if (lane_id() == 0 && vote) atomicAdd(counts + WELD_N_UNKEYED, __popcll(vote));
    if (full) atomicOr(counts + WELD_STATUS, WELD_STATUS_TABLE_FULL);
}

// Scan 1: corner i opens a vertex if it is its class's lowest corner (or has no class).  An own-vertex corner keeps its vertex id in slot[i] as
// -2 - id (still negative: count() stays 1 for it in every pass).
struct WeldVertexFunctor {
    WeldTable t;
    int* slot;
    const float* tri; const float* tri_std;
    float* vertices; float* vertex_std;
    long long* nsum;
    int* counts;
    __device__ int count(int i) const {
        const int s = slot[i];
        return (s < 0 || t.min_corner[s] == (unsigned)i) ? 1 : 0;
    }
    __device__ void emit(int i, int v) const {
        const int s = slot[i];
        if (s < 0) slot[i] = -2 - v; else t.vertex[s] = v;
        const float* p = tri + (size_t)i * 3;
        float* o = vertices + (size_t)v * 3;
        o[0] = p[0]; o[1] = p[1]; o[2] = p[2];
        vertex_std[v] = tri_std[i];
        long long* a = nsum + (size_t)v * 3;
        a[0] = 0; a[1] = 0; a[2] = 0;
    }
    __device__ void finish(int total) const { counts[WELD_N_VERTICES] = total; }
};

__global__ void __launch_bounds__(DIF_BLOCK) k_weld_triangles(WeldTable t, const int* __restrict__ slot, int n, int* __restrict__ corner_vertex) {
    const int i = (int)(blockIdx.x * DIF_BLOCK + threadIdx.x);
    if (i >= n) return;
    const int s = slot[i];
    corner_vertex[i] = s < 0 ? -2 - s : t.vertex[s];
}

__device__ __forceinline__ long long weld_fixed(float c) { return llrint((double)c * WELD_FIXED); }

// Scan 2: triangles with three different vertices, in soup order, and their normals.  e1, e2 in lattice units (a cell = 1), so the 2^-30 fixed
// point resolves a cell's triangle to 30 bits whatever the voxel size is; the cross product is three (mul, mul, sub) in float32, each rounded
// once (no contraction), each component converted exactly — the per-vertex sums are integers and come out the same in any order.
struct WeldTriangleFunctor {
    const int* corner_vertex;
    const int64_t* tri_id;
    const float* vertices;
    int32_t* triangles; int64_t* triangle_id;
    long long* nsum;
    float s;                    // lattice units per world unit
    int T;
    int* counts;
    __device__ int count(int t) const {
        const int a = corner_vertex[3 * (size_t)t], b = corner_vertex[3 * (size_t)t + 1], c = corner_vertex[3 * (size_t)t + 2];
        return ((a | b | c) >= 0 && a != b && b != c && a != c) ? 1 : 0;        // (every corner has a vertex after scan 1; a negative one would index out of bounds)
    }
    __device__ void emit(int t, int k) const {
        const int v0 = corner_vertex[3 * (size_t)t], v1 = corner_vertex[3 * (size_t)t + 1], v2 = corner_vertex[3 * (size_t)t + 2];
        int32_t* o = triangles + (size_t)k * 3;
        o[0] = v0; o[1] = v1; o[2] = v2;
        triangle_id[k] = tri_id[t];
        const float* p0 = vertices + (size_t)v0 * 3; const float* p1 = vertices + (size_t)v1 * 3; const float* p2 = vertices + (size_t)v2 * 3;
        const float ax = (p1[0] - p0[0]) * s, ay = (p1[1] - p0[1]) * s, az = (p1[2] - p0[2]) * s;
        const float bx = (p2[0] - p0[0]) * s, by = (p2[1] - p0[1]) * s, bz = (p2[2] - p0[2]) * s;
        const long long nx = weld_fixed(ay * bz - az * by), ny = weld_fixed(az * bx - ax * bz), nz = weld_fixed(ax * by - ay * bx);
        const int vs[3] = {v0, v1, v2};
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            unsigned long long* a = (unsigned long long*)(nsum + (size_t)vs[j] * 3);       // (two's complement: the unsigned add is the signed one)
            atomicAdd(a + 0, (unsigned long long)nx);
            atomicAdd(a + 1, (unsigned long long)ny);
            atomicAdd(a + 2, (unsigned long long)nz);
        }
    }
    __device__ void finish(int total) const { counts[WELD_N_KEPT] = total; counts[WELD_N_DROPPED] = T - total; }
};

// sum -> unit normal, in double (the sums pass 2^24); a vertex no kept triangle touches gets (0, 0, 0)
__global__ void __launch_bounds__(DIF_BLOCK) k_weld_normals(const long long* __restrict__ nsum, const int* __restrict__ counts, float* __restrict__ normals) {
    const int v = (int)(blockIdx.x * DIF_BLOCK + threadIdx.x);
    if (v >= counts[WELD_N_VERTICES]) return;
    const double x = (double)nsum[(size_t)v * 3], y = (double)nsum[(size_t)v * 3 + 1], z = (double)nsum[(size_t)v * 3 + 2];
    const double len = sqrt((x * x + y * y) + z * z);
    float* o = normals + (size_t)v * 3;
    o[0] = len > 0.0 ? (float)(x / len) : 0.0f;
    o[1] = len > 0.0 ? (float)(y / len) : 0.0f;
    o[2] = len > 0.0 ? (float)(z / len) : 0.0f;
}
