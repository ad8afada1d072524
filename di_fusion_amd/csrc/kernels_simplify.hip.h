// Simplifying an indexed mesh by vertex clustering on a grid (dif_mesh_simplify).
// No reference counterpart: the reference leaves this to Open3D (simplify_vertex_clustering), as it does the weld.  DESIGN.md "Simplifying an
// indexed mesh"; the contract is in include/difusion.h.
//
// All cluster arithmetic is double with every operation rounded once (the library is built without contraction); every sum is an integer, so
// the output is a pure function of the input, whatever the schedule.  A cluster is named by its LOWEST MEMBER VERTEX (`rep`): once the insert
// has run, the table is only read to find that name, and everything after is indexed by vertex id.
//
// House rules as in kernels_weld.hip.h: every launch is bounded, nothing spins on or waits for another workgroup, probe loops are bounded by
// the capacity and report instead of looping.  Kernels that count with wave ballots take one thread per element and have no early return;
// those that add up per workgroup take a few elements per thread and have none either.
//
// Chain:
//   k_simplify_insert    vertex -> cell key -> open-addressing table (64-bit CAS), atomicMin of the vertex id per slot (the weld's insert)
//   k_simplify_sums      vertex -> rep (written over its slot); fixed-point position / std / colour sums to the rep's row (64-bit atomicAdd,
//                        per workgroup in LDS first)
//   k_simplify_classify  triangle -> remapped triple, rotated so that its smallest index comes first; bad index / collapsed / a slot in the
//                        triangle table (32-bit CAS claims a slot for a triangle INDEX; an occupied slot is compared by the occupant's triple,
//                        recomputed from `tri` and `rep`, both read-only here; equal: atomicMin, different: probe on.  An occupant only ever
//                        changes to a lower triangle of the same triple, so the comparison holds whichever occupant was seen)
//   k_simplify_mark      kept = the triangle its slot holds; marks the reps of kept triangles as used; counts collapsed and duplicate
//   scan 1               used reps in vertex order -> output vertices; resolves the sums; clears the normal sums
//   k_simplify_clusters  vertex -> output vertex of its rep, or -1; counts the isolated clusters
//   scan 2               kept triangles in input order with remapped indices, their fixed-point area normals (the weld's, scaled by 1 / cell)
//   k_weld_normals       sum -> unit vector, in double
#pragma once

#define SIMPLIFY_EMPTY 0xFFFFFFFFFFFFFFFFull        // (a key uses 63 bits)
#define SIMPLIFY_NO_TRIANGLE 0xFFFFFFFFu
#define SIMPLIFY_AXIS_LIMIT 2097152.0               // 2^21: cell coordinates are packed in 21 bits each
#define SIMPLIFY_POS_ONE 65536.0                    // fixed point of the position inside a cell
#define SIMPLIFY_STD_ONE 16777216.0                 // 2^24, fixed point of the std
#define SIMPLIFY_STD_MAX 64.0
#define SIMPLIFY_WEIGHT_ONE 65536.0                 // the colourer's
#define SIMPLIFY_WEIGHT_MAX 16777216.0              // 2^24 pixels: a larger weight counts as this
#define SIMPLIFY_FLAT_LIMIT 2147483648.0f           // 2^31: a cross component from here on does not fit the fixed-point sums
enum { SIMPLIFY_N_VERTICES = 0, SIMPLIFY_N_TRIANGLES = 1, SIMPLIFY_N_UNKEYED = 2, SIMPLIFY_N_COLLAPSED = 3, SIMPLIFY_N_DUPLICATE = 4,
       SIMPLIFY_N_ISOLATED = 5, SIMPLIFY_N_BAD_STD = 6, SIMPLIFY_N_FLAT = 7, SIMPLIFY_STATUS = 8 };
enum { SIMPLIFY_TRI_BAD = -1, SIMPLIFY_TRI_COLLAPSED = -2, SIMPLIFY_TRI_NO_SLOT = -3 };
enum { SIMPLIFY_SUM_X = 0, SIMPLIFY_SUM_Y = 1, SIMPLIFY_SUM_Z = 2, SIMPLIFY_SUM_N = 3, SIMPLIFY_SUM_STD = 4, SIMPLIFY_SUM_M = 5, SIMPLIFY_SUMS = 6 };
static_assert(SIMPLIFY_N_VERTICES == WELD_N_VERTICES, "k_weld_normals reads the vertex count at the weld's index");

struct SimplifyTable {
    unsigned long long* key;    // [cap]  SIMPLIFY_EMPTY = free
    unsigned* min_vertex;       // [cap]  lowest member of the cluster (cleared to all-ones)
    unsigned mask;              // cap - 1
    int shift;                  // 64 - log2(cap)
};

struct SimplifyTriTable {
    unsigned* tri;              // [cap]  SIMPLIFY_NO_TRIANGLE = free, else the lowest triangle seen so far with the slot's triple
    unsigned mask;
    int shift;
};

struct SimplifyGeo { double ox, oy, oz, cell; };

// One axis: c = floor(t), f = t - c for t = (p - origin) / cell; false when t is not finite or c is outside [0, 2^21).
__device__ __forceinline__ bool simplify_axis(float p, double o, double cell, double& c, double& f) {
    const double t = ((double)p - o) / cell;
    c = floor(t);
    f = t - c;
    return isfinite(t) && c >= 0.0 && c < SIMPLIFY_AXIS_LIMIT;
}

__device__ __forceinline__ bool simplify_cell(const SimplifyGeo& g, const float* p, double c[3], double f[3]) {
    const bool x = simplify_axis(p[0], g.ox, g.cell, c[0], f[0]);
    const bool y = simplify_axis(p[1], g.oy, g.cell, c[1], f[1]);
    const bool z = simplify_axis(p[2], g.oz, g.cell, c[2], f[2]);
    return x && y && z;
}

// One thread per vertex (no grid-stride loop: the wave vote needs every lane).  slot[v] = the cluster's table slot, or -1: a cluster of its own.
__global__ void __launch_bounds__(DIF_BLOCK) k_simplify_insert(SimplifyTable t, SimplifyGeo g, const float* __restrict__ vertices, int V, int* __restrict__ slot,
                                                              int* __restrict__ counts) {
    const int v = (int)(blockIdx.x * DIF_BLOCK + threadIdx.x);
    bool unkeyed = false, full = false;
    if (v < V) {
        double c[3], f[3];
        int s = -1;
        if (simplify_cell(g, vertices + (size_t)v * 3, c, f)) {
            const unsigned long long key = ((unsigned long long)c[0] << 42) | ((unsigned long long)c[1] << 21) | (unsigned long long)c[2];
            unsigned h = (unsigned)((key * 0x9E3779B97F4A7C15ull) >> t.shift);
            // bounded by the capacity: a full table (it cannot be: capacity >= 2 V) ends the loop and is reported, it never spins
            for (unsigned probe = 0; probe <= t.mask; ++probe) {
                unsigned long long prev = __hip_atomic_load(t.key + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (prev == SIMPLIFY_EMPTY) prev = atomicCAS(t.key + h, SIMPLIFY_EMPTY, key);
                if (prev == SIMPLIFY_EMPTY || prev == key) { s = (int)h; break; }
                h = (h + 1) & t.mask;
            }
            full = s < 0;
            // (the minimum only goes down: a vertex that cannot lower it need not touch it — k_weld_insert has the reasoning)
            if (s >= 0 && __hip_atomic_load(t.min_vertex + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > (unsigned)v) atomicMin(t.min_vertex + s, (unsigned)v);
        } else {
            unkeyed = true;
        }
        slot[v] = s;
    }
    const unsigned long long vote = __ballot(unkeyed);
    if (lane_id() == 0 && vote) atomicAdd(counts + SIMPLIFY_N_UNKEYED, __popcll(vote));
    if (full) atomicOr(counts + SIMPLIFY_STATUS, MESH_STATUS_TABLE_FULL);
}

// Sums per workgroup first: a mesh's vertices come in spatial order, so the SIMPLIFY_SUM_ITEMS x DIF_BLOCK consecutive vertices of a workgroup
// fall into few clusters, and one 64-bit atomic per vertex and sum into global memory is what the launch would otherwise cost (49 us for the
// 0.8 million of a 132 k-vertex mesh against 17 us this way, profiles/mesh_simplify.md).  The workgroup adds into a small table in LDS keyed by rep and sends each row out once (CensusTable's scheme, kernels_components.hip.h);
// a rep that finds no room within eight probes goes to global memory directly.  Integer sums: the grouping does not show.
#define SIMPLIFY_SUM_ITEMS 4        // vertices per thread
#define SIMPLIFY_SUM_SLOTS 256
struct SimplifySumTable { int key[SIMPLIFY_SUM_SLOTS]; unsigned long long sum[SIMPLIFY_SUM_SLOTS][SIMPLIFY_SUMS]; };

__device__ __forceinline__ void simplify_sum_put(SimplifySumTable& t, unsigned long long* __restrict__ gsum, int rep, const long long (&x)[SIMPLIFY_SUMS]) {
    unsigned h = ((unsigned)rep * 0x9E3779B1u) >> 24;                // 8 bits
    for (int probe = 0; probe < 8; ++probe) {
        const int prev = atomicCAS(&t.key[h], -1, rep);
        if (prev == -1 || prev == rep) {
#pragma unroll
            for (int k = 0; k < SIMPLIFY_SUMS; ++k)
                if (x[k]) atomicAdd(&t.sum[h][k], (unsigned long long)x[k]);
            return;
        }
        h = (h + 1) & (SIMPLIFY_SUM_SLOTS - 1);
    }
#pragma unroll
    for (int k = 0; k < SIMPLIFY_SUMS; ++k)
        if (x[k]) atomicAdd(gsum + (size_t)rep * SIMPLIFY_SUMS + k, (unsigned long long)x[k]);
}

// SIMPLIFY_SUM_ITEMS vertices per thread, no early return (barriers).  rep[v] (over slot[v]) = the lowest member of v's cluster; v itself
// without a slot.  A keyed vertex adds llrint(f 2^16) per axis and 1 to its rep's row, and its std if that is finite and >= 0 (else it is
// counted); an unkeyed one adds nothing (scan 1 copies it).  Colours, when given, go to the rep's row either way, straight to global memory.
__global__ void __launch_bounds__(DIF_BLOCK) k_simplify_sums(SimplifyTable t, SimplifyGeo g, const float* __restrict__ vertices, const float* __restrict__ vertex_std,
                                                            const uint8_t* __restrict__ rgb8, const float* __restrict__ weight, int V, int* slot_rep,
                                                            unsigned long long* __restrict__ gsum, unsigned long long* __restrict__ csum, int* __restrict__ counts) {
    __shared__ SimplifySumTable table;
    __shared__ int smem[8];
    for (int h = (int)threadIdx.x; h < SIMPLIFY_SUM_SLOTS; h += DIF_BLOCK) {
        table.key[h] = -1;
#pragma unroll
        for (int k = 0; k < SIMPLIFY_SUMS; ++k) table.sum[h][k] = 0;
    }
    __syncthreads();
    int bad_std = 0;
    for (int i = 0; i < SIMPLIFY_SUM_ITEMS; ++i) {
        const long long vv = ((long long)blockIdx.x * SIMPLIFY_SUM_ITEMS + i) * DIF_BLOCK + threadIdx.x;
        if (vv >= V) continue;
        const int v = (int)vv;
        const int s = slot_rep[v];
        const int rep = s < 0 ? v : (int)t.min_vertex[s];
        slot_rep[v] = rep;
        double c[3], f[3];
        if (simplify_cell(g, vertices + (size_t)v * 3, c, f)) {
            long long x[SIMPLIFY_SUMS];
            x[SIMPLIFY_SUM_X] = llrint(f[0] * SIMPLIFY_POS_ONE);
            x[SIMPLIFY_SUM_Y] = llrint(f[1] * SIMPLIFY_POS_ONE);
            x[SIMPLIFY_SUM_Z] = llrint(f[2] * SIMPLIFY_POS_ONE);
            x[SIMPLIFY_SUM_N] = 1;
            const float sd = vertex_std[v];
            const bool ok = isfinite(sd) && sd >= 0.0f;
            x[SIMPLIFY_SUM_STD] = ok ? llrint(fmin((double)sd, SIMPLIFY_STD_MAX) * SIMPLIFY_STD_ONE) : 0;
            x[SIMPLIFY_SUM_M] = ok ? 1 : 0;
            bad_std += ok ? 0 : 1;
            simplify_sum_put(table, gsum, rep, x);
        }
        if (rgb8) {
            const float wf = weight[v];
            const unsigned long long w = isfinite(wf) ? (unsigned long long)llrint(fmin(fmax((double)wf, 0.0), SIMPLIFY_WEIGHT_MAX) * SIMPLIFY_WEIGHT_ONE) : 0ull;
            if (w) {
                unsigned long long* a = csum + (size_t)rep * 4;
                atomicAdd(a + 0, w * rgb8[(size_t)v * 3]);
                atomicAdd(a + 1, w * rgb8[(size_t)v * 3 + 1]);
                atomicAdd(a + 2, w * rgb8[(size_t)v * 3 + 2]);
                atomicAdd(a + 3, w);
            }
        }
    }
    __syncthreads();
    for (int h = (int)threadIdx.x; h < SIMPLIFY_SUM_SLOTS; h += DIF_BLOCK) {
        const int k0 = table.key[h];
        if (k0 < 0) continue;
#pragma unroll
        for (int k = 0; k < SIMPLIFY_SUMS; ++k)
            if (table.sum[h][k]) atomicAdd(gsum + (size_t)k0 * SIMPLIFY_SUMS + k, table.sum[h][k]);
    }
    const int bad = block_sum(bad_std, smem);
    if (threadIdx.x == 0 && bad) atomicAdd(counts + SIMPLIFY_N_BAD_STD, bad);
}

// The remapped triple of a triangle whose indices are in range, rotated so that the smallest comes first (orientation kept).
__device__ __forceinline__ void simplify_triple(const int* __restrict__ tri, const int* __restrict__ rep, int t, int& x, int& y, int& z) {
    const int a = rep[tri[3 * (size_t)t]], b = rep[tri[3 * (size_t)t + 1]], c = rep[tri[3 * (size_t)t + 2]];
    if (a <= b && a <= c) { x = a; y = b; z = c; }
    else if (b <= a && b <= c) { x = b; y = c; z = a; }
    else { x = c; y = a; z = b; }
}

// One thread per triangle.  tri_state[t] = SIMPLIFY_TRI_* or the slot of the triangle's triple.
__global__ void __launch_bounds__(DIF_BLOCK) k_simplify_classify(SimplifyTriTable d, const int* __restrict__ tri, const int* __restrict__ rep, int K, int V,
                                                                int* __restrict__ tri_state, int* __restrict__ counts) {
    const int t = (int)(blockIdx.x * DIF_BLOCK + threadIdx.x);
    if (t >= K) return;
    if (!comp_in_range(tri[3 * (size_t)t], tri[3 * (size_t)t + 1], tri[3 * (size_t)t + 2], V)) {           // never dereferenced
        tri_state[t] = SIMPLIFY_TRI_BAD;
        atomicOr(counts + SIMPLIFY_STATUS, MESH_STATUS_BAD_INDEX);
        return;
    }
    int x, y, z;
    simplify_triple(tri, rep, t, x, y, z);
    if (x == y || y == z || x == z) { tri_state[t] = SIMPLIFY_TRI_COLLAPSED; return; }
    const unsigned long long k = (((unsigned long long)(unsigned)x << 32) | (unsigned long long)(unsigned)y) * 0xD6E8FEB86659FD93ull + (unsigned long long)(unsigned)z;
    unsigned h = (unsigned)((k * 0x9E3779B97F4A7C15ull) >> d.shift);
    int s = SIMPLIFY_TRI_NO_SLOT;
    // bounded by the capacity (>= 2 K: at most half full)
    for (unsigned probe = 0; probe <= d.mask; ++probe) {
        unsigned prev = __hip_atomic_load(d.tri + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (prev == SIMPLIFY_NO_TRIANGLE) prev = atomicCAS(d.tri + h, SIMPLIFY_NO_TRIANGLE, (unsigned)t);
        if (prev == SIMPLIFY_NO_TRIANGLE) { s = (int)h; break; }
        if (prev < (unsigned)K) {                                                                   // (always: only triangle indices are stored)
            int px, py, pz;
            simplify_triple(tri, rep, (int)prev, px, py, pz);
            if (px == x && py == y && pz == z) {
                if (prev > (unsigned)t) atomicMin(d.tri + h, (unsigned)t);
                s = (int)h;
                break;
            }
        }
        h = (h + 1) & d.mask;
    }
    if (s < 0) atomicOr(counts + SIMPLIFY_STATUS, MESH_STATUS_TABLE_FULL);
    tri_state[t] = s;
}

// SIMPLIFY_MARK_ITEMS triangles per thread, no early return (barriers).  tri_state[t] becomes 1 for a kept triangle (the one its slot holds),
// else 0; the reps of a kept triangle are marked as used (every writer stores the same 1: plain stores).  Most triangles collapse, so a count
// per wave would queue K / 64 atomics on one word (about 90 per microsecond, whoever sends them): the workgroup adds up first.
#define SIMPLIFY_MARK_ITEMS 8
__global__ void __launch_bounds__(DIF_BLOCK) k_simplify_mark(SimplifyTriTable d, const int* __restrict__ tri, const int* __restrict__ rep, int K,
                                                            int* __restrict__ tri_state, int* __restrict__ used, int* __restrict__ counts) {
    __shared__ int smem[8];
    int collapsed = 0, duplicate = 0;
    for (int i = 0; i < SIMPLIFY_MARK_ITEMS; ++i) {
        const long long tt = ((long long)blockIdx.x * SIMPLIFY_MARK_ITEMS + i) * DIF_BLOCK + threadIdx.x;
        if (tt >= K) continue;
        const int t = (int)tt;
        const int s = tri_state[t];
        const bool kept = s >= 0 && d.tri[s] == (unsigned)t;
        collapsed += s == SIMPLIFY_TRI_COLLAPSED ? 1 : 0;
        duplicate += (s >= 0 && !kept) ? 1 : 0;
        if (kept) {
#pragma unroll
            for (int j = 0; j < 3; ++j) used[rep[tri[3 * (size_t)t + j]]] = 1;
        }
        tri_state[t] = kept ? 1 : 0;
    }
    const int nc = block_sum(collapsed, smem), nd = block_sum(duplicate, smem);
    if (threadIdx.x == 0 && nc) atomicAdd(counts + SIMPLIFY_N_COLLAPSED, nc);
    if (threadIdx.x == 0 && nd) atomicAdd(counts + SIMPLIFY_N_DUPLICATE, nd);
}

// Scan 1: a vertex that is the lowest member of a used cluster opens an output vertex and resolves the cluster's sums, in exactly the order
// the header states.  A vertex that is not keyed (a cluster of its own) is copied as 32-bit words.
struct SimplifyVertexFunctor {
    SimplifyGeo g;
    const int* rep; const int* used;
    const float* vertices; const float* vertex_std;
    const unsigned long long* gsum; const unsigned long long* csum;
    float* out_vertices; float* out_vertex_std;
    unsigned long long* out_accum;          // or nullptr
    long long* nsum;
    int* cluster_out;
    int* counts;
    __device__ int count(int v) const { return (rep[v] == v && used[v]) ? 1 : 0; }
    __device__ void emit(int v, int n) const {
        cluster_out[v] = n;
        const float* p = vertices + (size_t)v * 3;
        float* o = out_vertices + (size_t)n * 3;
        double c[3], f[3];
        if (simplify_cell(g, p, c, f)) {
            const long long* a = (const long long*)(gsum + (size_t)v * SIMPLIFY_SUMS);
            const double members = (double)a[SIMPLIFY_SUM_N], origin[3] = {g.ox, g.oy, g.oz};
#pragma unroll
            for (int k = 0; k < 3; ++k) o[k] = (float)(origin[k] + (c[k] + ((double)a[k] / members) / SIMPLIFY_POS_ONE) * g.cell);
            const long long m = a[SIMPLIFY_SUM_M];
            out_vertex_std[n] = m > 0 ? (float)(((double)a[SIMPLIFY_SUM_STD] / (double)m) / SIMPLIFY_STD_ONE) : __int_as_float(0x7FC00000);
        } else {
            const unsigned* pw = (const unsigned*)p;
            unsigned* ow = (unsigned*)o;
            ow[0] = pw[0]; ow[1] = pw[1]; ow[2] = pw[2];
            ((unsigned*)out_vertex_std)[n] = ((const unsigned*)vertex_std)[v];
        }
        long long* ns = nsum + (size_t)n * 3;
        ns[0] = 0; ns[1] = 0; ns[2] = 0;
        if (out_accum) {
#pragma unroll
            for (int k = 0; k < 4; ++k) out_accum[(size_t)n * 4 + k] = csum[(size_t)v * 4 + k];
        }
    }
    __device__ void finish(int total) const { counts[SIMPLIFY_N_VERTICES] = total; }
};

// One thread per vertex, no early return (vote).  cluster_out is written for used reps only, so it is read for them only.
__global__ void __launch_bounds__(DIF_BLOCK) k_simplify_clusters(const int* __restrict__ rep, const int* __restrict__ used, const int* __restrict__ cluster_out, int V,
                                                                int* __restrict__ vertex_cluster, int* __restrict__ counts) {
    const int v = (int)(blockIdx.x * DIF_BLOCK + threadIdx.x);
    bool isolated = false;
    if (v < V) {
        const int r = rep[v];
        const bool u = used[r] != 0;
        vertex_cluster[v] = u ? cluster_out[r] : -1;
        isolated = r == v && !u;
    }
    const unsigned long long vote = __ballot(isolated);
    if (lane_id() == 0 && vote) atomicAdd(counts + SIMPLIFY_N_ISOLATED, __popcll(vote));
}

// Scan 2: the kept triangles in input order, corners in their input order, and their normals as WeldTriangleFunctor adds them, with the
// edges in cells (s = 1.0f / cell).  A cross component that is not finite or reaches 2^31 would not fit the sums: such a triangle stays in
// the mesh, adds nothing and is counted (rare: a plain atomic).
struct SimplifyTriangleFunctor {
    const int* tri_state; const int* tri; const int* rep; const int* cluster_out;
    const int64_t* tri_id;
    const float* out_vertices;
    int32_t* out_triangles; int64_t* out_triangle_id;
    long long* nsum;
    float s;
    int* counts;
    __device__ int count(int t) const { return tri_state[t]; }
    __device__ void emit(int t, int k) const {
        const int v0 = cluster_out[rep[tri[3 * (size_t)t]]], v1 = cluster_out[rep[tri[3 * (size_t)t + 1]]], v2 = cluster_out[rep[tri[3 * (size_t)t + 2]]];
        int32_t* o = out_triangles + (size_t)k * 3;
        o[0] = v0; o[1] = v1; o[2] = v2;
        out_triangle_id[k] = tri_id[t];
        const float* p0 = out_vertices + (size_t)v0 * 3; const float* p1 = out_vertices + (size_t)v1 * 3; const float* p2 = out_vertices + (size_t)v2 * 3;
        const float ax = (p1[0] - p0[0]) * s, ay = (p1[1] - p0[1]) * s, az = (p1[2] - p0[2]) * s;
        const float bx = (p2[0] - p0[0]) * s, by = (p2[1] - p0[1]) * s, bz = (p2[2] - p0[2]) * s;
        const float cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
        if (!(fabsf(cx) < SIMPLIFY_FLAT_LIMIT && fabsf(cy) < SIMPLIFY_FLAT_LIMIT && fabsf(cz) < SIMPLIFY_FLAT_LIMIT)) {        // (NaN fails)
            atomicAdd(counts + SIMPLIFY_N_FLAT, 1);
            return;
        }
        const long long nx = weld_fixed(cx), ny = weld_fixed(cy), nz = weld_fixed(cz);
        const int vs[3] = {v0, v1, v2};
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            unsigned long long* a = (unsigned long long*)(nsum + (size_t)vs[j] * 3);
            atomicAdd(a + 0, (unsigned long long)nx);
            atomicAdd(a + 1, (unsigned long long)ny);
            atomicAdd(a + 2, (unsigned long long)nz);
        }
    }
    __device__ void finish(int total) const { counts[SIMPLIFY_N_TRIANGLES] = total; }
};
