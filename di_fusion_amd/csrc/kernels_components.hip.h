// Connected components, selection and edge census of an indexed mesh (dif_mesh_components, dif_mesh_select, dif_mesh_edge_census).
// No reference counterpart: the reference leaves this to Open3D, as it does the weld.  DESIGN.md "Components of an indexed mesh".
//
// All integer: every output is a pure function of the input, whatever the schedule.  Components are numbered in ascending order of their LOWEST
// VERTEX ID; a vertex no triangle names is a component of its own; a triangle with an index outside [0, V) joins nothing and gets component -1.
//
// House rules as in kernels_weld.hip.h: every launch is bounded, nothing spins on or waits for another workgroup, and a loop that could in
// principle run away carries an iteration bound, sets a status bit and leaves.
//
// Components chain:
//   k_comp_init      parent[v] = v
//   k_comp_hook      per triangle a lock-free union of (a, b) and (a, c), a few consecutive triangles per thread.  Every access to `parent` in this
//                    launch is an agent-scope atomic (relaxed load or CAS) — see comp_union.
//   k_comp_flatten   parent is read-only from here on: chase it to the root, write label[v]
//   scan             roots (label[v] == v) in vertex order -> component ids; clears the two per-component counts
//   k_comp_vertices  vertex -> component, vertices per component
//   k_comp_triangles triangle -> component, triangles per component
// Select chain:      k_select_mark, vertex scan (copies attributes, writes the remap), triangle scan (remaps indices, copies ids)
// Edge census chain: k_edge_insert (64-bit CAS table of undirected edges, uses per slot), k_edge_slots (per-component edges / boundary edges, max use)
#pragma once

#define EDGE_EMPTY 0xFFFFFFFFFFFFFFFFull          // (a key uses 62 bits)
enum { COMP_N = 0, COMP_STATUS = 1 };
enum { SELECT_N_VERTICES = 0, SELECT_N_TRIANGLES = 1, SELECT_STATUS = 2 };
enum { EDGE_MAX_USE = 0, EDGE_STATUS = 1 };
enum { MESH_STATUS_BAD_INDEX = 1, MESH_STATUS_RUNAWAY = 2, MESH_STATUS_TABLE_FULL = 4 };

__device__ __forceinline__ bool comp_in_range(int a, int b, int c, int V) {
    return (unsigned)a < (unsigned)V && (unsigned)b < (unsigned)V && (unsigned)c < (unsigned)V;
}

// Per-component counts: all triangles of one giant component add to ONE address, and one word takes about 90 atomics per microsecond on this chip
// whoever sends them (a launch of one atomic per wave is bound by exactly that; the weld's min_corner comment has the reasoning).  So a workgroup
// counts its chunk (several elements per thread) in a small table in LDS, keyed by component, and sends each entry out once at the end
// (census_flush); a component that finds no room within eight probes goes to global memory directly.  On the way in, the lanes of a wave that
// share the lowest active lane's component go as ONE add (a wave inside a giant component: one LDS atomic instead of 64 on one address).
// Integer counts, so the order does not matter.  Every lane of a wave must call census_add (votes); `n1` counts a second property (boundary edges) for dst1 — where nothing has one, dst1 = dst0.
#define CENSUS_ITEMS 8          // elements per thread (vertices, triangles)
#define CENSUS_SLOT_ITEMS 32    // table slots per thread: half of them are free, and nothing else is done per slot
#define CENSUS_TABLE 128

struct CensusTable { int key[CENSUS_TABLE]; int n0[CENSUS_TABLE]; int n1[CENSUS_TABLE]; };

__device__ __forceinline__ void census_clear(CensusTable& t) {
    for (int h = (int)threadIdx.x; h < CENSUS_TABLE; h += DIF_BLOCK) { t.key[h] = -1; t.n0[h] = 0; t.n1[h] = 0; }
    __syncthreads();
}

__device__ __forceinline__ void census_put(CensusTable& t, int* dst0, int* dst1, int c, int a0, int a1) {
    unsigned h = ((unsigned)c * 0x9E3779B1u) >> 25;                  // 7 bits
    for (int probe = 0; probe < 8; ++probe) {
        const int prev = atomicCAS(&t.key[h], -1, c);
        if (prev == -1 || prev == c) {
            atomicAdd(&t.n0[h], a0);
            if (a1) atomicAdd(&t.n1[h], a1);
            return;
        }
        h = (h + 1) & (CENSUS_TABLE - 1);
    }
    atomicAdd(dst0 + c, a0);
    if (a1) atomicAdd(dst1 + c, a1);
}

// one element per lane: component c (counted if `active`), and whether it also counts for dst1
__device__ __forceinline__ void census_add(CensusTable& t, int* dst0, int* dst1, bool active, int c, bool second) {
    const unsigned long long todo = __ballot(active);
    if (!todo) return;
    const int leader = __builtin_ctzll(todo);
    const int k0 = __shfl(c, leader);
    const bool mine = active && c == k0;
    const int s0 = __popcll(__ballot(mine)), s1 = __popcll(__ballot(mine && second));
    if (lane_id() == leader) census_put(t, dst0, dst1, k0, s0, s1);
    else if (active && !mine) census_put(t, dst0, dst1, c, 1, second ? 1 : 0);
}

__device__ __forceinline__ void census_flush(CensusTable& t, int* dst0, int* dst1) {
    __syncthreads();
    for (int h = (int)threadIdx.x; h < CENSUS_TABLE; h += DIF_BLOCK) {
        const int k = t.key[h];
        if (k < 0) continue;
        if (t.n0[h]) atomicAdd(dst0 + k, t.n0[h]);
        if (t.n1[h]) atomicAdd(dst1 + k, t.n1[h]);
    }
}

// ---- components ------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(DIF_BLOCK) k_comp_init(int* __restrict__ parent, int V) {
    const int v = (int)(blockIdx.x * DIF_BLOCK + threadIdx.x);
    if (v < V) parent[v] = v;
}

#define COMP_LOAD(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)

// Root of v as far as this thread can see it.  parent[x] <= x always, so a chain is strictly descending and at most V long.
__device__ __forceinline__ int comp_find(const int* parent, int v, int V, bool& runaway) {
    for (int it = 0; it <= V; ++it) {
        const int p = COMP_LOAD(parent + v);
        if (p == v) return v;
        v = p;
    }
    runaway = true;
    return v;
}

// Lock-free union.  The higher root is hooked under the lower by atomicCAS(parent + hi, hi, lo): only a ROOT is ever written, only once, and
// only to a lower id, so parent[v] <= v holds throughout and no cycle can form.  A failed CAS means another thread hooked `hi` first (so another
// CAS succeeded: at most V - 1 do, which bounds the retries); the value it returned is where `hi` hangs now, and the search goes on from there.
// Memory model: eight L2s that are not coherent with each other — a plain load could be served from a stale line for ever, and a plain store
// (path compression) could sit in one.  Hence no plain access and no compression write in this launch: relaxed agent-scope loads (served past
// the stale copies) and the CAS (executed at the memory side) only.  No fence: a stale read costs one more retry, the CAS is the arbiter.
// Returns the root both hang under now (as far as this thread has seen): the next union of the same triangle starts there, not at the leaf.
__device__ __forceinline__ int comp_union(int* parent, int a, int b, int V, bool& runaway) {
    for (int it = 0; it <= V; ++it) {
        a = comp_find(parent, a, V, runaway);
        b = comp_find(parent, b, V, runaway);
        if (a == b || runaway) return a;
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        const int prev = atomicCAS(parent + hi, hi, lo);
        if (prev == hi) return lo;
        a = prev; b = lo;
    }
    runaway = true;
    return a;
}

// A thread unions HOOK_ITEMS CONSECUTIVE triangles, one after the other.  Without compression the depth of the forest is set by how many hooks
// happen at the same time along one path: a mesh's triangles come in spatial order, every vertex hooks under its lower neighbour at once, and the
// chains get as long as a row of the mesh.  Unions made one after the other hook under the ROOT found so far (depth one), so the chains shrink by
// about the number of triangles a thread takes.
#ifndef HOOK_ITEMS
#define HOOK_ITEMS 4
#endif
__global__ void __launch_bounds__(DIF_BLOCK) k_comp_hook(const int* __restrict__ tri, int K, int V, int* parent, int* __restrict__ counts) {
    const long long first = ((long long)blockIdx.x * DIF_BLOCK + threadIdx.x) * HOOK_ITEMS;
    bool runaway = false, bad = false;
    for (int i = 0; i < HOOK_ITEMS; ++i) {
        const long long t = first + i;
        if (t >= K) break;
        const int a = tri[3 * (size_t)t], b = tri[3 * (size_t)t + 1], c = tri[3 * (size_t)t + 2];
        if (!comp_in_range(a, b, c, V)) { bad = true; continue; }      // never dereferenced
        const int r = a != b ? comp_union(parent, a, b, V, runaway) : a;
        if (a != c) comp_union(parent, r, c, V, runaway);
    }
    if (bad) atomicOr(counts + COMP_STATUS, MESH_STATUS_BAD_INDEX);
    if (runaway) atomicOr(counts + COMP_STATUS, MESH_STATUS_RUNAWAY);
}

// Behind the kernel boundary nobody writes `parent`: plain loads.
__global__ void __launch_bounds__(DIF_BLOCK) k_comp_flatten(const int* __restrict__ parent, int V, int* __restrict__ label, int* __restrict__ counts) {
    int v = (int)(blockIdx.x * DIF_BLOCK + threadIdx.x);
    if (v >= V) return;
    const int self = v;
    bool found = false;
    for (int it = 0; it <= V; ++it) {
        const int p = parent[v];
        if (p == v) { found = true; break; }
        v = p;
    }
    if (!found) atomicOr(counts + COMP_STATUS, MESH_STATUS_RUNAWAY);
    label[self] = v;
}

// A root is its component's lowest vertex (parent[v] <= v), so roots in vertex order ARE the numbering rule.  vertex_component[root] = id.
struct CompNumberFunctor {
    const int* label;
    int* vertex_component; int* comp_vertices; int* comp_triangles;
    int* counts;
    __device__ int count(int v) const { return label[v] == v ? 1 : 0; }
    __device__ void emit(int v, int c) const { vertex_component[v] = c; comp_vertices[c] = 0; comp_triangles[c] = 0; }
    __device__ void finish(int total) const { counts[COMP_N] = total; }
};

// CENSUS_ITEMS vertices per thread, no early return (census_add needs every lane).  A root's entry is already written and is only read here.
__global__ void __launch_bounds__(DIF_BLOCK) k_comp_vertices(const int* __restrict__ label, int V, int* vertex_component, int* __restrict__ comp_vertices) {
    __shared__ CensusTable table;
    census_clear(table);
    for (int i = 0; i < CENSUS_ITEMS; ++i) {
        const long long v = ((long long)blockIdx.x * CENSUS_ITEMS + i) * DIF_BLOCK + threadIdx.x;
        int c = -1;
        if (v < V) {
            const int r = label[v];
            c = vertex_component[r];
            if (r != (int)v) vertex_component[v] = c;
        }
        census_add(table, comp_vertices, comp_vertices, c >= 0, c, false);
    }
    census_flush(table, comp_vertices, comp_vertices);
}

__global__ void __launch_bounds__(DIF_BLOCK) k_comp_triangles(const int* __restrict__ tri, int K, int V, const int* __restrict__ vertex_component,
                                                            int* __restrict__ triangle_component, int* __restrict__ comp_triangles) {
    __shared__ CensusTable table;
    census_clear(table);
    for (int i = 0; i < CENSUS_ITEMS; ++i) {
        const long long t = ((long long)blockIdx.x * CENSUS_ITEMS + i) * DIF_BLOCK + threadIdx.x;
        int c = -1;
        if (t < K) {
            const int a = tri[3 * (size_t)t], b = tri[3 * (size_t)t + 1], d = tri[3 * (size_t)t + 2];
            if (comp_in_range(a, b, d, V)) c = vertex_component[a];
            triangle_component[t] = c;
        }
        census_add(table, comp_triangles, comp_triangles, c >= 0, c, false);
    }
    census_flush(table, comp_triangles, comp_triangles);
}

// ---- select ----------------------------------------------------------------------------------------------------------------------------
// (every writer stores the same 1: plain stores)
__global__ void __launch_bounds__(DIF_BLOCK) k_select_mark(const int* __restrict__ tri, const uint8_t* __restrict__ keep, int K, int V, int* __restrict__ mark,
                                                         int* __restrict__ counts) {
    const int t = (int)(blockIdx.x * DIF_BLOCK + threadIdx.x);
    if (t >= K || !keep[t]) return;
    const int a = tri[3 * (size_t)t], b = tri[3 * (size_t)t + 1], c = tri[3 * (size_t)t + 2];
    if (!comp_in_range(a, b, c, V)) { atomicOr(counts + SELECT_STATUS, MESH_STATUS_BAD_INDEX); return; }    // such a triangle is not kept
    mark[a] = 1; mark[b] = 1; mark[c] = 1;
}

// Attributes move as 32-bit words: bit for bit, NaN payloads included.
struct SelectVertexFunctor {
    const int* mark;
    const unsigned* vertices; const unsigned* normals; const unsigned* vertex_std;
    unsigned* out_vertices; unsigned* out_normals; unsigned* out_vertex_std;
    int* remap;
    int* counts;
    __device__ int count(int v) const { return mark[v]; }
    __device__ void emit(int v, int n) const {
        remap[v] = n;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            out_vertices[(size_t)n * 3 + k] = vertices[(size_t)v * 3 + k];
            out_normals[(size_t)n * 3 + k] = normals[(size_t)v * 3 + k];
        }
        out_vertex_std[n] = vertex_std[v];
    }
    __device__ void finish(int total) const { counts[SELECT_N_VERTICES] = total; }
};

struct SelectTriangleFunctor {
    const int* tri; const int64_t* tri_id; const uint8_t* keep;
    const int* remap;
    int32_t* out_tri; int64_t* out_tri_id;
    int V;
    int* counts;
    __device__ int count(int t) const {
        return (keep[t] && comp_in_range(tri[3 * (size_t)t], tri[3 * (size_t)t + 1], tri[3 * (size_t)t + 2], V)) ? 1 : 0;
    }
    __device__ void emit(int t, int k) const {
#pragma unroll
        for (int j = 0; j < 3; ++j) out_tri[(size_t)k * 3 + j] = remap[tri[3 * (size_t)t + j]];
        out_tri_id[k] = tri_id[t];
    }
    __device__ void finish(int total) const { counts[SELECT_N_TRIANGLES] = total; }
};

// ---- edge census -----------------------------------------------------------------------------------------------------------------------
struct EdgeTable {
    unsigned long long* key;    // [cap]  EDGE_EMPTY = free, else (low end << 31) | high end
    unsigned* uses;             // [cap]  triangles that name the edge (cleared to 0)
    unsigned mask;              // cap - 1
    int shift;                  // 64 - log2(cap)
};

// One thread per triangle side.  The weld's insert: CAS on the 64-bit key, probe loop bounded by the capacity (>= 2 x 3 K: at most half full).
__global__ void __launch_bounds__(DIF_BLOCK) k_edge_insert(EdgeTable t, const int* __restrict__ tri, int n, int V, int* __restrict__ counts) {
    const int i = (int)(blockIdx.x * DIF_BLOCK + threadIdx.x);
    if (i >= n) return;
    const int j = i % 3;
    const int* p = tri + (i - j);
    if (!comp_in_range(p[0], p[1], p[2], V)) {                                      // as in the components: such a triangle is part of nothing
        if (j == 0) atomicOr(counts + EDGE_STATUS, MESH_STATUS_BAD_INDEX);
        return;
    }
    const int a = p[j], b = p[j == 2 ? 0 : j + 1];
    if (a == b) return;                                                             // not an edge
    const unsigned long long key = ((unsigned long long)(unsigned)(a < b ? a : b) << 31) | (unsigned long long)(unsigned)(a < b ? b : a);
    unsigned h = (unsigned)((key * 0x9E3779B97F4A7C15ull) >> t.shift);
    bool found = false;
    for (unsigned probe = 0; probe <= t.mask; ++probe) {
        unsigned long long prev = __hip_atomic_load(t.key + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (prev == EDGE_EMPTY) prev = atomicCAS(t.key + h, EDGE_EMPTY, key);
        if (prev == EDGE_EMPTY || prev == key) { found = true; break; }
        h = (h + 1) & t.mask;
    }
    if (!found) { atomicOr(counts + EDGE_STATUS, MESH_STATUS_TABLE_FULL); return; }
    atomicAdd(t.uses + h, 1u);
}

// CENSUS_SLOT_ITEMS slots per thread, no early return (the wave votes need every lane).  An edge belongs to the component of its low end.
__global__ void __launch_bounds__(DIF_BLOCK) k_edge_slots(EdgeTable t, const int* __restrict__ vertex_component, int C, int* __restrict__ comp_edges,
                                                        int* __restrict__ comp_boundary, int* __restrict__ counts) {
    __shared__ CensusTable table;
    census_clear(table);
    unsigned most = 0;
    bool bad = false;
    for (int i = 0; i < CENSUS_SLOT_ITEMS; ++i) {
        const unsigned long long s = ((unsigned long long)blockIdx.x * CENSUS_SLOT_ITEMS + i) * DIF_BLOCK + threadIdx.x;
        int c = -1;
        unsigned u = 0;
        if (s <= t.mask) {
            const unsigned long long key = t.key[s];
            if (key != EDGE_EMPTY) {
                c = vertex_component[(int)(key >> 31)];
                if ((unsigned)c >= (unsigned)C) { bad = true; c = -1; }
                else u = t.uses[s];
            }
        }
        most = max(most, u);
        census_add(table, comp_edges, comp_boundary, c >= 0, c, u == 1);
    }
    census_flush(table, comp_edges, comp_boundary);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) most = max(most, (unsigned)__shfl_xor((int)most, d));
    if (lane_id() == 0 && most > 0 && (unsigned)__hip_atomic_load(counts + EDGE_MAX_USE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < most)
        atomicMax(counts + EDGE_MAX_USE, (int)most);
    if (bad) atomicOr(counts + EDGE_STATUS, MESH_STATUS_BAD_INDEX);
}
