// Closest point on an indexed mesh for a cloud of query points (dif_mesh_locator_build, dif_mesh_closest).
// No reference counterpart: the reference leaves this to Open3D on the CPU (compute_point_cloud_distance, raycasting scenes).  DESIGN.md
// "Closest point on an indexed mesh"; the contract is in include/difusion.h.
//
// The grid is the cloud ops' (kernels_cloud.hip.h): cubic cells of edge c, keyed by floor(fl(x * fl(1 / c))) per axis, hashed into an open-addressing
// table of 16-byte entries (key, count - 1, one past the last row) — no bounding box.  A triangle is an extended primitive: it is REGISTERED in every
// cell that its vertex box, widened (below), overlaps; the cells' rows are triangle INDICES (a CSR of references), and the nine floats of every usable
// triangle sit once in a table of three float4 per triangle (DESIGN.md says why).  A triangle whose box covers more than `max_cells` cells goes to
// the LARGE list, which every query walks directly (the rasteriser's split, kernels_raster.hip.h).
//
// The answer of a query is the minimum of the packed key (float bits of d2, triangle index) over all usable triangles with d2 <= max_distance^2;
// d2 of a pair is ONE fixed float32 sequence (loc_eval), so the answer is the all-pairs minimum whatever the cell size — IF no cell or ring that the
// search skips holds a triangle whose COMPUTED d2 beats the bound.  Why it does not:
//
//   (1) loc_eval returns a vertex, bit for bit, or a + t ab, b + t bc, a + (v ab + w ac) with t, v, w, v + w in [0, 1] up to one rounding (w <=
//       fl(1 - v)).  With m = the largest |coordinate| of the triangle and u = 2^-24: an edge vector is off by u 2m, its product with the weight by
//       another u 2m, the sum of the two products by u 2m, the final sum by u m (1 + ...), and v + w may pass 1 by u / 2 (an excursion of u m): the
//       computed point leaves the box of the three vertices by less than 9 u m per axis.
//   (2) Registration widens the box by wr = fl(2^-20 m) = 16 u m per side; the subtraction lo - wr rounds by at most u m, so the computed point
//       x satisfies fl(lo - wr) <= x <= fl(hi + wr).  The cell coordinate floor(fl(x * inv_c)) is a MONOTONIC function of the float x, and the
//       registered range is that function of fl(lo - wr) and fl(hi + wr): the cell of the computed closest point — under the very membership function
//       the query uses — is one the triangle is registered in.  No rounding of the membership enters here.
//   (3) So for a triangle T whose computed d2 would beat the bound, the cell Y of its computed closest point x holds T, and the question is the
//       cloud query's: can the cell box test or the ring bound skip a cell that holds a POINT x with |x - q|^2 (taken in the order (ex ex + ey ey) +
//       ez ez, as the bound is) below the bound?  kernels_cloud.hip.h:228-237 derives the slack for exactly that: cell membership rounding of both
//       cells (2.01 u |j| c each), the edge product (u |j| c), the subtraction (u of itself): `slack` = 2^-21 (max |q| + (max_ring + 2) c) = 8 u m'
//       covers the box test (4.02 u m') and the ring bound (6.03 u m') and its own three roundings.  Float32 rounding is monotonic, so the
//       inequality between the true gaps carries over to the computed squares and sums.
//   (4) Ties: a skipped cell or ring only holds points with d2 STRICTLY above the bound used (the best d2 so far, or max_distance^2), so an
//       equal d2 with a lower triangle index is never skipped.
//
// House rules as in kernels_weld.hip.h: every launch is bounded, nothing spins on or waits for another workgroup, probe loops are bounded by the
// table's capacity and report instead of looping.  Plain vector stores, atomicCAS / atomicAdd / atomicOr only.
#pragma once

#define LOC_ABS_LIMIT 0x1p60f                   // |coordinate| below this: no square of a difference leaves float32
#define LOC_WIDEN 0x1p-20f                      // (2) above
#define LOC_NB 16                               // cells looked up together
#define LOC_U 4                                 // triangles fetched together
#define LOC_NONE 0x7FFFFFFF
// the header of the workspace: the build's counts in the order of DIF_LOCATOR_*, and the pairs in 64 bits
enum { LOC_H_PAIRS64 = 14, LOC_H_WORDS = 16 };

struct Locator {
    CloudGrid g;                // tab, mask, shift, c, inv_c (sorted and slot are not used)
    int* refs;                  // [pair_capacity] triangle indices, grouped by cell
    float4* rec;                // [K][3] the vertices of a usable triangle
    int* ncell;                 // [K] cells an indexed triangle is registered in, 0 for every other triangle
    int* large;                 // [K] the large list (its length: head[DIF_LOCATOR_LARGE])
    int* head;                  // [LOC_H_WORDS]
    int capacity;               // pair_capacity
};

__device__ __forceinline__ float loc_dot(float ux, float uy, float uz, float vx, float vy, float vz) { return (ux * vx + uy * vy) + uz * vz; }

// num / den where den > 0, else 0; clamped to [0, 1] (fmaxf / fminf drop a NaN)
__device__ __forceinline__ float loc_ratio(float num, float den) {
    const float t = den > 0.0f ? __fdiv_rn(num, den) : 0.0f;
    return fminf(fmaxf(t, 0.0f), 1.0f);
}

// THE float32 sequence (tests/closest_ref.py:evaluate restates it).  FULL: closest point and barycentrics as well.
template <bool FULL>
__device__ __forceinline__ float loc_eval(float px, float py, float pz, const float4& A, const float4& B, const float4& C, float* point, float* bary) {
    const float abx = B.x - A.x, aby = B.y - A.y, abz = B.z - A.z;
    const float acx = C.x - A.x, acy = C.y - A.y, acz = C.z - A.z;
    const float bcx = C.x - B.x, bcy = C.y - B.y, bcz = C.z - B.z;
    const float apx = px - A.x, apy = py - A.y, apz = pz - A.z;
    const float bpx = px - B.x, bpy = py - B.y, bpz = pz - B.z;
    const float cpx = px - C.x, cpy = py - C.y, cpz = pz - C.z;
    const float d1 = loc_dot(abx, aby, abz, apx, apy, apz), d2 = loc_dot(acx, acy, acz, apx, apy, apz);
    const float d3 = loc_dot(abx, aby, abz, bpx, bpy, bpz), d4 = loc_dot(acx, acy, acz, bpx, bpy, bpz);
    const float d5 = loc_dot(abx, aby, abz, cpx, cpy, cpz), d6 = loc_dot(acx, acy, acz, cpx, cpy, cpz);
    const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    const float e43 = d4 - d3, e56 = d5 - d6;
    const bool eq_a = px == A.x && py == A.y && pz == A.z, eq_b = px == B.x && py == B.y && pz == B.z, eq_c = px == C.x && py == C.y && pz == C.z;
    int region;
    if (eq_a) region = 0;
    else if (eq_b) region = 1;
    else if (eq_c) region = 2;
    else if (d1 <= 0.0f && d2 <= 0.0f) region = 0;
    else if (d3 >= 0.0f && d4 <= d3) region = 1;
    else if (d6 >= 0.0f && d5 <= d6) region = 2;
    else if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) region = 3;
    else if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) region = 4;
    else if (va <= 0.0f && e43 >= 0.0f && e56 >= 0.0f) region = 5;
    else region = 6;
    float cx, cy, cz, b0, b1, b2;
    if (region == 0) { cx = A.x; cy = A.y; cz = A.z; b0 = 1.0f; b1 = 0.0f; b2 = 0.0f; }
    else if (region == 1) { cx = B.x; cy = B.y; cz = B.z; b0 = 0.0f; b1 = 1.0f; b2 = 0.0f; }
    else if (region == 2) { cx = C.x; cy = C.y; cz = C.z; b0 = 0.0f; b1 = 0.0f; b2 = 1.0f; }
    else if (region == 3) {
        const float t = loc_ratio(d1, d1 - d3);
        cx = A.x + t * abx; cy = A.y + t * aby; cz = A.z + t * abz; b0 = 1.0f - t; b1 = t; b2 = 0.0f;
    } else if (region == 4) {
        const float t = loc_ratio(d2, d2 - d6);
        cx = A.x + t * acx; cy = A.y + t * acy; cz = A.z + t * acz; b0 = 1.0f - t; b1 = 0.0f; b2 = t;
    } else if (region == 5) {
        const float t = loc_ratio(e43, e43 + e56);
        cx = B.x + t * bcx; cy = B.y + t * bcy; cz = B.z + t * bcz; b0 = 0.0f; b1 = 1.0f - t; b2 = t;
    } else {
        const float den = (va + vb) + vc;
        const float v = loc_ratio(vb, den);
        const float w = fminf(loc_ratio(vc, den), 1.0f - v);
        cx = A.x + (v * abx + w * acx); cy = A.y + (v * aby + w * acy); cz = A.z + (v * abz + w * acz); b0 = (1.0f - v) - w; b1 = v; b2 = w;
    }
    if (FULL) { point[0] = cx; point[1] = cy; point[2] = cz; bary[0] = b0; bary[1] = b1; bary[2] = b2; }
    const float ex = cx - px, ey = cy - py, ez = cz - pz;
    return (ex * ex + ey * ey) + ez * ez;
}

// The cells [lo, hi] per axis that the widened vertex box overlaps; false: a coordinate is not finite, reaches LOC_ABS_LIMIT, or a cell coordinate
// leaves the key range.
__device__ __forceinline__ bool loc_box(const CloudGrid& g, const float4& A, const float4& B, const float4& C, int lo[3], int hi[3]) {
    const float a[3] = {A.x, A.y, A.z}, b[3] = {B.x, B.y, B.z}, c[3] = {C.x, C.y, C.z};
    float m = 0.0f;
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        ok = ok && fabsf(a[k]) < LOC_ABS_LIMIT && fabsf(b[k]) < LOC_ABS_LIMIT && fabsf(c[k]) < LOC_ABS_LIMIT;      // (NaN fails)
        m = fmaxf(m, fmaxf(fabsf(a[k]), fmaxf(fabsf(b[k]), fabsf(c[k]))));
    }
    const float wr = LOC_WIDEN * m, lim = (float)(CLOUD_OFF - 64);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float fl = floorf((fminf(fminf(a[k], b[k]), c[k]) - wr) * g.inv_c), fh = floorf((fmaxf(fmaxf(a[k], b[k]), c[k]) + wr) * g.inv_c);
        ok = ok && fabsf(fl) < lim && fabsf(fh) < lim;
        lo[k] = ok ? (int)fl : 0;
        hi[k] = ok ? (int)fh : 0;
    }
    return ok;
}

// One thread per triangle, no early return (votes and block sums).  Classes, tested in this order: an index outside [0, V) (never dereferenced);
// SKIPPED (loc_box fails); DEGENERATE (the float32 cross product of the two edge vectors is exactly zero); LARGE; else indexed, with its cell count.
__global__ void __launch_bounds__(DIF_BLOCK) k_loc_classify(Locator L, const float* __restrict__ vertices, const int* __restrict__ tri, int K, int V, int max_cells) {
    __shared__ int smem[8];
    const long long t = (long long)blockIdx.x * DIF_BLOCK + threadIdx.x;
    bool bad = false, large = false;
    int skipped = 0, degenerate = 0, indexed = 0, cells = 0;
    if (t < K) {
        const int a = tri[3 * (size_t)t], b = tri[3 * (size_t)t + 1], c = tri[3 * (size_t)t + 2];
        if (!comp_in_range(a, b, c, V)) {
            bad = true;
        } else {
            const float* pa = vertices + (size_t)a * 3; const float* pb = vertices + (size_t)b * 3; const float* pc = vertices + (size_t)c * 3;
            const float4 A = make_float4(pa[0], pa[1], pa[2], 0.0f), B = make_float4(pb[0], pb[1], pb[2], 0.0f), C = make_float4(pc[0], pc[1], pc[2], 0.0f);
            int lo[3], hi[3];
            if (!loc_box(L.g, A, B, C, lo, hi)) {
                skipped = 1;
            } else {
                const float abx = B.x - A.x, aby = B.y - A.y, abz = B.z - A.z, acx = C.x - A.x, acy = C.y - A.y, acz = C.z - A.z;
                const float nx = aby * acz - abz * acy, ny = abz * acx - abx * acz, nz = abx * acy - aby * acx;
                if (nx == 0.0f && ny == 0.0f && nz == 0.0f) {
                    degenerate = 1;
                } else {
                    L.rec[3 * (size_t)t] = A; L.rec[3 * (size_t)t + 1] = B; L.rec[3 * (size_t)t + 2] = C;
                    const long long ex = (long long)hi[0] - lo[0] + 1, ey = (long long)hi[1] - lo[1] + 1, ez = (long long)hi[2] - lo[2] + 1;      // each <= 2^21
                    large = max_cells < 0 || ex > max_cells || ey > max_cells || ez > max_cells || ex * ey * ez > max_cells;
                    if (!large) { indexed = 1; cells = (int)(ex * ey * ez); }
                }
            }
        }
        L.ncell[t] = cells;
    }
    // one reservation per wave; the list's order does not matter (the answer is a minimum); at most K entries: each triangle appends once
    const int lane = lane_id();
    const unsigned long long vl = __ballot(large);
    if (vl) {
        const int leader = __builtin_ctzll(vl);
        int base = 0;
        if (lane == leader) base = atomicAdd(L.head + DIF_LOCATOR_LARGE, __popcll(vl));
        base = __shfl(base, leader);
        if (large) L.large[base + __popcll(vl & ((1ull << lane) - 1ull))] = (int)t;
    }
    const int ns = block_sum(skipped, smem), nd = block_sum(degenerate, smem), ni = block_sum(indexed, smem), nb = block_sum(bad ? 1 : 0, smem);
    const int np = block_sum(cells, smem);              // <= 256 max_cells: the cap is refused above 2^20
    if (threadIdx.x == 0) {
        if (ns) atomicAdd(L.head + DIF_LOCATOR_SKIPPED, ns);
        if (nd) atomicAdd(L.head + DIF_LOCATOR_DEGENERATE, nd);
        if (ni) atomicAdd(L.head + DIF_LOCATOR_INDEXED, ni);
        if (nb) { atomicAdd(L.head + DIF_LOCATOR_BAD_INDEX, nb); atomicOr(L.head + DIF_LOCATOR_STATUS, MESH_STATUS_BAD_INDEX); }
        if (np) atomicAdd((unsigned long long*)(L.head + LOC_H_PAIRS64), (unsigned long long)np);
    }
}

__device__ __forceinline__ bool loc_fits(const Locator& L) { return *(const unsigned long long*)(L.head + LOC_H_PAIRS64) <= (unsigned long long)L.capacity; }

// One thread per triangle, no early return past the first line (block sums).  Nothing is inserted when the pairs do not fit: the table holds twice
// the capacity, so with pairs <= capacity it is never more than half full and every probe ends.
__global__ void __launch_bounds__(DIF_BLOCK) k_loc_insert(Locator L, int K) {
    __shared__ int smem[8];
    if (!loc_fits(L)) {                                                     // (uniform over the launch)
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(L.head + DIF_LOCATOR_STATUS, DIF_MESH_STATUS_PAIR_OVERFLOW);
        return;
    }
    const long long t = (long long)blockIdx.x * DIF_BLOCK + threadIdx.x;
    int fresh = 0;
    bool full = false;
    if (t < K && L.ncell[t] > 0) {
        int lo[3], hi[3];
        loc_box(L.g, L.rec[3 * (size_t)t], L.rec[3 * (size_t)t + 1], L.rec[3 * (size_t)t + 2], lo, hi);
        for (int x = lo[0]; x <= hi[0]; ++x)
            for (int y = lo[1]; y <= hi[1]; ++y)
                for (int z = lo[2]; z <= hi[2]; ++z) {
                    const unsigned long long key = cloud_key(x, y, z);
                    unsigned h = cloud_hash(L.g, key);
                    bool home = true, placed = false;
                    for (unsigned probe = 0; probe <= L.g.mask; ++probe) {
                        const unsigned long long prev = atomicCAS(&L.g.tab[h].key, CLOUD_EMPTY, key);
                        if (prev == CLOUD_EMPTY) ++fresh;
                        if (prev == CLOUD_EMPTY || prev == key) { placed = true; break; }
                        h = home ? cloud_hash2(L.g, key) : ((h + 1) & L.g.mask);
                        home = false;
                    }
                    if (placed) atomicAdd(&L.g.tab[h].cnt_m1, 1);
                    else full = true;
                }
    }
    const int nf = block_sum(fresh, smem);
    if (threadIdx.x == 0 && nf) atomicAdd(L.head + DIF_LOCATOR_CELLS, nf);
    if (full) atomicOr(L.head + DIF_LOCATOR_STATUS, MESH_STATUS_TABLE_FULL);
}

// The slot of a cell that k_loc_insert placed (the table is final here: plain loads), or -1.
__device__ __forceinline__ int loc_find(const CloudGrid& g, unsigned long long key) {
    unsigned h = cloud_hash(g, key);
    bool home = true;
    for (unsigned probe = 0; probe <= g.mask; ++probe) {
        const unsigned long long got = g.tab[h].key;
        if (got == key) return (int)h;
        if (got == CLOUD_EMPTY) return -1;
        h = home ? cloud_hash2(g, key) : ((h + 1) & g.mask);
        home = false;
    }
    return -1;
}

// One thread per triangle.  The scan (CloudStartFunctor) left every cell's first row in `end`: it is the placement cursor, and one past the cell's
// last row afterwards.  The order of the rows inside a cell depends on the schedule; no answer does.
__global__ void __launch_bounds__(DIF_BLOCK) k_loc_fill(Locator L, int K) {
    if (!loc_fits(L)) return;
    const long long t = (long long)blockIdx.x * DIF_BLOCK + threadIdx.x;
    if (t >= K || L.ncell[t] <= 0) return;
    int lo[3], hi[3];
    loc_box(L.g, L.rec[3 * (size_t)t], L.rec[3 * (size_t)t + 1], L.rec[3 * (size_t)t + 2], lo, hi);
    for (int x = lo[0]; x <= hi[0]; ++x)
        for (int y = lo[1]; y <= hi[1]; ++y)
            for (int z = lo[2]; z <= hi[2]; ++z) {
                const int s = loc_find(L.g, cloud_key(x, y, z));
                if (s < 0) continue;                                        // (cannot be: k_loc_insert placed it, or reported)
                const int pos = atomicAdd(&L.g.tab[s].end, 1);
                if ((unsigned)pos < (unsigned)L.capacity) L.refs[pos] = (int)t;
            }
}

// head -> the caller's counts (the pairs saturate at INT32_MAX)
__global__ void k_loc_finish(Locator L, int* __restrict__ counts) {
    const int k = (int)threadIdx.x;
    if (k >= DIF_LOCATOR_COUNT) return;
    const unsigned long long pairs = *(const unsigned long long*)(L.head + LOC_H_PAIRS64);
    counts[k] = k == DIF_LOCATOR_PAIRS ? (pairs > 0x7FFFFFFFull ? 0x7FFFFFFF : (int)pairs) : L.head[k];
}

struct LocQueryOut { float* d2; int* triangle; float* point; float* bary; };

// One thread per query point, in the caller's order (consecutive points that lie close to each other walk the same cells: the time depends on
// that coherence).  The large list first, then ring by ring as k_cloud_query does: LOC_NB first-probe table entries requested together, the rows
// of the batch's cells walked as one flat sequence, LOC_U references and then their 3 LOC_U float4 at a time — a chain of dependent loads (entry ->
// reference -> record), so what a thread keeps in flight decides the time.  Only the packed key of the best pair is kept; the winner is evaluated
// once more for its point and barycentrics.  No early return (block sums at the end).
__global__ void __launch_bounds__(DIF_BLOCK) k_loc_query(Locator L, int K, const float* __restrict__ pts, int n, int stride, float r2, int max_ring, LocQueryOut out,
                                                        int* __restrict__ counts) {
    __shared__ int2 s_run[LOC_NB * DIF_BLOCK];             // [cell of the batch][thread]: (first row - rows before it in the batch, rows before it)
    __shared__ int smem[8];
    const long long i = (long long)blockIdx.x * DIF_BLOCK + threadIdx.x;
    const CloudGrid& g = L.g;
    const bool built = (L.head[DIF_LOCATOR_STATUS] & (DIF_MESH_STATUS_PAIR_OVERFLOW | MESH_STATUS_TABLE_FULL)) == 0;
    float qx = 0.0f, qy = 0.0f, qz = 0.0f;
    int cx = 0, cy = 0, cz = 0;
    bool ok = false;
    if (i < n) {
        const float* p = pts + (size_t)i * stride;
        qx = p[0]; qy = p[1]; qz = p[2];
        ok = cloud_cell(g, qx, qy, qz, cx, cy, cz) && fabsf(qx) < LOC_ABS_LIMIT && fabsf(qy) < LOC_ABS_LIMIT && fabsf(qz) < LOC_ABS_LIMIT;
    }
    unsigned long long best = cloud_pack(__builtin_inff(), LOC_NONE);
    if (ok && built) {
        const int nl = min(L.head[DIF_LOCATOR_LARGE], K);
        for (int e = 0; e < nl; ++e) {
            const int t = L.large[e];
            if ((unsigned)t >= (unsigned)K) continue;                       // (cannot be for a workspace built with this K: never read out of bounds)
            const float d2 = loc_eval<false>(qx, qy, qz, L.rec[3 * (size_t)t], L.rec[3 * (size_t)t + 1], L.rec[3 * (size_t)t + 2], nullptr, nullptr);
            const unsigned long long ck = cloud_pack(d2, t);
            best = ck < best ? ck : best;
        }
        // `slack`: (3) of the file comment
        const float slack = 0x1p-21f * (fmaxf(fmaxf(fabsf(qx), fabsf(qy)), fabsf(qz)) + (float)(max_ring + 2) * g.c);
        const uint4* __restrict__ tab4 = reinterpret_cast<const uint4*>(g.tab);
        int2* const run = s_run + threadIdx.x;
        // Ring max_ring (the host: floor(max_distance / c) + 1) bounds every unvisited point beyond max_distance while slack stays small; far from the
        // origin ring max_ring + 1 does (slack <= c / 2 at the key range's end).  The loop ends through the tests below, never through its own limit.
        for (int rho = 0; rho <= max_ring + 1; ++rho) {
            int dx = -rho, dy = -rho, dz = -rho;           // the shell in the order of three nested loops, interior columns reduced to their end caps
            bool more = true;
            while (more) {
                uint4 ent[LOC_NB];
                int off[LOC_NB];
                // a cell whose nearest corner is strictly farther than the best so far, or than max_distance, is not looked up at all
                const float far2 = fminf(__uint_as_float((unsigned)(best >> 32)), r2);
#pragma unroll
                for (int b = 0; b < LOC_NB; ++b) {
                    off[b] = -1;
                    ent[b] = uint4{0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u};
                    if (more) {
                        const float gx = dx < 0 ? qx - (float)(cx + dx + 1) * g.c : dx > 0 ? (float)(cx + dx) * g.c - qx : 0.0f;
                        const float gy = dy < 0 ? qy - (float)(cy + dy + 1) * g.c : dy > 0 ? (float)(cy + dy) * g.c - qy : 0.0f;
                        const float gz = dz < 0 ? qz - (float)(cz + dz + 1) * g.c : dz > 0 ? (float)(cz + dz) * g.c - qz : 0.0f;
                        const float hx = fmaxf(gx - slack, 0.0f), hy = fmaxf(gy - slack, 0.0f), hz = fmaxf(gz - slack, 0.0f);
                        if ((hx * hx + hy * hy) + hz * hz <= far2) {
                            off[b] = ((dx + 64) << 16) | ((dy + 64) << 8) | (dz + 64);
                            ent[b] = tab4[cloud_hash(g, cloud_key(cx + dx, cy + dy, cz + dz))];
                        }
                        const bool face = (dx == -rho) || (dx == rho) || (dy == -rho) || (dy == rho);
                        dz += (face || rho == 0) ? 1 : 2 * rho;
                        if (dz > rho) { dz = -rho; if (++dy > rho) { dy = -rho; if (++dx > rho) more = false; } }
                    }
                }
                // ---- which of them exist, and where their rows are ----
                int m = 0, tot = 0;
#pragma unroll
                for (int b = 0; b < LOC_NB; ++b) {
                    if (off[b] < 0) continue;
                    const unsigned long long key = cloud_key(cx + (off[b] >> 16) - 64, cy + ((off[b] >> 8) & 0xFF) - 64, cz + (off[b] & 0xFF) - 64);
                    unsigned long long got = ((unsigned long long)ent[b].y << 32) | ent[b].x;
                    int c = (int)ent[b].z + 1, e = (int)ent[b].w;
                    if (got != key && got != CLOUD_EMPTY) {                 // the first probe hit another cell's entry (rare): walk on, bounded
                        unsigned h = cloud_hash2(g, key);
                        for (unsigned probe = 0; probe <= g.mask; ++probe) {
                            const uint4 v = tab4[h];
                            got = ((unsigned long long)v.y << 32) | v.x;
                            c = (int)v.z + 1; e = (int)v.w;
                            if (got == key || got == CLOUD_EMPTY) break;
                            h = (h + 1) & g.mask;
                        }
                    }
                    if (got == key) {
                        run[m * DIF_BLOCK] = make_int2(e - c - tot, tot);
                        tot += c;
                        ++m;
                    }
                }
                // ---- the batch's rows as one sequence ----
                int cur = 0, base = 0, lim = 0;
                if (m > 0) { base = run[0].x; lim = m > 1 ? run[DIF_BLOCK].y : tot; }
                for (int t0 = 0; t0 < tot; t0 += LOC_U) {
                    int ref[LOC_U];
#pragma unroll
                    for (int u = 0; u < LOC_U; ++u) {
                        const int t = t0 + u;
                        ref[u] = -1;
                        if (t < tot) {
                            while (t >= lim) {
                                ++cur;
                                base = run[cur * DIF_BLOCK].x;
                                lim = cur + 1 < m ? run[(cur + 1) * DIF_BLOCK].y : tot;
                            }
                            const unsigned row = (unsigned)(base + t);
                            if (row < (unsigned)L.capacity) ref[u] = L.refs[row];
                        }
                    }
                    float4 A[LOC_U], B[LOC_U], C[LOC_U];
#pragma unroll
                    for (int u = 0; u < LOC_U; ++u) {
                        if ((unsigned)ref[u] < (unsigned)K) { A[u] = L.rec[3 * (size_t)ref[u]]; B[u] = L.rec[3 * (size_t)ref[u] + 1]; C[u] = L.rec[3 * (size_t)ref[u] + 2]; }
                    }
#pragma unroll
                    for (int u = 0; u < LOC_U; ++u) {
                        if ((unsigned)ref[u] < (unsigned)K) {
                            const float d2 = loc_eval<false>(qx, qy, qz, A[u], B[u], C[u], nullptr, nullptr);
                            const unsigned long long ck = cloud_pack(d2, ref[u]);
                            best = ck < best ? ck : best;
                        }
                    }
                }
            }
            const float lb = (float)rho * g.c - slack;     // every unvisited computed closest point is at least this far
            if (lb > 0.0f && (r2 < lb * lb || __uint_as_float((unsigned)(best >> 32)) < lb * lb)) break;
        }
    }
    const float bd2 = __uint_as_float((unsigned)(best >> 32));
    const int bt = (int)(unsigned)best;
    const bool found = ok && built && (unsigned)bt < (unsigned)K && bd2 <= r2;       // (LOC_NONE is not below K)
    if (i < n) {
        const float nan = __int_as_float(0x7FC00000);
        float point[3] = {nan, nan, nan}, bary[3] = {nan, nan, nan};
        if (found) loc_eval<true>(qx, qy, qz, L.rec[3 * (size_t)bt], L.rec[3 * (size_t)bt + 1], L.rec[3 * (size_t)bt + 2], point, bary);
        out.d2[i] = found ? bd2 : __builtin_inff();
        out.triangle[i] = found ? bt : -1;
#pragma unroll
        for (int k = 0; k < 3; ++k) { out.point[(size_t)i * 3 + k] = point[k]; out.bary[(size_t)i * 3 + k] = bary[k]; }
    }
    const int nf = block_sum(found ? 1 : 0, smem), nfar = block_sum((i < n && ok && !found) ? 1 : 0, smem), nbad = block_sum((i < n && !ok) ? 1 : 0, smem);
    if (threadIdx.x == 0) {
        if (nf) atomicAdd(counts + DIF_CLOSEST_FOUND, nf);
        if (nfar) atomicAdd(counts + DIF_CLOSEST_FAR, nfar);
        if (nbad) atomicAdd(counts + DIF_CLOSEST_BAD_POINT, nbad);
        if (!built && blockIdx.x == 0) atomicOr(counts + DIF_CLOSEST_STATUS, L.head[DIF_LOCATOR_STATUS] & (DIF_MESH_STATUS_PAIR_OVERFLOW | MESH_STATUS_TABLE_FULL));
    }
}
