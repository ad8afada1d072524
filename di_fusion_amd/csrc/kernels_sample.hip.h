// Points drawn uniformly by area from the surface of an indexed mesh (dif_mesh_sampler_build, dif_mesh_sample).
// No reference counterpart: the reference leaves this to Open3D on the CPU (sample_points_uniformly).  DESIGN.md "Sampling an indexed mesh"; the
// contract is in include/difusion.h and tests/sample_ref.py restates it in numpy.
//
// Everything that decides WHICH triangle a sample falls on is an integer: the weight of a triangle is its doubled area in double, scaled by a power
// of two so that the largest one lies in [2^31, 2^32), and floored.  Sums of such integers are exact in any order, so the inclusive prefix sums P
// (uint64) and their total T are the same whatever the scan layout, and sample j is a pure function of (mesh, N, seed): stratum j of N over [0, T),
// one splitmix64 draw inside it, the first triangle whose prefix passes the target, one more draw for the barycentrics (24-bit integers, exact in
// float32), and the point in the float32 sequence of `interpolate`.
//
// The build is three bounded launches (the nine floats per triangle and the largest doubled area; the block totals of the weights; the 64-bit scan:
// common.hip.h's scans are 32-bit, this one is new), the sampler one: a binary search over P per sample.  Nothing spins on or waits for another
// workgroup.  Plain vector stores, atomicAdd / atomicMax / atomicOr only.
#pragma once

#define SMP_ABS_LIMIT 0x1p60f                   // the closest operator's limit on |coordinate|

struct SamplerHead {
    unsigned long long max_bits;                // bits of the largest doubled area (a non-negative double: its bits order as it does)
    unsigned long long total;                   // T
    int counts[DIF_SAMPLER_COUNT];
};

struct Sampler {
    SamplerHead* head;
    double* norm;                               // [K] |e1 x e2| in double; 0 for a triangle that is skipped or holds a bad index
    unsigned long long* prefix;                 // [K] P
    unsigned long long* block_tot;              // [1024] the weights per block of the scan
};

__device__ __forceinline__ unsigned long long smp_mix(unsigned long long z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__device__ __forceinline__ unsigned long long smp_wave_sum(unsigned long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// sum over the block, in every thread; smem: blockDim.x / 64 words
__device__ __forceinline__ unsigned long long smp_block_sum(unsigned long long v, unsigned long long* smem) {
    const int lane = lane_id(), wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
    v = smp_wave_sum(v);
    __syncthreads();                            // protect smem from the previous use
    if (lane == 0) smem[wid] = v;
    __syncthreads();
    unsigned long long tot = 0;
    for (int w = 0; w < nw; ++w) tot += smem[w];
    return tot;
}

// exclusive prefix of v across the block; the block's sum in `total`
__device__ __forceinline__ unsigned long long smp_block_excl_scan(unsigned long long v, unsigned long long* smem, unsigned long long& total) {
    const int lane = lane_id(), wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
    unsigned long long inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long o = __shfl_up(inc, d);
        if (lane >= d) inc += o;
    }
    __syncthreads();
    if (lane == 63) smem[wid] = inc;
    __syncthreads();
    unsigned long long base = 0, tot = 0;
    for (int w = 0; w < nw; ++w) {
        const unsigned long long s = smem[w];
        if (w < wid) base += s;
        tot += s;
    }
    total = tot;
    return base + inc - v;
}

// the weight of a doubled area n under the mesh's exponent e: floor(n 2^(32 - e)), below 2^32 because n <= m < 2^e
__device__ __forceinline__ unsigned long long smp_weight(double n, int e) { return (unsigned long long)ldexp(n, 32 - e); }

__device__ __forceinline__ int smp_exponent(const SamplerHead* head) {
    int e;
    (void)frexp(__longlong_as_double((long long)head->max_bits), &e);             // (0 gives 0)
    return e;
}

// One thread per triangle, no early return (block sums).  Classes, tested in this order: an index outside [0, V) (never dereferenced); SKIPPED: a
// coordinate that is not finite or reaches 2^60; the other two are told apart once the largest doubled area is known (k_smp_sum).
__global__ void __launch_bounds__(DIF_BLOCK) k_smp_weigh(Sampler S, const float* __restrict__ vertices, const int* __restrict__ tri, int K, int V) {
    __shared__ int smem[8];
    const long long t = (long long)blockIdx.x * DIF_BLOCK + threadIdx.x;
    int bad = 0, skipped = 0;
    double n = 0.0;
    if (t < K) {
        const int i0 = tri[3 * t], i1 = tri[3 * t + 1], i2 = tri[3 * t + 2];
        if ((unsigned)i0 >= (unsigned)V || (unsigned)i1 >= (unsigned)V || (unsigned)i2 >= (unsigned)V) {
            bad = 1;
        } else {
            float p[9];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                p[k] = vertices[3 * (long long)i0 + k];
                p[3 + k] = vertices[3 * (long long)i1 + k];
                p[6 + k] = vertices[3 * (long long)i2 + k];
            }
            bool ok = true;
#pragma unroll
            for (int k = 0; k < 9; ++k) ok = ok && fabsf(p[k]) < SMP_ABS_LIMIT;       // (NaN fails)
            if (!ok) {
                skipped = 1;
            } else {
                const double e1x = (double)p[3] - (double)p[0], e1y = (double)p[4] - (double)p[1], e1z = (double)p[5] - (double)p[2];
                const double e2x = (double)p[6] - (double)p[0], e2y = (double)p[7] - (double)p[1], e2z = (double)p[8] - (double)p[2];
                const double cx = e1y * e2z - e1z * e2y, cy = e1z * e2x - e1x * e2z, cz = e1x * e2y - e1y * e2x;
                n = sqrt((cx * cx + cy * cy) + cz * cz);
            }
        }
        S.norm[t] = n;
    }
    double m = n;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = fmax(m, __shfl_xor(m, d));
    if (lane_id() == 0 && m > 0.0) atomicMax(&S.head->max_bits, (unsigned long long)__double_as_longlong(m));
    const int nb = block_sum(bad, smem), ns = block_sum(skipped, smem);
    if (threadIdx.x == 0) {
        if (nb) { atomicAdd(&S.head->counts[DIF_SAMPLER_BAD_INDEX], nb); atomicOr(&S.head->counts[DIF_SAMPLER_STATUS], DIF_MESH_STATUS_BAD_INDEX); }
        if (ns) atomicAdd(&S.head->counts[DIF_SAMPLER_SKIPPED], ns);
    }
}

// the weights of one block's range of the scan (scan_range's partition), and how many of them are not zero
__global__ void __launch_bounds__(DIF_BLOCK) k_smp_sum(Sampler S, int K) {
    __shared__ unsigned long long smem[4];
    __shared__ int ismem[8];
    const int e = smp_exponent(S.head);
    int lo, hi;
    scan_range(K, lo, hi);
    unsigned long long sum = 0;
    int weighted = 0;
    for (int i = lo + (int)threadIdx.x; i < hi; i += DIF_BLOCK) {
        const unsigned long long w = smp_weight(S.norm[i], e);
        sum += w;
        weighted += w > 0;
    }
    const unsigned long long tot = smp_block_sum(sum, smem);
    const int nw = block_sum(weighted, ismem);
    if (threadIdx.x == 0) {
        S.block_tot[blockIdx.x] = tot;
        if (nw) atomicAdd(&S.head->counts[DIF_SAMPLER_WEIGHTED], nw);
    }
}

// P over one block's range; block 0 finishes the header and hands the counts and T out
__global__ void __launch_bounds__(DIF_BLOCK) k_smp_scan(Sampler S, int K, int* __restrict__ counts, unsigned long long* __restrict__ total_out) {
    __shared__ unsigned long long smem[4];
    const int e = smp_exponent(S.head);
    int lo, hi;
    scan_range(K, lo, hi);
    unsigned long long before = 0, all = 0;
    if (K > 0) {
        for (int b = (int)threadIdx.x; b < (int)gridDim.x; b += DIF_BLOCK) {
            const unsigned long long t = S.block_tot[b];
            all += t;
            if (b < (int)blockIdx.x) before += t;
        }
    }
    unsigned long long offset = smp_block_sum(before, smem);
    const unsigned long long total = smp_block_sum(all, smem);
    for (int base = lo; base < hi; base += DIF_BLOCK) {
        const int i = base + (int)threadIdx.x;
        const unsigned long long w = i < hi ? smp_weight(S.norm[i], e) : 0;
        unsigned long long chunk;
        const unsigned long long ex = smp_block_excl_scan(w, smem, chunk);
        if (i < hi) S.prefix[i] = offset + ex + w;
        offset += chunk;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        int* c = S.head->counts;
        c[DIF_SAMPLER_WEIGHTLESS] = K - c[DIF_SAMPLER_BAD_INDEX] - c[DIF_SAMPLER_SKIPPED] - c[DIF_SAMPLER_WEIGHTED];
        c[DIF_SAMPLER_EXPONENT] = e;
        S.head->total = total;
        for (int k = 0; k < DIF_SAMPLER_COUNT; ++k) counts[k] = c[k];
        *total_out = total;
    }
}

struct SampleOut { float* point; int* triangle; float* bary; };

// One thread per sample.  T = 0: every row is NaN / -1 / NaN.
__global__ void __launch_bounds__(DIF_BLOCK) k_smp_sample(Sampler S, const float* __restrict__ vertices, const int* __restrict__ tri, int K, int V, int N,
                                                          unsigned long long seed, SampleOut out, int* __restrict__ counts) {
    const unsigned long long T = S.head->total;
    const long long jl = (long long)blockIdx.x * DIF_BLOCK + threadIdx.x;
    if (jl == 0) {                                                                 // (counts were cleared by the call)
        counts[DIF_SAMPLE_SAMPLES] = T > 0 ? N : 0;
        atomicOr(&counts[DIF_SAMPLE_STATUS], S.head->counts[DIF_SAMPLER_STATUS]);
    }
    if (jl >= N) return;
    const unsigned long long j = (unsigned long long)jl, n = (unsigned long long)N;
    const float nan = __int_as_float(0x7FC00000);
    int chosen = -1;
    float b0 = nan, b1 = nan, b2 = nan, px = nan, py = nan, pz = nan;
    if (T > 0 && K > 0) {
        const unsigned long long base = smp_mix(seed);
        const unsigned long long r0 = smp_mix(base ^ smp_mix(2 * j)), r1 = smp_mix(base ^ smp_mix(2 * j + 1));
        const unsigned long long q = T / n, r = T % n;
        const unsigned long long lo_t = q * j + (r * j) / n, hi_t = q * (j + 1) + (r * (j + 1)) / n;      // r j < 2^62
        const unsigned long long width = hi_t - lo_t;                                                    // >= 1: T >= 2^31 > N
        const unsigned long long target = lo_t + (width ? r0 % width : 0);
        int lo = 0, hi = K;                                                                              // the first i with P[i] > target
        while (lo < hi) {
            const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
            if (S.prefix[mid] > target) hi = mid; else lo = mid + 1;
        }
        const int i = lo < K ? lo : K - 1;
        const int i0 = tri[3 * (long long)i], i1 = tri[3 * (long long)i + 1], i2 = tri[3 * (long long)i + 2];
        // (a triangle with a weight has its indices in range; a workspace that was not built for this mesh may say otherwise)
        if ((unsigned)i0 < (unsigned)V && (unsigned)i1 < (unsigned)V && (unsigned)i2 < (unsigned)V) {
            unsigned u = (unsigned)(r1 >> 40), v = (unsigned)(r1 >> 16) & 0xFFFFFFu;
            if (u + v > (1u << 24)) { u = (1u << 24) - u; v = (1u << 24) - v; }
            b1 = (float)u * 0x1p-24f;
            b2 = (float)v * 0x1p-24f;
            b0 = (float)((1u << 24) - u - v) * 0x1p-24f;
            const float* p0 = vertices + 3 * (long long)i0;
            const float* p1 = vertices + 3 * (long long)i1;
            const float* p2 = vertices + 3 * (long long)i2;
            px = (b0 * p0[0] + b1 * p1[0]) + b2 * p2[0];
            py = (b0 * p0[1] + b1 * p1[1]) + b2 * p2[1];
            pz = (b0 * p0[2] + b1 * p1[2]) + b2 * p2[2];
            chosen = i;
        } else {
            atomicOr(&counts[DIF_SAMPLE_STATUS], DIF_MESH_STATUS_BAD_INDEX);
        }
    }
    out.triangle[j] = chosen;
    out.point[3 * j] = px; out.point[3 * j + 1] = py; out.point[3 * j + 2] = pz;
    out.bary[3 * j] = b0; out.bary[3 * j + 1] = b1; out.bary[3 * j + 2] = b2;
}
