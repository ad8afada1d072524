// The box grid of point_box_filter (system/tracker.py:15-19) and its input contract, in plain C++ for host and device: the kernels of
// kernels_points.hip.h include it, and tools/pbf_grid_check.cpp walks it on the CPU under the sanitizers.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PBF_HD __host__ __device__ __forceinline__
#else
#define PBF_HD inline
#endif

struct BoxGrid { float minb[3]; int n[3]; };

// verdicts of pbf_grid; the non-zero ones are what dif_point_box_filter leaves in scratch[4102] (include/difusion.h)
#define PBF_GRID_OK 0
#define PBF_GRID_TOO_MANY_CELLS 1      /* an axis count >= 2^31 - 16, or n_x * n_y * n_z > max_cells */
#define PBF_GRID_NOT_FINITE 2          /* a NaN or infinite coordinate (or a voxel_size that makes a bound infinite) */

// lo / hi: the cloud's bounding box.  The grid of tracker.py:15-18 in the reference's float arithmetic; the verdict is taken in double,
// before anything is converted to an integer.  PBF_GRID_OK promises: every n[a] is in [16, 2^31 - 16), cells = n_x * n_y * n_z <=
// max_cells, and pbf_cell of any point inside [lo, hi] lies in [0, cells).  On any other verdict G.n is all zero.
PBF_HD int pbf_grid(const float* lo, const float* hi, float vs, int64_t max_cells, BoxGrid& G) {
    double cnt[3];
    int verdict = PBF_GRID_OK;
    for (int a = 0; a < 3; ++a) {
        const float mn = lo[a] - vs * 0.5f, mx = hi[a] + vs * 0.5f;                      // tracker.py:15-16
        G.minb[a] = mn;
        G.n[a] = 0;
        cnt[a] = 0.0;
        if (!(mn - mn == 0.0f) || !(mx - mx == 0.0f)) { verdict = PBF_GRID_NOT_FINITE; continue; }      // x - x is 0 only for a finite x
        cnt[a] = (double)floorf((mx - mn) / vs) + 16.0;                                   // tracker.py:18
        if (!(cnt[a] >= 16.0 && cnt[a] < 2147483632.0) && verdict == PBF_GRID_OK) verdict = PBF_GRID_TOO_MANY_CELLS;
    }
    if (verdict == PBF_GRID_OK) {
        const double xy = cnt[0] * cnt[1];                       // < 2^62; exact wherever it can pass the test (max_cells < 2^36)
        if (xy > (double)max_cells || xy * cnt[2] > (double)max_cells) verdict = PBF_GRID_TOO_MANY_CELLS;
    }
    if (verdict == PBF_GRID_OK)
        for (int a = 0; a < 3; ++a) G.n[a] = (int)cnt[a];
    return verdict;
}

PBF_HD int64_t pbf_cell(const BoxGrid& G, const float* p, float vs) {
    int64_t cx = (int64_t)floorf((p[0] - G.minb[0]) / vs), cy = (int64_t)floorf((p[1] - G.minb[1]) / vs), cz = (int64_t)floorf((p[2] - G.minb[2]) / vs);
    return cx + cy * G.n[0] + cz * (int64_t)G.n[0] * G.n[1];                          // tracker.py:17,19
}
