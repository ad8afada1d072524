// Walks the box grid of point_box_filter (di_fusion_amd/csrc/pbf_grid.hip.h) on the CPU: the verdict on clouds the grid cannot hold, and
// that every point of an accepted cloud lands in a cell of [0, cells).  Host code only; meant to be built with
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fsanitize=float-cast-overflow -fno-sanitize-recover=all -I di_fusion_amd/csrc tools/pbf_grid_check.cpp
// so that a float -> int conversion out of range or a signed overflow in the grid arithmetic ends the run.
// tests/test_frontend_cpu.py builds and runs it.  Prints one summary line and exits 0, or says what failed and exits 1.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <vector>

#include "pbf_grid.hip.h"

static int failures = 0;
static long accepted = 0, refused = 0, points_checked = 0;

#define EXPECT(cond, ...) do { if (!(cond)) { ++failures; std::fprintf(stderr, "FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); } } while (0)

// what k_pbf_bounds computes (min / max per axis; a NaN becomes the maximum or, with its sign bit set, the minimum, as in the ordered-uint encoding)
static void bounds_of(const std::vector<float>& p, float* lo, float* hi) {
    for (int a = 0; a < 3; ++a) {
        lo[a] = std::numeric_limits<float>::infinity(); hi[a] = -std::numeric_limits<float>::infinity();
        bool nan = false;
        for (size_t i = a; i < p.size(); i += 3) { if (p[i] != p[i]) nan = true; else { lo[a] = std::fmin(lo[a], p[i]); hi[a] = std::fmax(hi[a], p[i]); } }
        if (nan) hi[a] = std::numeric_limits<float>::quiet_NaN();
    }
}

// the verdict for a cloud, and for an accepted one the range of every point's cell; returns the verdict
static int walk(const std::vector<float>& p, float vs, int64_t max_cells, const char* what) {
    float lo[3], hi[3];
    bounds_of(p, lo, hi);
    BoxGrid G;
    const int verdict = pbf_grid(lo, hi, vs, max_cells, G);
    if (verdict != PBF_GRID_OK) {
        ++refused;
        EXPECT(G.n[0] == 0 && G.n[1] == 0 && G.n[2] == 0, "%s: a refused grid has counts", what);
        return verdict;
    }
    ++accepted;
    for (int a = 0; a < 3; ++a) EXPECT(G.n[a] >= 16 && (double)G.n[a] < 2147483632.0, "%s: n[%d] = %d", what, a, G.n[a]);
    const int64_t cells = (int64_t)G.n[0] * G.n[1] * G.n[2];
    EXPECT(cells > 0 && cells <= max_cells, "%s: cells %lld of %lld", what, (long long)cells, (long long)max_cells);
    for (size_t i = 0; i + 2 < p.size(); i += 3) {
        const int64_t c = pbf_cell(G, &p[i], vs);
        ++points_checked;
        EXPECT(c >= 0 && c < cells, "%s: point %zu (%g %g %g) -> cell %lld of %lld", what, i / 3, p[i], p[i + 1], p[i + 2], (long long)c, (long long)cells);
        if (!(c >= 0 && c < cells)) break;
    }
    return verdict;
}

int main() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const int64_t def_cells = (int64_t)1 << 27, big_cells = ((int64_t)1 << 36) - 1;       // the wrapper's default; the largest dif_point_box_filter takes
    std::mt19937 rng(20240611u);
    std::uniform_real_distribution<float> U(-1.0f, 1.0f);
    auto cloud = [&](int n, float scale, float cx, float cy, float cz) {
        std::vector<float> p((size_t)n * 3);
        for (int i = 0; i < n; ++i) { p[3 * i] = cx + scale * U(rng); p[3 * i + 1] = cy + scale * U(rng); p[3 * i + 2] = cz + scale * U(rng); }
        return p;
    };

    // ---- non-finite bounds: refused as such whatever the axis, the sign and max_cells
    const float bad[] = {nan, -nan, inf, -inf};
    for (float b : bad)
        for (int a = 0; a < 3; ++a)
            for (int64_t mc : {(int64_t)4096, def_cells, big_cells}) {
                std::vector<float> p = cloud(65, 1.0f, 0.0f, 0.0f, 2.0f);
                p[3 * 17 + a] = b;
                EXPECT(walk(p, 0.02f, mc, "non-finite") == PBF_GRID_NOT_FINITE, "value %g on axis %d, max_cells %lld", b, a, (long long)mc);
            }
    {   // bounds given directly, as the device decodes them
        BoxGrid G;
        const float lo[3] = {0.0f, 0.0f, 0.0f}, hi_nan[3] = {1.0f, nan, 1.0f}, lo_inf[3] = {-inf, 0.0f, 0.0f}, hi[3] = {1.0f, 1.0f, 1.0f};
        EXPECT(pbf_grid(lo, hi_nan, 0.02f, def_cells, G) == PBF_GRID_NOT_FINITE, "NaN upper bound");
        EXPECT(pbf_grid(lo_inf, hi, 0.02f, def_cells, G) == PBF_GRID_NOT_FINITE, "-Inf lower bound");
        EXPECT(pbf_grid(lo, hi, inf, def_cells, G) == PBF_GRID_NOT_FINITE, "infinite voxel_size");
        const float lo_max[3] = {-3.0e38f, 0.0f, 0.0f}, hi_max[3] = {3.0e38f, 1.0f, 1.0f};      // finite bounds whose difference is not
        EXPECT(pbf_grid(lo_max, hi_max, 0.02f, big_cells, G) == PBF_GRID_TOO_MANY_CELLS, "extent beyond FLT_MAX");
    }

    // ---- a far outlier: extent 1e12 (and more) at every voxel_size down to 1e-6; per-axis count far beyond int
    for (float far : {1.0e12f, -1.0e12f, 3.0e9f, 1.0e30f})
        for (float vs : {1.0f, 0.05f, 0.02f, 1.0e-3f, 1.0e-6f})
            for (int a = 0; a < 3; ++a) {
                std::vector<float> p = cloud(64, 1.0f, 0.0f, 0.0f, 2.0f);
                p[3 * 5 + a] = far;
                EXPECT(walk(p, vs, big_cells, "outlier") == PBF_GRID_TOO_MANY_CELLS, "outlier %g on axis %d at voxel_size %g", far, a, vs);
            }
    // an axis count just on either side of what max_cells admits (256 boxes on the two thin axes)
    {
        std::vector<float> p = {0.0f, 0.0f, 0.0f, 1000.0f, 0.0f, 0.0f};
        EXPECT(walk(p, 1.0f, (int64_t)1017 * 17 * 17, "thin") == PBF_GRID_OK, "1017 x 17 x 17 fits exactly");
        EXPECT(walk(p, 1.0f, (int64_t)1017 * 17 * 17 - 1, "thin") == PBF_GRID_TOO_MANY_CELLS, "one cell short");
    }

    // ---- small voxels: a 1 m cloud at voxel_size 1e-6 is ~1e6 boxes per axis (refused), a tiny cloud at the same voxel_size is not
    EXPECT(walk(cloud(257, 0.5f, 0.0f, 0.0f, 1.0f), 1.0e-6f, big_cells, "1 m at 1e-6") == PBF_GRID_TOO_MANY_CELLS, "1 m cloud at voxel_size 1e-6");
    for (float vs : {1.0e-6f, 1.0e-5f, 1.0e-4f, 1.0e-3f})
        for (int rep = 0; rep < 20; ++rep) {
            const float c = rep % 2 ? 0.0f : vs * 1000.0f;            // around the origin, and where the coordinates' spacing is near voxel_size / 10
            EXPECT(walk(cloud(257, vs * 20.0f, c, -c, c), vs, def_cells, "tiny voxels") == PBF_GRID_OK, "cloud of 40 voxels across at voxel_size %g", vs);
        }

    // ---- ordinary clouds: a room's worth of points at the tracker's voxel sizes, off-centre, negative coordinates, degenerate extents
    for (float vs : {0.02f, 0.05f, 0.1f, 1.0f})
        for (int rep = 0; rep < 25; ++rep) {
            const float s = 0.25f + 0.25f * (float)(rep % 8);
            EXPECT(walk(cloud(2000, s, 3.0f * U(rng), 3.0f * U(rng), 3.0f * U(rng)), vs, def_cells, "ordinary") == PBF_GRID_OK, "scale %g voxel_size %g", s, vs);
        }
    EXPECT(walk({1.5f, -2.5f, 0.25f}, 0.02f, 4096, "one point") == PBF_GRID_OK, "one point is a 16^3 grid");
    EXPECT(walk({1.5f, -2.5f, 0.25f}, 0.02f, 4095, "one point") == PBF_GRID_TOO_MANY_CELLS, "16^3 > 4095");
    EXPECT(walk({-0.0f, 0.0f, -0.0f, 0.0f, -0.0f, 0.0f}, 0.02f, def_cells, "zeros") == PBF_GRID_OK, "signed zeros");
    {   // points on a lattice of exact multiples of voxel_size: every quotient sits on a floor() boundary
        std::vector<float> p;
        for (int i = -20; i <= 20; ++i) for (int j = -3; j <= 3; ++j) { p.push_back(0.25f * (float)i); p.push_back(0.25f * (float)j); p.push_back(0.25f * (float)(i + j)); }
        EXPECT(walk(p, 0.25f, def_cells, "lattice") == PBF_GRID_OK, "lattice");
        EXPECT(walk(p, 0.125f, def_cells, "lattice") == PBF_GRID_OK, "lattice, half voxels");
    }
    {   // large but representable: 4 km at 1 m voxels is too much for 2^27 cells and fine for 2^36 - 1
        std::vector<float> p = cloud(1000, 2000.0f, 0.0f, 0.0f, 0.0f);
        EXPECT(walk(p, 1.0f, def_cells, "4 km") == PBF_GRID_TOO_MANY_CELLS, "4 km at 1 m: 2^27 cells");
        EXPECT(walk(p, 2.0f, big_cells, "4 km") == PBF_GRID_OK, "4 km at 2 m: 2^36 cells");
    }

    std::printf("pbf_grid_check: %ld grids accepted (%ld points, every cell in range), %ld refused, %d failures\n", accepted, points_checked, refused, failures);
    return failures ? 1 : 0;
}
