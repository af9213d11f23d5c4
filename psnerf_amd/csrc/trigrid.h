// The uniform grid of triangle lists (PsnTriGrid) as its builder and its queries see it: csrc/meshdist.hip builds it and asks
// for the closest point, csrc/meshray.hip casts rays through it, csrc/meshinside.hip counts a line's crossings in it.  All must map
// a coordinate to a cell, and a triangle to its range of cells, in exactly one way, so both mappings live here; so do the one check of
// the index the queries take (PsnMeshIndex) and the per-wave counter reduction they share.
#pragma once
#include "common.h"

namespace psn {

__device__ __forceinline__ int md_lane() { return threadIdx.x & 63; }

// the cell of coordinate x on one axis, clamped into the grid (NaN -> 0).  Monotone in x: a rounded subtraction and a rounded
// product with a positive constant are monotone, floor and the clamp are.
__device__ __forceinline__ int md_cell(double x, double lo, double inv_cell, int n) {
    const double t = floor((x - lo) * inv_cell);
    if (!(t >= 0.0)) return 0;
    return t > (double)(n - 1) ? n - 1 : (int)t;
}

struct MdTri {
    double ax, ay, az, bx, by, bz, cx, cy, cz;
};
__device__ __forceinline__ MdTri md_load(const double* __restrict__ v, const int64_t* __restrict__ f, int64_t t) {
    const int64_t i = f[3 * t], j = f[3 * t + 1], k = f[3 * t + 2];
    return MdTri{v[3 * i], v[3 * i + 1], v[3 * i + 2], v[3 * j], v[3 * j + 1], v[3 * j + 2], v[3 * k], v[3 * k + 1], v[3 * k + 2]};
}

__device__ __forceinline__ double md_min3(double a, double b, double c) { return fmin(a, fmin(b, c)); }
__device__ __forceinline__ double md_max3(double a, double b, double c) { return fmax(a, fmax(b, c)); }

// the cell range of a triangle's bounding box; returns the number of cells
__device__ __forceinline__ int64_t md_range(const PsnTriGrid& g, const MdTri& t, int* c0, int* c1) {
    const double inv = 1.0 / g.cell;
    c0[0] = md_cell(md_min3(t.ax, t.bx, t.cx), g.lo[0], inv, g.n[0]);
    c1[0] = md_cell(md_max3(t.ax, t.bx, t.cx), g.lo[0], inv, g.n[0]);
    c0[1] = md_cell(md_min3(t.ay, t.by, t.cy), g.lo[1], inv, g.n[1]);
    c1[1] = md_cell(md_max3(t.ay, t.by, t.cy), g.lo[1], inv, g.n[1]);
    c0[2] = md_cell(md_min3(t.az, t.bz, t.cz), g.lo[2], inv, g.n[2]);
    c1[2] = md_cell(md_max3(t.az, t.bz, t.cz), g.lo[2], inv, g.n[2]);
    return (int64_t)(c1[0] - c0[0] + 1) * (c1[1] - c0[1] + 1) * (c1[2] - c0[2] + 1);
}

// the sum of a per-lane count over the wave, added to the counter once (every lane of the wave must call this)
__device__ __forceinline__ void md_add_tests(unsigned long long* __restrict__ n_tests, unsigned int tests) {
    if (n_tests == nullptr) return;
    unsigned long long s = tests;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    if (md_lane() == 0 && s > 0) atomicAdd(n_tests, s);
}

static inline int md_check_grid(const PsnTriGrid* g, const char* what) {
    PSN_CHECK_ARG(g != nullptr, "%s: null grid descriptor", what);
    PSN_CHECK_ARG(g->cell > 0.0 && g->cell < __builtin_inf(), "%s: cell size %g", what, g->cell);
    for (int a = 0; a < 3; ++a) {
        PSN_CHECK_ARG(g->n[a] >= 1 && g->n[a] <= PSN_TRI_GRID_MAX_CELLS_PER_AXIS, "%s: %d cells on axis %d (1 .. %d)", what, g->n[a], a,
                      PSN_TRI_GRID_MAX_CELLS_PER_AXIS);
        PSN_CHECK_ARG(g->lo[a] <= g->hi[a] && g->lo[a] - g->lo[a] == 0.0 && g->hi[a] - g->hi[a] == 0.0, "%s: bounding box [%g, %g] on axis %d", what,
                      g->lo[a], g->hi[a], a);
    }
    PSN_CHECK_ARG(g->max_span >= 1, "%s: max_span=%d", what, g->max_span);
    return PSN_OK;
}
// the PsnMeshIndex of a query, as include/psnerf_hip.h states it
static inline int md_check_index(const PsnMeshIndex* ix, const char* what) {
    PSN_CHECK_ARG(ix != nullptr, "%s: null index", what);
    if (int rc = md_check_grid(&ix->grid, what)) return rc;
    PSN_CHECK_ARG(ix->vertices && ix->faces && ix->cell_start, "%s: null pointer", what);
    PSN_CHECK_ARG(ix->n_faces >= 1 && ix->n_faces <= PSN_TRI_GRID_MAX_FACES, "%s: n_faces=%lld (1 .. %lld)", what, (long long)ix->n_faces,
                  (long long)PSN_TRI_GRID_MAX_FACES);
    PSN_CHECK_ARG(ix->n_over >= 0 && ix->n_over <= ix->n_faces && (ix->n_over == 0 || ix->over_list), "%s: n_over=%lld / null oversize list", what,
                  (long long)ix->n_over);
    PSN_CHECK_ARG(ix->n_over == ix->n_faces || ix->list, "%s: null cell list", what);
    return PSN_OK;
}
static inline unsigned md_blocks(int64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace psn
