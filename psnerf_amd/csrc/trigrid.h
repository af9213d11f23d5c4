// The uniform grid of triangle lists (PsnTriGrid) as its builder and its two queries see it: csrc/meshdist.hip builds it and asks
// for the closest point, csrc/meshray.hip casts rays through it.  Both must map a coordinate to a cell in exactly one way, so the
// mapping lives here.
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
static inline unsigned md_blocks(int64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace psn
