// Crossing counts of an axis-parallel line with a triangle mesh on the device, over the uniform grid of triangle lists that
// csrc/meshdist.hip builds (the grid's conventions are in csrc/trigrid.h).
//   psn_mesh_crossings   per point p: how many triangles of the WHOLE mesh the line through p along ``axis`` crosses above p, below
//                        p and exactly at p.  inside = above & 1; (above + below + on) & 1 says the line sees no closed surface.
// Geometry is float64 throughout and -ffp-contract=off, so the test below rounds exactly as the numpy definition
// psnerf_amd/meshdist.py:host_crossings does.  A thread per point; the counter is an integer atomic aggregated per wave.
//
// The test.  kz = axis, kx = (axis + 1) % 3, ky = (axis + 2) % 3 (the direction is +1: no swap).  The corners are translated by -p
// and nothing else: it is meshray.hip's watertight test with S = (0, 0, 1), written without the shear.  U, V, W are the directed-
// edge functions e(P, Q) = Qx Py - Qy Px of (B, C), (C, A), (A, B) in that file's order; the two products commute, so
// e(Q, P) = -e(P, Q) holds exactly in floating point.
//   The tie rule.  A first hit may accept a ray through a shared edge for both triangles; a parity may not.  The side of an edge is
//   decided by simulation of simplicity, p moved by (+d, +d^2) in (kx, ky) for an infinitesimal d: e becomes
//   e + d (Qy - Py) + d^2 (Px - Qx) (the d^3 terms cancel), hence
//       s(P, Q) = sign(e), or if that is 0 sign(Qy - Py), or if that is 0 sign(Px - Qx), or 0 (P = Q; a NaN e gives 0 too).
//   Every term changes sign when P and Q are exchanged, so s(Q, P) = -s(P, Q): of two triangles on opposite sides of a shared edge,
//   which run through it in opposite directions, exactly one owns a point of the edge; two on the same side both own it or neither.
//   A triangle is accepted when the line lies in the closed bounding box of its projection (min <= 0 <= max over Ax, Bx, Cx and over
//   Ay, By, Cy: exact comparisons, since a rounded difference has the sign of the exact one), sU = sV = sW != 0 and
//   det = U + V + W != 0; then z = (U Az + V Bz + W Cz) / det and it counts above for z > 0, below for z < 0, on for z == 0, nowhere
//   for a non-finite z.  The box is implied by the sides in exact arithmetic; it is there for slivers: when the projected corners
//   and p are collinear up to rounding, U, V and W are all rounding noise and can agree in sign for a p anywhere on that line.
//   Zero-area and edge-on triangles are never counted (two equal translated corners give one s = 0 or det = 0); a point with a
//   non-finite coordinate gets three zeros.
//
// The walk, and why it is conservative.  The counts are defined without the grid, so the grid may only ever save tests.  An
// accepted triangle T has p[kx] and p[ky] inside its bounding box, exactly; md_cell is monotone, so T's cell range (md_range, the
// builder's own) contains the cell of p[kx] on kx and of p[ky] on ky.  And U, V, W of one sign make z a combination of Az, Bz, Cz with
// weights of one sign: z >= 0 needs a corner with Az >= 0, which puts T's upper end along kz at or above the cell of p[kz].  The walk
// visits more than that: with the margin m = 1e-9 x cell + 1e-12 x scale (scale = the largest |coordinate| of p and of the grid's
// box; meshray.hip's, some thousand times every rounding of md_cell) the rectangle of columns md_cell(p[kx] -+ m) x
// md_cell(p[ky] -+ m) -- one column, two by two when p sits on a column boundary; no comparison ever chooses a single neighbour --
// and along kz every cell of the column when ``below`` is wanted, else the cells from md_cell(p[kz] - m) upward.  T is a mesh
// triangle, so it lies in the grid's box: a point outside the box -+ m in kx or ky is in no triangle's box and writes zeros without
// walking.  Oversize triangles are in no cell list; every walking point tests the oversize list once.
//
// Each triangle exactly once.  A triangle is listed in every cell of its range [c0, c1] (per axis), so the walk meets it in every
// visited cell of that range; a count must not depend on how many those are.  The visited cells form a box [f, l] per axis
// (f = the first visited index).  T is met if and only if [c0, c1] and [f, l] intersect on all three axes, i.e. max(c0, f) <=
// min(c1, l) on each; and then the cell (max(c0, f)) per axis lies in both, is visited, lists T, and is the only visited cell with
// those three indices.  So T is tested at visited cell (i, j, k) only when each index equals max(c0, f) on its axis: exactly once if
// it is met at all, never otherwise -- whatever the order of the lists.  The check comes before the edge functions; n_tests counts
// the triangles that pass it, so it can not exceed Q x F.
//
// Block shape.  Points arrive sorted by column, then by cell along the axis, so the lanes of a wave read the same cell_start
// entries and the same list entries (one fetch serves the wave) and leave the loops together; what divergence remains is between
// columns of different length.  That holds for the whole-column walk.  The upward-only walk starts each lane at its own cell, the
// lanes of a column leave lockstep, and although it does half the tests it measures five times slower on sorted points
// (profiles/mesh_inside.json).  There is no LDS and no barrier, so a block is one wave of 64: nothing ties a finished wave to a
// longer column next to it.  ``axis`` is a template parameter: every index into p, the grid and a triangle's range is a constant,
// and nothing per-thread is addressed at run time.
#include "trigrid.h"

namespace psn {

__device__ __forceinline__ int mi_side(double e, double Px, double Py, double Qx, double Qy) {
    if (e > 0.0) return 1;
    if (e < 0.0) return -1;
    if (!(e == 0.0)) return 0;
    if (Qy > Py) return 1;
    if (Qy < Py) return -1;
    if (Px > Qx) return 1;
    if (Px < Qx) return -1;
    return 0;
}

// Operation for operation meshdist.py:_line_triangles.  (ax .. cz): the corners' (kx, ky, kz) coordinates.
__device__ __forceinline__ void mi_count(double px, double py, double pz, double ax, double ay, double az, double bx, double by, double bz,
                                         double cx, double cy, double cz, int& above, int& below, int& on) {
    const double Ax = ax - px, Ay = ay - py, Az = az - pz;
    const double Bx = bx - px, By = by - py, Bz = bz - pz;
    const double Cx = cx - px, Cy = cy - py, Cz = cz - pz;
    if (!(md_min3(Ax, Bx, Cx) <= 0.0 && md_max3(Ax, Bx, Cx) >= 0.0 && md_min3(Ay, By, Cy) <= 0.0 && md_max3(Ay, By, Cy) >= 0.0)) return;
    const double U = Cx * By - Cy * Bx;
    const double V = Ax * Cy - Ay * Cx;
    const double W = Bx * Ay - By * Ax;
    const int sU = mi_side(U, Bx, By, Cx, Cy);
    if (sU == 0 || mi_side(V, Cx, Cy, Ax, Ay) != sU || mi_side(W, Ax, Ay, Bx, By) != sU) return;
    const double det = U + V + W;
    if (!(det != 0.0)) return;
    const double z = (U * Az + V * Bz + W * Cz) / det;
    if (!(z - z == 0.0)) return;
    if (z > 0.0) ++above;
    else if (z < 0.0) ++below;
    else ++on;
}

template <int AXIS>
__device__ __forceinline__ void mi_count_tri(const double (&p)[3], const MdTri& t, int& above, int& below, int& on) {
    constexpr int KX = (AXIS + 1) % 3, KY = (AXIS + 2) % 3, KZ = AXIS;
    const double a[3] = {t.ax, t.ay, t.az}, b[3] = {t.bx, t.by, t.bz}, c[3] = {t.cx, t.cy, t.cz};
    mi_count(p[KX], p[KY], p[KZ], a[KX], a[KY], a[KZ], b[KX], b[KY], b[KZ], c[KX], c[KY], c[KZ], above, below, on);
}

// One thread per point, points taken in the caller's order.  The walk, the once-only rule and the block shape: the head of this file.
template <int AXIS>
__global__ __launch_bounds__(64) void mesh_crossings_kernel(PsnMeshIndex ix, const double* __restrict__ points, const int64_t* __restrict__ order,
                                                            int64_t n_points, int* __restrict__ above_out, int* __restrict__ below_out,
                                                            int* __restrict__ on_out, unsigned long long* __restrict__ n_tests) {
    const PsnTriGrid& g = ix.grid;
    const double* __restrict__ vertices = ix.vertices; const int64_t* __restrict__ faces = ix.faces;
    const int* __restrict__ cell_start = ix.cell_start; const int* __restrict__ list = ix.list;
    const int* __restrict__ over_list = ix.over_list; const int64_t n_over = ix.n_over;
    constexpr int KX = (AXIS + 1) % 3, KY = (AXIS + 2) % 3, KZ = AXIS;
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    unsigned int tests = 0;
    if (i < n_points) {
        const int64_t q = order != nullptr ? order[i] : i;
        const double p[3] = {points[3 * q], points[3 * q + 1], points[3 * q + 2]};
        int above = 0, below = 0, on = 0;
        if (p[0] - p[0] == 0.0 && p[1] - p[1] == 0.0 && p[2] - p[2] == 0.0) {
            const double cell = g.cell, inv = 1.0 / cell;
            double scale = fmax(fabs(p[0]), fmax(fabs(p[1]), fabs(p[2])));
#pragma unroll
            for (int a = 0; a < 3; ++a) scale = fmax(scale, fmax(fabs(g.lo[a]), fabs(g.lo[a] + (double)g.n[a] * cell)));
            const double m = 1e-9 * cell + 1e-12 * scale;
            if (!(p[KX] < g.lo[KX] - m || p[KX] > g.hi[KX] + m || p[KY] < g.lo[KY] - m || p[KY] > g.hi[KY] + m)) {
                for (int64_t k = 0; k < n_over; ++k) {
                    ++tests;
                    mi_count_tri<AXIS>(p, md_load(vertices, faces, over_list[k]), above, below, on);
                }
                const int i0 = md_cell(p[KX] - m, g.lo[KX], inv, g.n[KX]), i1 = min(md_cell(p[KX] + m, g.lo[KX], inv, g.n[KX]), i0 + 1);
                const int j0 = md_cell(p[KY] - m, g.lo[KY], inv, g.n[KY]), j1 = min(md_cell(p[KY] + m, g.lo[KY], inv, g.n[KY]), j0 + 1);
                const int k0 = below_out != nullptr ? 0 : md_cell(p[KZ] - m, g.lo[KZ], inv, g.n[KZ]);
                const int64_t stride[3] = {(int64_t)g.n[1] * g.n[2], g.n[2], 1};
                for (int ci = i0; ci <= i1; ++ci)            // (at most 2 x 2 x n[kz] cells, whatever the input)
                    for (int cj = j0; cj <= j1; ++cj)
                        for (int ck = k0; ck < g.n[KZ]; ++ck) {
                            const int64_t c = ci * stride[KX] + cj * stride[KY] + ck * stride[KZ];
                            const int e = cell_start[c + 1];
                            for (int k = cell_start[c]; k < e; ++k) {
                                const MdTri t = md_load(vertices, faces, list[k]);
                                int c0[3], c1[3];
                                md_range(g, t, c0, c1);
                                if (ci != max(c0[KX], i0) || cj != max(c0[KY], j0) || ck != max(c0[KZ], k0)) continue;
                                ++tests;
                                mi_count_tri<AXIS>(p, t, above, below, on);
                            }
                        }
            }
        }
        above_out[q] = above;
        if (below_out != nullptr) below_out[q] = below;
        if (on_out != nullptr) on_out[q] = on;
    }
    md_add_tests(n_tests, tests);   // one atomic per wave (every lane reaches this point)
}

}  // namespace psn

// The query.  points [n_points, 3]; order: null, or a permutation of 0 .. n_points - 1 in which the points are taken (sorted by
// column, then by cell along the axis); outputs are written at the point's own row whatever the order.  above [n_points]; below, on
// [n_points] or null (without below the walk starts at the point's own cell; above and on do not change).  n_tests: null, or one
// counter to which the number of line-triangle tests is ADDED.
extern "C" int psn_mesh_crossings(const PsnMeshIndex* index, const double* points, const int64_t* order, int64_t n_points, int axis, int* above,
                                  int* below, int* on, long long* n_tests, void* stream) {
    using namespace psn;
    if (int rc = md_check_index(index, "mesh_crossings")) return rc;
    PSN_CHECK_ARG(n_points >= 0 && n_points <= PSN_CROSSINGS_MAX_POINTS, "mesh_crossings: n_points=%lld (0 .. %lld)", (long long)n_points,
                  (long long)PSN_CROSSINGS_MAX_POINTS);
    PSN_CHECK_ARG(axis >= 0 && axis <= 2, "mesh_crossings: axis=%d (0 .. 2)", axis);
    if (n_points == 0) return PSN_OK;
    PSN_CHECK_ARG(points && above, "mesh_crossings: null point / output pointer");
    const dim3 blocks((unsigned)((n_points + 63) / 64)), threads(64);
    const auto kernel = axis == 0 ? mesh_crossings_kernel<0> : (axis == 1 ? mesh_crossings_kernel<1> : mesh_crossings_kernel<2>);
    hipLaunchKernelGGL(kernel, blocks, threads, 0, (hipStream_t)stream, *index, points, order, n_points, above, below, on,
                       reinterpret_cast<unsigned long long*>(n_tests));
    PSN_CHECK_LAUNCH("mesh_crossings");
    return PSN_OK;
}
