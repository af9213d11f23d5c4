// Point-to-mesh distance on the device: what the reference asks of trimesh.proximity.closest_point (chamfer_dist.py:24-25,
// stage2/utils/metrics.py:84-85,107), over a uniform grid of triangle lists instead of an r-tree.
//   psn_tri_grid_count   per triangle: the cells its bounding box overlaps -> per-cell counts; triangles that span more than
//                        max_span cells go to a short "oversize" list instead (every query tests those directly)
//   psn_tri_grid_fill    the triangle ids into the cell lists (positions from the caller's exclusive scan of the counts)
//   psn_closest_point    per query point: closest point, distance and triangle id over the WHOLE mesh
// Geometry is float64 throughout (the vertices are float64 since marching cubes; -ffp-contract=off, so every formula below rounds
// as the numpy definition psnerf_amd/meshdist.py:host_closest_point does).  A thread per triangle / per query point; counters
// are integer atomics aggregated per wave.  The order of the ids within a cell list (and of the oversize list) is not defined;
// the query's result does not depend on it: it is the minimum of (squared distance, triangle id) in lexicographic order.
#include "trigrid.h"

namespace psn {

__global__ __launch_bounds__(256) void tri_grid_count_kernel(PsnTriGrid g, const double* __restrict__ vertices, const int64_t* __restrict__ faces,
                                                             int64_t n_faces, int* __restrict__ cell_count, int* __restrict__ over_list,
                                                             unsigned long long* __restrict__ n_over) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool over = false;
    if (t < n_faces) {
        int c0[3], c1[3];
        const int64_t span = md_range(g, md_load(vertices, faces, t), c0, c1);
        over = span > g.max_span;
        if (!over)
            for (int x = c0[0]; x <= c1[0]; ++x)
                for (int y = c0[1]; y <= c1[1]; ++y)
                    for (int z = c0[2]; z <= c1[2]; ++z) atomicAdd(cell_count + ((int64_t)x * g.n[1] + y) * g.n[2] + z, 1);
    }
    // the oversize list: one atomic per wave (every lane reaches this point)
    const unsigned long long m = __ballot(over);
    if (m == 0ull) return;   // wave-uniform
    const int lane = md_lane(), leader = __ffsll((long long)m) - 1;
    unsigned long long base = 0;
    if (lane == leader) base = atomicAdd(n_over, (unsigned long long)__popcll(m));
    base = __shfl(base, leader, 64);
    if (over) over_list[base + __popcll(m & ((1ull << lane) - 1ull))] = (int)t;
}

__global__ __launch_bounds__(256) void tri_grid_fill_kernel(PsnTriGrid g, const double* __restrict__ vertices, const int64_t* __restrict__ faces,
                                                            int64_t n_faces, int* __restrict__ cursor, int64_t n_entries, int* __restrict__ list) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_faces) return;
    int c0[3], c1[3];
    if (md_range(g, md_load(vertices, faces, t), c0, c1) > g.max_span) return;
    for (int x = c0[0]; x <= c1[0]; ++x)
        for (int y = c0[1]; y <= c1[1]; ++y)
            for (int z = c0[2]; z <= c1[2]; ++z) {
                const int at = atomicAdd(cursor + ((int64_t)x * g.n[1] + y) * g.n[2] + z, 1);
                if (at >= 0 && at < n_entries) list[at] = (int)t;   // (a scan that does not belong to these counts must not write out of bounds)
            }
}

// The point of segment [a, b] closest to p (a zero-length segment is the point a).
__device__ __forceinline__ void md_segment(double px, double py, double pz, double ax, double ay, double az, double bx, double by, double bz,
                                           double& qx, double& qy, double& qz) {
    const double ex = bx - ax, ey = by - ay, ez = bz - az;
    const double num = ex * (px - ax) + ey * (py - ay) + ez * (pz - az);
    const double den = ex * ex + ey * ey + ez * ez;
    double s = den > 0.0 ? num / den : 0.0;
    s = s < 0.0 ? 0.0 : (s > 1.0 ? 1.0 : s);
    qx = ax + s * ex; qy = ay + s * ey; qz = az + s * ez;
}
__device__ __forceinline__ double md_dist2(double px, double py, double pz, double qx, double qy, double qz) {
    const double dx = px - qx, dy = py - qy, dz = pz - qz;
    return dx * dx + dy * dy + dz * dz;
}

// The point of the closed triangle (a, b, c) closest to p: the Voronoi-region test of Ericson, Real-Time Collision Detection
// 5.1.5, operation for operation as meshdist.py:_closest_on_triangles.  Zero-area triangles end in a vertex or edge region (no
// division by the area).  Two additions to the book's code: an edge of zero length (a repeated corner) is no edge region -- its
// test would pass trivially and return the corner --, and where rounding sends a sliver through to the face region with a
// vanishing or negative normal^2, or with barycentric coordinates outside the triangle, the best of the three edges is taken.
__device__ __forceinline__ void md_closest(double px, double py, double pz, const MdTri& t, double& qx, double& qy, double& qz) {
    const double abx = t.bx - t.ax, aby = t.by - t.ay, abz = t.bz - t.az;
    const double acx = t.cx - t.ax, acy = t.cy - t.ay, acz = t.cz - t.az;
    const double apx = px - t.ax, apy = py - t.ay, apz = pz - t.az;
    const double d1 = abx * apx + aby * apy + abz * apz, d2 = acx * apx + acy * apy + acz * apz;
    if (d1 <= 0.0 && d2 <= 0.0) { qx = t.ax; qy = t.ay; qz = t.az; return; }
    const double bpx = px - t.bx, bpy = py - t.by, bpz = pz - t.bz;
    const double d3 = abx * bpx + aby * bpy + abz * bpz, d4 = acx * bpx + acy * bpy + acz * bpz;
    if (d3 >= 0.0 && d4 <= d3) { qx = t.bx; qy = t.by; qz = t.bz; return; }
    const double cpx = px - t.cx, cpy = py - t.cy, cpz = pz - t.cz;
    const double d5 = abx * cpx + aby * cpy + abz * cpz, d6 = acx * cpx + acy * cpy + acz * cpz;
    if (d6 >= 0.0 && d5 <= d6) { qx = t.cx; qy = t.cy; qz = t.cz; return; }
    const double vc = d1 * d4 - d3 * d2;
    if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0 && d1 - d3 > 0.0) {   // (d1 - d3 = |ab|^2: an edge of zero length is no edge region)
        const double v = d1 / (d1 - d3);
        qx = t.ax + v * abx; qy = t.ay + v * aby; qz = t.az + v * abz;
        return;
    }
    const double vb = d5 * d2 - d1 * d6;
    if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0 && d2 - d6 > 0.0) {
        const double w = d2 / (d2 - d6);
        qx = t.ax + w * acx; qy = t.ay + w * acy; qz = t.az + w * acz;
        return;
    }
    const double va = d3 * d6 - d5 * d4;
    const double e43 = d4 - d3, e56 = d5 - d6;
    if (va <= 0.0 && e43 >= 0.0 && e56 >= 0.0 && e43 + e56 > 0.0) {
        const double w = e43 / (e43 + e56);
        qx = t.bx + w * (t.cx - t.bx); qy = t.by + w * (t.cy - t.by); qz = t.bz + w * (t.cz - t.bz);
        return;
    }
    const double sum = va + vb + vc;
    const double v = vb / sum, w = vc / sum;
    if (sum > 0.0 && v >= 0.0 && w >= 0.0 && v + w <= 1.0) {
        qx = t.ax + abx * v + acx * w; qy = t.ay + aby * v + acy * w; qz = t.az + abz * v + acz * w;
        return;
    }
    double ex, ey, ez;
    md_segment(px, py, pz, t.ax, t.ay, t.az, t.bx, t.by, t.bz, qx, qy, qz);
    double best = md_dist2(px, py, pz, qx, qy, qz);
    md_segment(px, py, pz, t.ax, t.ay, t.az, t.cx, t.cy, t.cz, ex, ey, ez);
    double d = md_dist2(px, py, pz, ex, ey, ez);
    if (d < best) { best = d; qx = ex; qy = ey; qz = ez; }
    md_segment(px, py, pz, t.bx, t.by, t.bz, t.cx, t.cy, t.cz, ex, ey, ez);
    d = md_dist2(px, py, pz, ex, ey, ez);
    if (d < best) { qx = ex; qy = ey; qz = ez; }
}

// One thread per query point, points taken in the caller's order (sorted by home cell, so that the lanes of a wave walk
// neighbouring cells and end after a similar number of shells).
//
// The search: the oversize list first, then the cell lists of the shells of Chebyshev radius r = 0, 1, 2, ... around the home
// cell H (the cell of p, clamped into the grid), each shell clipped to the grid.  After shell r every triangle whose cell range
// meets the block B_r = [H - r, H + r]^3 has been tested (a triangle is listed in every cell of its range).
//
// The stop rule, and why it is exact.  A triangle T not yet tested has a cell range that misses B_r, so on some axis a its whole
// range lies above B_r's last cell k1 (possible only if k1 < n_a - 1) or below B_r's first cell k0 (only if k0 > 0).  Say above:
// every point x of T has cell(x_a) >= k1 + 1, hence x_a >= lo_a + (k1 + 1) cell up to the rounding of md_cell, i.e.
// x_a - p_a >= D := lo_a + (k1 + 1) cell - p_a - slack.  T also lies inside the mesh's bounding box [lo, hi] (the exact minimum and
// maximum of the vertices), so on every axis b: |x_b - p_b| >= E_b := max(lo_b - p_b, p_b - hi_b, 0) - slack.  Therefore
//     dist(p, T)^2 >= max(D, E_a, 0)^2 + sum_{b != a} max(E_b, 0)^2,
// and the minimum of that over the (at most six) open sides of B_r bounds every untested triangle from below, wherever p lies:
// inside the grid, outside the bounding box (then H is the clamped cell and the E terms carry the distance to the box, so a far
// point stops after the shells that cover the near face of the box rather than after the whole grid), or far away.  slack =
// 1e-12 x (largest coordinate magnitude involved) is some thousand times the rounding of md_cell, of the plane positions and of
// the computed distances, and makes the bound conservative: it can only cost an extra shell, never a triangle.  The search stops
// when best^2 < bound^2 -- strictly, so that an untested triangle can not even tie (ties go to the lowest id) -- or when B_r
// covers the grid.  The result is therefore the lexicographic minimum of (d^2, id) over all triangles, what a brute-force
// pass in index order returns, and it is bitwise reproducible.
__global__ __launch_bounds__(256) void closest_point_kernel(PsnTriGrid g, const double* __restrict__ vertices, const int64_t* __restrict__ faces,
                                                            const int* __restrict__ cell_start, const int* __restrict__ list,
                                                            const int* __restrict__ over_list, int64_t n_over, const double* __restrict__ points,
                                                            const int64_t* __restrict__ order, int64_t n_points, double* __restrict__ closest,
                                                            double* __restrict__ dist, int64_t* __restrict__ tri,
                                                            unsigned long long* __restrict__ n_tests) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    unsigned int tests = 0;
    if (i < n_points) {
        const int64_t q = order != nullptr ? order[i] : i;
        const double p[3] = {points[3 * q], points[3 * q + 1], points[3 * q + 2]};
        double best = __builtin_inf();
        int best_id = 0x7fffffff;
        auto test = [&](int id) {
            double qx, qy, qz;
            md_closest(p[0], p[1], p[2], md_load(vertices, faces, id), qx, qy, qz);
            const double d = md_dist2(p[0], p[1], p[2], qx, qy, qz);
            if (d < best || (d == best && id < best_id)) { best = d; best_id = id; }
            ++tests;
        };
        for (int64_t k = 0; k < n_over; ++k) test(over_list[k]);
        const double inv = 1.0 / g.cell;
        int H[3];
        double E[3], scale = 0.0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            H[a] = md_cell(p[a], g.lo[a], inv, g.n[a]);
            scale = fmax(scale, fmax(fabs(p[a]), fmax(fabs(g.lo[a]), fabs(g.lo[a] + (double)g.n[a] * g.cell))));
        }
        const double slack = 1e-12 * scale;
#pragma unroll
        for (int a = 0; a < 3; ++a) E[a] = fmax(fmax(g.lo[a] - p[a], p[a] - g.hi[a]) - slack, 0.0);
        const int r_max = max(max(max(H[0], g.n[0] - 1 - H[0]), max(H[1], g.n[1] - 1 - H[1])), max(H[2], g.n[2] - 1 - H[2]));
        for (int r = 0; r <= r_max; ++r) {
            const int x0 = max(H[0] - r, 0), x1 = min(H[0] + r, g.n[0] - 1);
            const int y0 = max(H[1] - r, 0), y1 = min(H[1] + r, g.n[1] - 1);
            const int z0 = max(H[2] - r, 0), z1 = min(H[2] + r, g.n[2] - 1);
            for (int x = x0; x <= x1; ++x) {
                const bool fx = x == H[0] - r || x == H[0] + r;
                for (int y = y0; y <= y1; ++y) {
                    const bool fxy = fx || y == H[1] - r || y == H[1] + r;
                    const int64_t row = ((int64_t)x * g.n[1] + y) * g.n[2];
                    // on a face of the shell along x or y: the whole z run (consecutive cells = one run of the list); else its two ends
                    if (fxy) {
                        const int e = cell_start[row + z1 + 1];
                        for (int k = cell_start[row + z0]; k < e; ++k) test(list[k]);
                    } else {
                        if (H[2] - r >= 0) {
                            const int e = cell_start[row + z0 + 1];
                            for (int k = cell_start[row + z0]; k < e; ++k) test(list[k]);
                        }
                        if (H[2] + r <= g.n[2] - 1) {
                            const int e = cell_start[row + z1 + 1];
                            for (int k = cell_start[row + z1]; k < e; ++k) test(list[k]);
                        }
                    }
                }
            }
            // the bound over the open sides of the block (see above)
            const int k0[3] = {x0, y0, z0}, k1[3] = {x1, y1, z1};
            double bound2 = __builtin_inf();
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const double others = E[(a + 1) % 3] * E[(a + 1) % 3] + E[(a + 2) % 3] * E[(a + 2) % 3];
                if (k1[a] < g.n[a] - 1) {
                    const double D = fmax(fmax(g.lo[a] + (double)(k1[a] + 1) * g.cell - p[a] - slack, E[a]), 0.0);
                    bound2 = fmin(bound2, D * D + others);
                }
                if (k0[a] > 0) {
                    const double D = fmax(fmax(p[a] - (g.lo[a] + (double)k0[a] * g.cell) - slack, E[a]), 0.0);
                    bound2 = fmin(bound2, D * D + others);
                }
            }
            if (best < bound2 * (1.0 - 1e-12)) break;   // (the factor: the roundings of the squares and of their sum)
        }
        if (best_id != 0x7fffffff) {
            double qx, qy, qz;
            md_closest(p[0], p[1], p[2], md_load(vertices, faces, best_id), qx, qy, qz);
            closest[3 * q] = qx; closest[3 * q + 1] = qy; closest[3 * q + 2] = qz;
            dist[q] = sqrt(md_dist2(p[0], p[1], p[2], qx, qy, qz));
            tri[q] = best_id;
        } else {   // a point with a NaN coordinate is at no distance from anything
            closest[3 * q] = closest[3 * q + 1] = closest[3 * q + 2] = dist[q] = __builtin_nan("");
            tri[q] = -1;
        }
    }
    md_add_tests(n_tests, tests);   // one atomic per wave (every lane reaches this point)
}

}  // namespace psn

// Index build, first pass.  cell_count [n0 n1 n2] (x-major) is zeroed here, then receives per cell the number of triangles whose
// bounding box overlaps it; triangles that overlap more than grid->max_span cells are appended to over_list [n_faces] instead
// (order not defined) and counted in n_over[0] (set here).  Vertex indices are the caller's responsibility (0 <= index < V).
extern "C" int psn_tri_grid_count(const PsnTriGrid* grid, const double* vertices, const int64_t* faces, int64_t n_faces, int* cell_count,
                                  int* over_list, long long* n_over, void* stream) {
    using namespace psn;
    if (int rc = md_check_grid(grid, "tri_grid_count")) return rc;
    PSN_CHECK_ARG(vertices && faces && cell_count && over_list && n_over, "tri_grid_count: null pointer");
    PSN_CHECK_ARG(n_faces >= 1 && n_faces <= PSN_TRI_GRID_MAX_FACES, "tri_grid_count: n_faces=%lld (1 .. %lld)", (long long)n_faces,
                  (long long)PSN_TRI_GRID_MAX_FACES);
    const int64_t cells = (int64_t)grid->n[0] * grid->n[1] * grid->n[2];
    if (hipMemsetAsync(cell_count, 0, sizeof(int) * cells, (hipStream_t)stream) != hipSuccess ||
        hipMemsetAsync(n_over, 0, sizeof(long long), (hipStream_t)stream) != hipSuccess) {
        set_error("tri_grid_count: hipMemsetAsync failed");
        return PSN_E_LAUNCH;
    }
    hipLaunchKernelGGL(tri_grid_count_kernel, dim3(md_blocks(n_faces)), dim3(256), 0, (hipStream_t)stream, *grid, vertices, faces, n_faces, cell_count,
                       over_list, reinterpret_cast<unsigned long long*>(n_over));
    PSN_CHECK_LAUNCH("tri_grid_count");
    return PSN_OK;
}

// Index build, second pass.  cursor [cells]: the exclusive scan of psn_tri_grid_count's counts (advanced here: afterwards it is
// the inclusive scan); list [n_entries], n_entries = the total of the counts, receives the triangle ids cell by cell, within a
// cell in no defined order.
extern "C" int psn_tri_grid_fill(const PsnTriGrid* grid, const double* vertices, const int64_t* faces, int64_t n_faces, int* cursor,
                                 int64_t n_entries, int* list, void* stream) {
    using namespace psn;
    if (int rc = md_check_grid(grid, "tri_grid_fill")) return rc;
    PSN_CHECK_ARG(vertices && faces && cursor && (list || n_entries == 0), "tri_grid_fill: null pointer");
    PSN_CHECK_ARG(n_faces >= 1 && n_faces <= PSN_TRI_GRID_MAX_FACES, "tri_grid_fill: n_faces=%lld (1 .. %lld)", (long long)n_faces,
                  (long long)PSN_TRI_GRID_MAX_FACES);
    PSN_CHECK_ARG(n_entries >= 0 && n_entries < ((int64_t)1 << 31), "tri_grid_fill: n_entries=%lld does not fit 32-bit list positions",
                  (long long)n_entries);
    if (n_entries == 0) return PSN_OK;   // every triangle is oversize
    hipLaunchKernelGGL(tri_grid_fill_kernel, dim3(md_blocks(n_faces)), dim3(256), 0, (hipStream_t)stream, *grid, vertices, faces, n_faces, cursor,
                       n_entries, list);
    PSN_CHECK_LAUNCH("tri_grid_fill");
    return PSN_OK;
}

// The query.  index: the grid and lists built above (PsnMeshIndex, include/psnerf_hip.h).  points [n_points, 3]; order: null, or a
// permutation of 0 .. n_points - 1 in which the points are taken (sorted by home cell: neighbouring lanes then walk neighbouring
// cells); outputs are written at the point's own row whatever the order.  closest [n_points, 3], dist [n_points], tri [n_points] (a
// point with a NaN coordinate: NaN, NaN, -1).  n_tests: null, or one counter to which the number of point-triangle tests is ADDED.
extern "C" int psn_closest_point(const PsnMeshIndex* index, const double* points, const int64_t* order, int64_t n_points, double* closest,
                                 double* dist, int64_t* tri, long long* n_tests, void* stream) {
    using namespace psn;
    if (int rc = md_check_index(index, "closest_point")) return rc;
    PSN_CHECK_ARG(n_points >= 0, "closest_point: n_points=%lld", (long long)n_points);
    if (n_points == 0) return PSN_OK;
    PSN_CHECK_ARG(points && closest && dist && tri, "closest_point: null point / output pointer");
    // (the index expanded: with the struct by value this kernel's unchanged search loop measured 1.5 % slower at 1 M points)
    hipLaunchKernelGGL(closest_point_kernel, dim3(md_blocks(n_points)), dim3(256), 0, (hipStream_t)stream, index->grid, index->vertices,
                       index->faces, index->cell_start, index->list, index->over_list, index->n_over, points, order, n_points, closest, dist, tri,
                       reinterpret_cast<unsigned long long*>(n_tests));
    PSN_CHECK_LAUNCH("closest_point");
    return PSN_OK;
}
