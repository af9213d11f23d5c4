// Ray casting against a triangle mesh on the device, over the uniform grid of triangle lists that csrc/meshdist.hip builds
// (psn_tri_grid_count / psn_tri_grid_fill; the grid's conventions are in csrc/trigrid.h).
//   psn_ray_cast   per ray: the first hit (t, triangle id, barycentrics) over the WHOLE mesh, or whether anything is hit at all
// Geometry is float64 throughout and -ffp-contract=off, so the intersection test below rounds exactly as the numpy definition
// psnerf_amd/meshdist.py:host_ray_cast does.  A thread per ray; the counter is an integer atomic aggregated per wave.
//
// The test is the watertight one of Woop, Benthin and Wald (JCGT 2013): kz = the axis of the largest |d| (the first on a tie),
// kx, ky the next two cyclically, swapped when d[kz] < 0; the corners are translated by -o and sheared by Sx = d[kx] / d[kz],
// Sy = d[ky] / d[kz] onto the plane perpendicular to kz; the ray hits when the three edge functions U, V, W of the sheared corners
// are all >= 0 or all <= 0 and det = U + V + W != 0; t = (U Az + V Bz + W Cz) / det with Az = A[kz] / d[kz], and the hit counts
// when t_min <= t <= t_max.  Two triangles that share an edge see the same two sheared end points, so a ray cannot slip between
// them.  The result is the minimum of (t, triangle id) in lexicographic order over all accepted triangles.  A ray with a
// non-finite component or a zero direction hits nothing; a triangle with det == 0 (zero area, or seen edge-on) is never hit.
//
// The traversal, and why it is conservative.  The result is defined without the grid, so the grid may only ever save tests.
//   What an accepted triangle T guarantees.  U, V, W are the signed areas the ray's axis spans with T's edges in the sheared
//   plane; all of one sign means that plane's origin lies in the sheared triangle up to the rounding of the translation, the
//   shear and the products: there is a point x of the exact triangle whose offset from the ray at x's own kz-coordinate, i.e. at
//   t_x = (x[kz] - o[kz]) / d[kz], is at most eps on every axis, with eps a few ulps of the largest coordinate involved
//   (|o| and the vertices): some 1e-15 x scale.  And t is a convex combination of Az, Bz, Cz, so t lies where T lies along kz.
//   x lies in T's bounding box, md_cell is monotone, hence T is listed in the cell of x (or is in the oversize list, which
//   every ray tests first).  It is therefore enough to visit, for every point of the ray within [t_min, t_max], every cell that
//   holds a point within eps of it.
//   The margin.  m = 1e-9 x cell + 1e-12 x scale (scale = the largest |coordinate| of the origin and of the grid's box): tiny
//   against a cell, and some thousand times eps and every rounding below (each is a few ulps of scale).
//   The walk.  The ray is cut into slabs along its major axis kz, where it advances fastest: slab s is the layer of cells with
//   index s on that axis, widened to [lo + s cell - m, lo + (s + 1) cell + m] (the first and last slab reach to the box's faces
//   -+ m, as md_cell clamps).  Within the slab's parameter interval [ta, tb], cut to [t_min - m / |d[kz]|, t_max + m / |d[kz]|],
//   the ray's other two coordinates run between their values at ta and tb; that interval, widened by m, is mapped through md_cell
//   (monotone, clamping) and the rectangle of cells is visited -- at most 2 x 2 cells unless the margin straddles a boundary,
//   since the ray moves at most one cell edge sideways per slab.  A slab whose rectangle lies outside the box -+ m is skipped, so
//   a ray that misses the box tests the oversize list only.  No comparison decides which SINGLE neighbour to enter: a ray
//   through a cell corner or along a cell edge or boundary plane visits every cell that touches it.  With x as above: x's slab
//   contains t_x (eps < m), the rectangle there contains x's other two cells (eps < m), so T is tested when its slab is reached.
//   The stop rule.  Slabs are taken in order of increasing t; before slab s the walk stops if best < ta(s), the slab's entry
//   parameter (already lowered by the margin) -- strictly, so that an untested triangle can not even tie, and the lower id wins
//   ties among the tested ones.  An untested triangle T' is listed in a slab at or behind s, so t_x' >= ta(s) + m / |d[kz]|.
//   Its own t' differs from t_x' by the conditioning of t = T / det: about eps / sin^2 of the angle between the ray and T's
//   plane.  Wherever that stays below the margin -- wherever the definition's t is itself determined to 1e-9 of a cell -- t' >=
//   ta(s) > best and T' can not be the answer.  (A triangle seen within some 1e-3 rad of edge-on whose hit also falls within
//   that error of a slab plane is outside this argument: there the definition's own first hit is decided by rounding noise.  The
//   hit flag does not depend on the stop rule.)  In any-hit mode the walk ends at the first accepted hit.
// The same triangle may be tested in several cells; the test is idempotent and the result does not depend on the order of the
// lists, so two runs give the same bits.
#include "trigrid.h"

namespace psn {

struct MrRay {
    double ox, oy, oz;   // o[kx], o[ky], o[kz]
    double Sx, Sy, Sz;
    int kx, ky, kz;
};

__device__ __forceinline__ double mr_sel(double a0, double a1, double a2, int k) { return k == 0 ? a0 : (k == 1 ? a1 : a2); }
__device__ __forceinline__ int mr_seli(int a0, int a1, int a2, int k) { return k == 0 ? a0 : (k == 1 ? a1 : a2); }

// Operation for operation meshdist.py:_ray_triangles.
__device__ __forceinline__ bool mr_test(const MrRay& r, const double* __restrict__ v, const int64_t* __restrict__ f, int64_t id, double t_min,
                                        double t_max, double& t, double& U, double& V, double& W, double& det) {
    const int64_t i = 3 * f[3 * id], j = 3 * f[3 * id + 1], k = 3 * f[3 * id + 2];
    const double Akz = v[i + r.kz] - r.oz, Bkz = v[j + r.kz] - r.oz, Ckz = v[k + r.kz] - r.oz;
    const double Ax = (v[i + r.kx] - r.ox) - r.Sx * Akz, Ay = (v[i + r.ky] - r.oy) - r.Sy * Akz;
    const double Bx = (v[j + r.kx] - r.ox) - r.Sx * Bkz, By = (v[j + r.ky] - r.oy) - r.Sy * Bkz;
    const double Cx = (v[k + r.kx] - r.ox) - r.Sx * Ckz, Cy = (v[k + r.ky] - r.oy) - r.Sy * Ckz;
    U = Cx * By - Cy * Bx;
    V = Ax * Cy - Ay * Cx;
    W = Bx * Ay - By * Ax;
    if (!((U >= 0.0 && V >= 0.0 && W >= 0.0) || (U <= 0.0 && V <= 0.0 && W <= 0.0))) return false;
    det = U + V + W;
    if (!(det != 0.0)) return false;
    const double Az = r.Sz * Akz, Bz = r.Sz * Bkz, Cz = r.Sz * Ckz;
    t = (U * Az + V * Bz + W * Cz) / det;
    return t >= t_min && t <= t_max;
}

// One thread per ray, rays taken in the caller's order (sorted by the cell where they enter the box, or pixels in small tiles, so
// that the lanes of a wave walk neighbouring cells).  The walk and its argument: the head of this file.
template <bool ANY>
__global__ __launch_bounds__(256) void ray_cast_kernel(PsnTriGrid g, const double* __restrict__ vertices, const int64_t* __restrict__ faces,
                                                       const int* __restrict__ cell_start, const int* __restrict__ list,
                                                       const int* __restrict__ over_list, int64_t n_over, const double* __restrict__ origins,
                                                       const double* __restrict__ directions, const int64_t* __restrict__ order, int64_t n_rays,
                                                       double t_min, double t_max, double* __restrict__ t_out, int64_t* __restrict__ tri_out,
                                                       double* __restrict__ bary_out, unsigned char* __restrict__ hit_out,
                                                       unsigned long long* __restrict__ n_tests) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    unsigned int tests = 0;
    if (i < n_rays) {
        const int64_t q = order != nullptr ? order[i] : i;
        const double o0 = origins[3 * q], o1 = origins[3 * q + 1], o2 = origins[3 * q + 2];
        const double d0 = directions[3 * q], d1 = directions[3 * q + 1], d2 = directions[3 * q + 2];
        const bool finite = o0 - o0 == 0.0 && o1 - o1 == 0.0 && o2 - o2 == 0.0 && d0 - d0 == 0.0 && d1 - d1 == 0.0 && d2 - d2 == 0.0;
        const bool valid = finite && (d0 != 0.0 || d1 != 0.0 || d2 != 0.0);
        double best = __builtin_inf();
        int best_id = 0x7fffffff;
        bool found = false;
        MrRay r;
        if (valid) {
            int kz = 0;
            double big = fabs(d0);
            if (fabs(d1) > big) { kz = 1; big = fabs(d1); }
            if (fabs(d2) > big) kz = 2;
            const int ku = kz == 2 ? 0 : kz + 1, kv = ku == 2 ? 0 : ku + 1;   // the next two axes cyclically
            const double dk = mr_sel(d0, d1, d2, kz), du = mr_sel(d0, d1, d2, ku), dv = mr_sel(d0, d1, d2, kv);
            const double ok = mr_sel(o0, o1, o2, kz), ou = mr_sel(o0, o1, o2, ku), ov = mr_sel(o0, o1, o2, kv);
            const bool swap = dk < 0.0;
            r.kz = kz; r.kx = swap ? kv : ku; r.ky = swap ? ku : kv;
            r.ox = swap ? ov : ou; r.oy = swap ? ou : ov; r.oz = ok;
            r.Sx = (swap ? dv : du) / dk; r.Sy = (swap ? du : dv) / dk; r.Sz = 1.0 / dk;
            auto test = [&](int id) {
                double t, U, V, W, det;
                ++tests;
                if (!mr_test(r, vertices, faces, id, t_min, t_max, t, U, V, W, det)) return false;
                if (t < best || (t == best && id < best_id)) { best = t; best_id = id; }
                found = true;
                return true;
            };
            [&]() {   // (a lambda, so that any-hit mode leaves every loop with one return)
                for (int64_t k = 0; k < n_over; ++k)
                    if (test(over_list[k]) && ANY) return;
                const double cell = g.cell, inv = 1.0 / cell;
                double scale = fmax(fabs(o0), fmax(fabs(o1), fabs(o2)));
#pragma unroll
                for (int a = 0; a < 3; ++a) scale = fmax(scale, fmax(fabs(g.lo[a]), fabs(g.lo[a] + (double)g.n[a] * cell)));
                const double m = 1e-9 * cell + 1e-12 * scale;
                const double mt = m / fabs(dk);
                const double tA = t_min - mt, tB = t_max + mt;
                const double lo_k = mr_sel(g.lo[0], g.lo[1], g.lo[2], kz), hi_k = mr_sel(g.hi[0], g.hi[1], g.hi[2], kz);
                const double lo_u = mr_sel(g.lo[0], g.lo[1], g.lo[2], ku), hi_u = mr_sel(g.hi[0], g.hi[1], g.hi[2], ku);
                const double lo_v = mr_sel(g.lo[0], g.lo[1], g.lo[2], kv), hi_v = mr_sel(g.hi[0], g.hi[1], g.hi[2], kv);
                const int n_k = mr_seli(g.n[0], g.n[1], g.n[2], kz), n_u = mr_seli(g.n[0], g.n[1], g.n[2], ku);
                const int n_v = mr_seli(g.n[0], g.n[1], g.n[2], kv);
                const int64_t st0 = (int64_t)g.n[1] * g.n[2], st1 = g.n[2];
                const int64_t st_k = kz == 0 ? st0 : (kz == 1 ? st1 : 1), st_u = ku == 0 ? st0 : (ku == 1 ? st1 : 1);
                const int64_t st_v = kv == 0 ? st0 : (kv == 1 ? st1 : 1);
                // the part of the major axis the ray covers within [tA, tB] (an infinite end gives an infinite coordinate: it clamps)
                const double kA = ok + tA * dk, kB = ok + tB * dk;
                const double k_lo = fmin(kA, kB) - m, k_hi = fmax(kA, kB) + m;
                if (k_hi < lo_k - m || k_lo > hi_k + m) return;
                const int s_lo = md_cell(k_lo, lo_k, inv, n_k), s_hi = md_cell(k_hi, lo_k, inv, n_k);
                const int step = swap ? -1 : 1;
                int s = swap ? s_hi : s_lo;
                for (int left = s_hi - s_lo; left >= 0; --left, s += step) {   // (counted: the walk stays in the grid whatever the input)
                    const double c0 = lo_k + (double)s * cell - m;
                    const double c1 = s == n_k - 1 ? fmax(lo_k + (double)(s + 1) * cell, hi_k) + m : lo_k + (double)(s + 1) * cell + m;
                    double ta = ((swap ? c1 : c0) - ok) * r.Sz, tb = ((swap ? c0 : c1) - ok) * r.Sz;
                    if (best < ta) return;
                    ta = fmax(ta, tA); tb = fmin(tb, tB);
                    if (ta <= tb) {
                        const double ua = ou + ta * du, ub = ou + tb * du, va = ov + ta * dv, vb = ov + tb * dv;
                        const double u0 = fmin(ua, ub) - m, u1 = fmax(ua, ub) + m, v0 = fmin(va, vb) - m, v1 = fmax(va, vb) + m;
                        if (!(u1 < lo_u - m || u0 > hi_u + m || v1 < lo_v - m || v0 > hi_v + m)) {
                            const int iu0 = md_cell(u0, lo_u, inv, n_u), iu1 = md_cell(u1, lo_u, inv, n_u);
                            const int iv0 = md_cell(v0, lo_v, inv, n_v), iv1 = md_cell(v1, lo_v, inv, n_v);
                            for (int iu = iu0; iu <= iu1; ++iu)
                                for (int iv = iv0; iv <= iv1; ++iv) {
                                    const int64_t c = s * st_k + iu * st_u + iv * st_v;
                                    const int e = cell_start[c + 1];
                                    for (int k = cell_start[c]; k < e; ++k)
                                        if (test(list[k]) && ANY) return;
                                }
                        }
                    }
                }
            }();
        }
        const double nan = __builtin_nan("");
        if (!ANY && best_id != 0x7fffffff) {
            double t, U, V, W, det;
            mr_test(r, vertices, faces, best_id, t_min, t_max, t, U, V, W, det);
            t_out[q] = t;
            tri_out[q] = best_id;
            if (bary_out != nullptr) { bary_out[3 * q] = U / det; bary_out[3 * q + 1] = V / det; bary_out[3 * q + 2] = W / det; }
        } else {
            t_out[q] = __builtin_inf();
            tri_out[q] = -1;
            if (bary_out != nullptr) bary_out[3 * q] = bary_out[3 * q + 1] = bary_out[3 * q + 2] = nan;
        }
        hit_out[q] = found ? 1 : 0;
    }
    if (n_tests != nullptr) {   // one atomic per wave (every lane reaches this point)
        unsigned long long s = tests;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
        if (md_lane() == 0 && s > 0) atomicAdd(n_tests, s);
    }
}

}  // namespace psn

// The query.  grid / cell_start / list / over_list / n_over: the index as psn_closest_point takes it.  origins, directions
// [n_rays, 3]; order: null, or a permutation of 0 .. n_rays - 1 in which the rays are taken; outputs are written at the ray's own
// row whatever the order.  mode PSN_RAY_FIRST_HIT: t [n_rays] (inf on a miss), tri [n_rays] (-1), bary [n_rays, 3] or null (NaN),
// hit [n_rays] bytes.  mode PSN_RAY_ANY_HIT: hit only; t, tri and bary receive the values of a miss.  n_tests: null, or one counter
// to which the number of ray-triangle tests is ADDED.
extern "C" int psn_ray_cast(const PsnTriGrid* grid, const double* vertices, const int64_t* faces, int64_t n_faces, const int* cell_start,
                            const int* list, const int* over_list, int64_t n_over, const double* origins, const double* directions,
                            const int64_t* order, int64_t n_rays, double t_min, double t_max, int mode, double* t, int64_t* tri, double* bary,
                            unsigned char* hit, long long* n_tests, void* stream) {
    using namespace psn;
    if (int rc = md_check_grid(grid, "ray_cast")) return rc;
    PSN_CHECK_ARG(vertices && faces && cell_start, "ray_cast: null pointer");
    PSN_CHECK_ARG(n_faces >= 1 && n_faces <= PSN_TRI_GRID_MAX_FACES, "ray_cast: n_faces=%lld (1 .. %lld)", (long long)n_faces,
                  (long long)PSN_TRI_GRID_MAX_FACES);
    PSN_CHECK_ARG(n_over >= 0 && n_over <= n_faces && (n_over == 0 || over_list), "ray_cast: n_over=%lld / null oversize list", (long long)n_over);
    PSN_CHECK_ARG(n_over == n_faces || list, "ray_cast: null cell list");
    PSN_CHECK_ARG(n_rays >= 0, "ray_cast: n_rays=%lld", (long long)n_rays);
    PSN_CHECK_ARG(mode == PSN_RAY_FIRST_HIT || mode == PSN_RAY_ANY_HIT, "ray_cast: mode=%d", mode);
    PSN_CHECK_ARG(t_min <= t_max, "ray_cast: t_min=%g > t_max=%g (or a NaN)", t_min, t_max);
    if (n_rays == 0) return PSN_OK;
    PSN_CHECK_ARG(origins && directions && t && tri && hit, "ray_cast: null ray / output pointer");
    const dim3 blocks(md_blocks(n_rays)), threads(256);
    if (mode == PSN_RAY_ANY_HIT)
        hipLaunchKernelGGL(ray_cast_kernel<true>, blocks, threads, 0, (hipStream_t)stream, *grid, vertices, faces, cell_start, list, over_list, n_over,
                           origins, directions, order, n_rays, t_min, t_max, t, tri, bary, hit, reinterpret_cast<unsigned long long*>(n_tests));
    else
        hipLaunchKernelGGL(ray_cast_kernel<false>, blocks, threads, 0, (hipStream_t)stream, *grid, vertices, faces, cell_start, list, over_list, n_over,
                           origins, directions, order, n_rays, t_min, t_max, t, tri, bary, hit, reinterpret_cast<unsigned long long*>(n_tests));
    PSN_CHECK_LAUNCH("ray_cast");
    return PSN_OK;
}
