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
// The traversal (csrc/meshray.h:mr_cast, which psn_ray_cast and csrc/meshocclude.hip's psn_occlusion_rows both instantiate), and why
// it is conservative.  The result is defined without the grid, so the grid may only ever save tests.
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
#include "meshray.h"

namespace psn {

// One thread per ray, rays taken in the caller's order (sorted by the cell where they enter the box, or pixels in small tiles, so
// that the lanes of a wave walk neighbouring cells).  The walk and its argument: the head of this file.
template <bool ANY>
__global__ __launch_bounds__(256) void ray_cast_kernel(PsnMeshIndex ix, const double* __restrict__ origins, const double* __restrict__ directions,
                                                       const int64_t* __restrict__ order, int64_t n_rays, double t_min, double t_max,
                                                       double* __restrict__ t_out, int64_t* __restrict__ tri_out, double* __restrict__ bary_out,
                                                       unsigned char* __restrict__ hit_out, unsigned long long* __restrict__ n_tests) {
    const double* __restrict__ vertices = ix.vertices; const int64_t* __restrict__ faces = ix.faces;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    unsigned int tests = 0;
    if (i < n_rays) {
        const int64_t q = order != nullptr ? order[i] : i;
        const double o0 = origins[3 * q], o1 = origins[3 * q + 1], o2 = origins[3 * q + 2];
        const double d0 = directions[3 * q], d1 = directions[3 * q + 1], d2 = directions[3 * q + 2];
        MrBest best;
        MrRay r;
        if (mr_valid(o0, o1, o2, d0, d1, d2))
            mr_cast<ANY>(ix, o0, o1, o2, d0, d1, d2, t_min, t_max, r, best, tests);
        const double nan = __builtin_nan("");
        if (!ANY && best.id != 0x7fffffff) {
            double t, U, V, W, det;
            mr_test(r, vertices, faces, best.id, t_min, t_max, t, U, V, W, det);
            t_out[q] = t;
            tri_out[q] = best.id;
            if (bary_out != nullptr) { bary_out[3 * q] = U / det; bary_out[3 * q + 1] = V / det; bary_out[3 * q + 2] = W / det; }
        } else {
            t_out[q] = __builtin_inf();
            tri_out[q] = -1;
            if (bary_out != nullptr) bary_out[3 * q] = bary_out[3 * q + 1] = bary_out[3 * q + 2] = nan;
        }
        hit_out[q] = best.found ? 1 : 0;
    }
    md_add_tests(n_tests, tests);   // one atomic per wave (every lane reaches this point)
}

}  // namespace psn

// The query.  origins, directions [n_rays, 3]; order: null, or a permutation of 0 .. n_rays - 1 in which the rays are taken; outputs
// are written at the ray's own row whatever the order.  mode PSN_RAY_FIRST_HIT: t [n_rays] (inf on a miss), tri [n_rays] (-1), bary
// [n_rays, 3] or null (NaN), hit [n_rays] bytes.  mode PSN_RAY_ANY_HIT: hit only; t, tri and bary receive the values of a miss.
// n_tests: null, or one counter to which the number of ray-triangle tests is ADDED.
extern "C" int psn_ray_cast(const PsnMeshIndex* index, const double* origins, const double* directions, const int64_t* order, int64_t n_rays,
                            double t_min, double t_max, int mode, double* t, int64_t* tri, double* bary, unsigned char* hit, long long* n_tests,
                            void* stream) {
    using namespace psn;
    if (int rc = md_check_index(index, "ray_cast")) return rc;
    PSN_CHECK_ARG(n_rays >= 0, "ray_cast: n_rays=%lld", (long long)n_rays);
    PSN_CHECK_ARG(mode == PSN_RAY_FIRST_HIT || mode == PSN_RAY_ANY_HIT, "ray_cast: mode=%d", mode);
    PSN_CHECK_ARG(t_min <= t_max, "ray_cast: t_min=%g > t_max=%g (or a NaN)", t_min, t_max);
    if (n_rays == 0) return PSN_OK;
    PSN_CHECK_ARG(origins && directions && t && tri && hit, "ray_cast: null ray / output pointer");
    const dim3 blocks(md_blocks(n_rays)), threads(256);
    hipLaunchKernelGGL(mode == PSN_RAY_ANY_HIT ? ray_cast_kernel<true> : ray_cast_kernel<false>, blocks, threads, 0, (hipStream_t)stream, *index,
                       origins, directions, order, n_rays, t_min, t_max, t, tri, bary, hit, reinterpret_cast<unsigned long long*>(n_tests));
    PSN_CHECK_LAUNCH("ray_cast");
    return PSN_OK;
}
