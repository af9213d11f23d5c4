// Occlusion of surface rows by the mesh: ambient occlusion, bent normals and visibility bits, over the uniform grid of triangle lists
// that csrc/meshdist.hip builds (conventions: csrc/trigrid.h).
//   psn_occlusion_rows   per row (point, normal): K rays from a direction table, any-hit against the WHOLE mesh
// The rays are never in memory: a row is 6 doubles, the table K x 3 doubles in LDS, and each ray (o, d) is formed in registers in the
// operation order of the numpy definition psnerf_amd/meshocclude.py:host_occlusion_rows, float64 with -ffp-contract=off, so it is
// the definition's ray bit for bit.  It is then walked by csrc/meshray.h:mr_cast<true>, the very function psn_ray_cast instantiates
// (the argument why that walk loses no triangle: the head of csrc/meshray.hip), so ``blocked`` is what psn_ray_cast in any-hit mode
// reports, which is what the definition reports.  Counts are integers, the bent normal is a sum in index order: every output is
// equal to the definition's, and two runs give the same bits.
//
// Layout.  One thread per row, looping over the directions; lanes are consecutive rows.  In the bake the K rows of a face are
// consecutive, share the face's normal (hence the frame) and lie within one triangle, so the lanes of a wave cast nearly the same
// ray at every k and walk the same cells: the coherence psn_ray_cast gets from sorting its rays comes here from the row order.  The
// table sits in LDS; every lane reads the same entry (a broadcast).  The frame and the origin are computed once per row; a direction
// ends at its first accepted triangle.
#include "meshray.h"

namespace psn {

template <bool WORLD>
__global__ __launch_bounds__(256) void occlusion_rows_kernel(PsnMeshIndex ix, const double* __restrict__ points, const double* __restrict__ normals,
                                                             int64_t n_rows, const double* __restrict__ table, int K, double bias, double t_max,
                                                             int* __restrict__ hits_out, int* __restrict__ visible_out, double* __restrict__ ao_out,
                                                             double* __restrict__ bent_out, int* __restrict__ words_out,
                                                             unsigned long long* __restrict__ n_tests) {
    extern __shared__ double tab[];   // [K, 3]
    for (int e = threadIdx.x; e < 3 * K; e += 256) tab[e] = table[e];
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int n_words = (K + 31) >> 5;
    unsigned int tests = 0;
    if (i < n_rows) {
        const double p0 = points[3 * i], p1 = points[3 * i + 1], p2 = points[3 * i + 2];
        const double n0 = normals[3 * i], n1 = normals[3 * i + 1], n2 = normals[3 * i + 2];
        if (!mr_valid(p0, p1, p2, n0, n1, n2)) {   // (the same rule: every component finite, the normal not zero)
            hits_out[i] = -1;
            visible_out[i] = 0;
            ao_out[i] = __builtin_nan("");
            bent_out[3 * i] = bent_out[3 * i + 1] = bent_out[3 * i + 2] = 0.0;
            if (words_out != nullptr)
                for (int w = 0; w < n_words; ++w) words_out[i * n_words + w] = 0;
        } else {
            double t0 = 0.0, t1 = 0.0, t2 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0;
            if (!WORLD) {   // Duff et al., operation for operation meshocclude.py:frame
                const double s = n2 >= 0.0 ? 1.0 : -1.0;
                const double a = -1.0 / (s + n2);
                const double q = (n0 * n1) * a;
                t0 = 1.0 + (s * (n0 * n0)) * a; t1 = s * q; t2 = (-s) * n0;
                b0 = q; b1 = s + (n1 * n1) * a; b2 = -n1;
            }
            const double o0 = p0 + bias * n0, o1 = p1 + bias * n1, o2 = p2 + bias * n2;
            int hits = 0, visible = 0;
            double m0 = 0.0, m1 = 0.0, m2 = 0.0;
            unsigned int word = 0;
            for (int k = 0; k < K; ++k) {
                const double x = tab[3 * k], y = tab[3 * k + 1], z = tab[3 * k + 2];
                double d0 = x, d1 = y, d2 = z;
                bool cast = true;
                if (WORLD) {
                    cast = (n0 * d0 + n1 * d1) + n2 * d2 > 0.0;
                } else {
                    d0 = (x * t0 + y * b0) + z * n0;
                    d1 = (x * t1 + y * b1) + z * n1;
                    d2 = (x * t2 + y * b2) + z * n2;
                }
                if (cast) {
                    MrBest best;
                    MrRay r;
                    if (mr_valid(o0, o1, o2, d0, d1, d2))
                        mr_cast<true>(ix, o0, o1, o2, d0, d1, d2, 0.0, t_max, r, best, tests);
                    if (best.found) {
                        ++hits;
                    } else {
                        ++visible;
                        m0 += d0; m1 += d1; m2 += d2;
                        word |= 1u << (k & 31);
                    }
                }
                if ((k & 31) == 31 || k == K - 1) {
                    if (words_out != nullptr) words_out[i * n_words + (k >> 5)] = (int)word;
                    word = 0;
                }
            }
            const int n_cast = hits + visible;
            hits_out[i] = hits;
            visible_out[i] = visible;
            ao_out[i] = n_cast > 0 ? 1.0 - (double)hits / (double)n_cast : 1.0;
            const double len = sqrt((m0 * m0 + m1 * m1) + m2 * m2);
            const bool ok = len > 0.0;   // (a zero sum, and one whose length is NaN, stay zero)
            bent_out[3 * i] = ok ? m0 / len : 0.0;
            bent_out[3 * i + 1] = ok ? m1 / len : 0.0;
            bent_out[3 * i + 2] = ok ? m2 / len : 0.0;
        }
    }
    md_add_tests(n_tests, tests);   // one atomic per wave (every lane reaches this point)
}

}  // namespace psn

// The query.  points, normals [n_rows, 3]; table [n_dirs, 3]; outputs per row: hits, visible int32, ao float64, bent float64 [3],
// words int32 [(n_dirs + 31) / 32] or null.  n_tests: null, or one counter to which the number of ray-triangle tests is ADDED.
extern "C" int psn_occlusion_rows(const PsnMeshIndex* index, const double* points, const double* normals, int64_t n_rows, const double* table,
                                  int n_dirs, int mode, double bias, double t_max, int* hits, int* visible, double* ao, double* bent, int* words,
                                  long long* n_tests, void* stream) {
    using namespace psn;
    if (int rc = md_check_index(index, "occlusion_rows")) return rc;
    PSN_CHECK_ARG(n_rows >= 0 && n_rows <= 2147483647LL * 256, "occlusion_rows: n_rows=%lld", (long long)n_rows);
    PSN_CHECK_ARG(n_dirs >= 1 && n_dirs <= PSN_OCC_MAX_DIRS, "occlusion_rows: n_dirs=%d (1 .. %d)", n_dirs, PSN_OCC_MAX_DIRS);
    PSN_CHECK_ARG(mode == PSN_OCC_LOCAL || mode == PSN_OCC_WORLD, "occlusion_rows: mode=%d", mode);
    PSN_CHECK_ARG(bias - bias == 0.0, "occlusion_rows: bias=%g is not finite", bias);
    PSN_CHECK_ARG(t_max >= 0.0, "occlusion_rows: t_max=%g < 0 (or a NaN)", t_max);
    PSN_CHECK_ARG(table != nullptr, "occlusion_rows: null direction table");
    if (n_rows == 0) return PSN_OK;
    PSN_CHECK_ARG(points && normals && hits && visible && ao && bent, "occlusion_rows: null row / output pointer");
    const dim3 blocks(md_blocks(n_rows)), threads(256);
    const size_t lds = (size_t)n_dirs * 3 * sizeof(double);
    hipLaunchKernelGGL(mode == PSN_OCC_WORLD ? occlusion_rows_kernel<true> : occlusion_rows_kernel<false>, blocks, threads, lds, (hipStream_t)stream,
                       *index, points, normals, n_rows, table, n_dirs, bias, t_max, hits, visible, ao, bent, words,
                       reinterpret_cast<unsigned long long*>(n_tests));
    PSN_CHECK_LAUNCH("occlusion_rows");
    return PSN_OK;
}
