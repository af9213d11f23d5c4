// The views projected onto surface rows: which of V cameras see a row (point, normal) of the mesh, and what their images show there,
// over the uniform grid of triangle lists that csrc/meshdist.hip builds (conventions: csrc/trigrid.h).
//   psn_project_rows   per row: V views in ascending order; projection, footprint, facing, mask, then an any-hit walk to the camera
// The definition is psnerf_amd/meshproject.py:host_project_rows; every operation below is the definition's, in its order, float64
// with -ffp-contract=off.  The segment to a camera is never in memory: a row is 6 doubles, a view 16 doubles in LDS, and the ray
// (q, o - q) is formed in registers and walked by csrc/meshray.h:mr_cast<true>, the very function psn_ray_cast instantiates (why that
// walk loses no triangle: the head of csrc/meshray.hip), so ``blocked`` is what psn_ray_cast in any-hit mode reports for it with
// t in [0, 1].  A row's views accumulate in its one thread in ascending order, so the sums are the definition's bits and the same
// in every run; there is no floating-point atomic.
//
// Layout.  One thread per row, looping over the views; lanes are consecutive rows.  The rows of an atlas chunk and of a vertex list
// are neighbours on the surface, so at every view the lanes of a wave aim at the same camera from nearly the same point and walk the
// same cells: the coherence psn_ray_cast gets from sorting comes here from the row order (what csrc/meshocclude.hip found for its
// rows holds for these).  The four cheap tests come first and are one short divergent region; only the survivors walk.  A typical
// row is seen by fewer than half of a ring of cameras (the facing test), so a lane idles while its neighbours walk only where the
// terminator of a view crosses the wave.
// Block of 256 like the other row kernels: the view table is at most 256 x 16 doubles = 32 KiB of LDS, which five blocks share
// a CU's 160 KiB with, more than the walk's registers let run; every lane reads the same entry (a broadcast, no bank conflict).
#include "meshray.h"

namespace psn {

// one pixel as the definition's double: a byte u is u / 255.0, a float is widened exactly
__device__ __forceinline__ double pj_pixel(const void* __restrict__ images, bool u8, int64_t at) {
    return u8 ? (double)static_cast<const unsigned char*>(images)[at] / 255.0 : (double)static_cast<const float*>(images)[at];
}

template <int C>
__global__ __launch_bounds__(256) void project_rows_kernel(PsnMeshIndex ix, const double* __restrict__ points, const double* __restrict__ normals,
                                                           int64_t n_rows, const double* __restrict__ views, int V,
                                                           const void* __restrict__ images, int u8, int H, int W,
                                                           const unsigned char* __restrict__ masks, double bias, double cos_min, int uniform,
                                                           int camera_normal, double* __restrict__ sum_out, double* __restrict__ sum_sq_out,
                                                           double* __restrict__ weight_out, int* __restrict__ n_seen_out,
                                                           int* __restrict__ best_view_out, double* __restrict__ best_value_out,
                                                           int* __restrict__ words_out, unsigned long long* __restrict__ n_tests) {
    extern __shared__ double tab[];   // [V, 16]: R row-major, o, K00, K02, K12, 0 (hull.py:_views)
    for (int e = threadIdx.x; e < 16 * V; e += 256) tab[e] = views[e];
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int n_words = (V + 31) >> 5;
    constexpr int CC = C > 0 ? C : 1;
    unsigned int tests = 0;
    if (i < n_rows) {
        const double p0 = points[3 * i], p1 = points[3 * i + 1], p2 = points[3 * i + 2];
        const double n0 = normals[3 * i], n1 = normals[3 * i + 1], n2 = normals[3 * i + 2];
        double sum[CC], sum_sq[CC], best_value[CC];
#pragma unroll
        for (int c = 0; c < CC; ++c) sum[c] = sum_sq[c] = best_value[c] = 0.0;
        double weight = 0.0, best_w = 0.0;
        int n_seen = 0, best_view = -1;
        const bool row_ok = mr_valid(p0, p1, p2, n0, n1, n2);   // (every component finite, the normal not zero)
        if (!row_ok) {
            if (words_out != nullptr)
                for (int w = 0; w < n_words; ++w) words_out[i * n_words + w] = 0;
        } else {
            const double q0 = p0 + bias * n0, q1 = p1 + bias * n1, q2 = p2 + bias * n2;
            const double right = (double)(W - 1), bottom = (double)(H - 1);
            unsigned int word = 0;
            for (int v = 0; v < V; ++v) {
                const double* t = tab + 16 * v;
                const double o0 = t[9], o1 = t[10], o2 = t[11];
                bool sees = false;
                double c = 0.0, fx = 0.0, fy = 0.0;
                int x0 = 0, x1 = 0, y0 = 0, y1 = 0;
                // 1. projection (hull.py:_project_uv)
                const double d0 = p0 - o0, d1 = p1 - o1, d2 = p2 - o2;
                const double xc0 = (d0 * t[0] + d1 * t[3]) + d2 * t[6];
                const double xc1 = (d0 * t[1] + d1 * t[4]) + d2 * t[7];
                const double xc2 = (d0 * t[2] + d1 * t[5]) + d2 * t[8];
                if (xc2 > 0.0) {
                    const double pu = t[13] + t[12] * (xc0 / xc2);
                    const double pv = t[14] + t[12] * (xc1 / xc2);
                    // 2. footprint (a NaN is outside)
                    if (pu >= 0.0 && pu <= right && pv >= 0.0 && pv <= bottom) {
                        // 3. facing
                        const double e0 = o0 - p0, e1 = o1 - p1, e2 = o2 - p2;
                        c = ((n0 * e0 + n1 * e1) + n2 * e2) / sqrt((e0 * e0 + e1 * e1) + e2 * e2);
                        if (c > cos_min) {
                            const double flx = floor(pu), fly = floor(pv);
                            x0 = (int)flx; y0 = (int)fly;   // (0 .. W - 1 and 0 .. H - 1 by the footprint test)
                            x1 = x0 + 1 < W - 1 ? x0 + 1 : W - 1;
                            y1 = y0 + 1 < H - 1 ? y0 + 1 : H - 1;
                            fx = pu - flx; fy = pv - fly;
                            // 4. mask: all four pixels of the footprint set
                            bool open = true;
                            if (masks != nullptr) {
                                const unsigned char* m = masks + (int64_t)v * H * W;
                                open = m[(int64_t)y0 * W + x0] != 0 && m[(int64_t)y0 * W + x1] != 0 && m[(int64_t)y1 * W + x0] != 0 &&
                                       m[(int64_t)y1 * W + x1] != 0;
                            }
                            // 5. not blocked: the segment from q to the camera, t = 1 at the camera
                            if (open) {
                                const double r0 = o0 - q0, r1 = o1 - q1, r2 = o2 - q2;
                                MrBest best;
                                MrRay r;
                                if (mr_valid(q0, q1, q2, r0, r1, r2)) mr_cast<true>(ix, q0, q1, q2, r0, r1, r2, 0.0, 1.0, r, best, tests);
                                sees = !best.found;
                            }
                        }
                    }
                }
                if (sees) {
                    const double w = uniform ? 1.0 : c;
                    double val[CC];
                    if (C > 0) {
                        const int64_t base = (int64_t)v * H * W;
                        const int64_t a00 = (base + (int64_t)y0 * W + x0) * C, a10 = (base + (int64_t)y0 * W + x1) * C;
                        const int64_t a01 = (base + (int64_t)y1 * W + x0) * C, a11 = (base + (int64_t)y1 * W + x1) * C;
#pragma unroll
                        for (int ch = 0; ch < CC; ++ch) {
                            const double t00 = pj_pixel(images, u8 != 0, a00 + ch), t10 = pj_pixel(images, u8 != 0, a10 + ch);
                            const double t01 = pj_pixel(images, u8 != 0, a01 + ch), t11 = pj_pixel(images, u8 != 0, a11 + ch);
                            val[ch] = (1.0 - fy) * ((1.0 - fx) * t00 + fx * t10) + fy * ((1.0 - fx) * t01 + fx * t11);
                        }
                        if constexpr (C == 3) {
                            if (camera_normal) {   // camera frame -> world, the trainer's rule: y and z flipped, then R
                                const double a = val[0], b = -val[1], g = -val[2];
                                val[0] = (t[0] * a + t[1] * b) + t[2] * g;
                                val[1] = (t[3] * a + t[4] * b) + t[5] * g;
                                val[2] = (t[6] * a + t[7] * b) + t[8] * g;
                            }
                        }
#pragma unroll
                        for (int ch = 0; ch < CC; ++ch) {
                            sum[ch] += w * val[ch];
                            sum_sq[ch] += w * (val[ch] * val[ch]);
                        }
                    }
                    if (n_seen == 0 || w > best_w) {   // (the largest weight; a tie stays with the lower view)
                        best_w = w;
                        best_view = v;
                        if (C > 0) {
#pragma unroll
                            for (int ch = 0; ch < CC; ++ch) best_value[ch] = val[ch];
                        }
                    }
                    weight += w;
                    ++n_seen;
                    word |= 1u << (v & 31);
                }
                if ((v & 31) == 31 || v == V - 1) {
                    if (words_out != nullptr) words_out[i * n_words + (v >> 5)] = (int)word;
                    word = 0;
                }
            }
        }
        weight_out[i] = weight;
        n_seen_out[i] = n_seen;
        best_view_out[i] = best_view;
        if (C > 0) {
#pragma unroll
            for (int ch = 0; ch < CC; ++ch) {
                sum_out[i * C + ch] = sum[ch];
                sum_sq_out[i * C + ch] = sum_sq[ch];
                best_value_out[i * C + ch] = best_value[ch];
            }
        }
    }
    md_add_tests(n_tests, tests);   // one atomic per wave (every lane reaches this point)
}

}  // namespace psn

// The query.  points, normals [n_rows, 3]; views [n_views, 16]; images [n_views, H, W, C] (null with C = 0: visibility only);
// masks uint8 [n_views, H, W] or null; outputs per row: sum, sum_sq, best_value float64 [C] (not touched with C = 0), weight float64,
// n_seen, best_view int32, words int32 [(n_views + 31) / 32] or null.  n_tests: null, or one counter to which the number of
// ray-triangle tests is ADDED.
extern "C" int psn_project_rows(const PsnMeshIndex* index, const double* points, const double* normals, int64_t n_rows, const double* views,
                                int n_views, const void* images, int image_type, int H, int W, int C, const unsigned char* masks, double bias,
                                double cos_min, int weight_mode, int frame_mode, double* sum, double* sum_sq, double* weight, int* n_seen,
                                int* best_view, double* best_value, int* words, long long* n_tests, void* stream) {
    using namespace psn;
    if (int rc = md_check_index(index, "project_rows")) return rc;
    PSN_CHECK_ARG(n_rows >= 0 && n_rows <= 2147483647LL * 256, "project_rows: n_rows=%lld", (long long)n_rows);
    PSN_CHECK_ARG(n_views >= 1 && n_views <= PSN_PROJECT_MAX_VIEWS, "project_rows: n_views=%d (1 .. %d)", n_views, PSN_PROJECT_MAX_VIEWS);
    PSN_CHECK_ARG(H >= 1 && H <= PSN_PROJECT_MAX_EXTENT && W >= 1 && W <= PSN_PROJECT_MAX_EXTENT, "project_rows: images of %d x %d (1 .. %d)", H, W,
                  PSN_PROJECT_MAX_EXTENT);
    PSN_CHECK_ARG(C >= 0 && C <= PSN_PROJECT_MAX_CHANNELS && (C == 0) == (images == nullptr),
                  "project_rows: C=%d (1 .. %d with images, 0 with a null image pointer)", C, PSN_PROJECT_MAX_CHANNELS);
    PSN_CHECK_ARG(C == 0 || image_type == PSN_IMG_F32 || image_type == PSN_IMG_U8, "project_rows: image_type=%d", image_type);
    PSN_CHECK_ARG(weight_mode == PSN_PROJECT_WEIGHT_COSINE || weight_mode == PSN_PROJECT_WEIGHT_UNIFORM, "project_rows: weight_mode=%d", weight_mode);
    PSN_CHECK_ARG(frame_mode == PSN_PROJECT_FRAME_RAW || frame_mode == PSN_PROJECT_FRAME_CAMERA_NORMAL, "project_rows: frame_mode=%d", frame_mode);
    PSN_CHECK_ARG(frame_mode == PSN_PROJECT_FRAME_RAW || C == 3, "project_rows: frame_mode camera_normal needs C = 3, got %d", C);
    PSN_CHECK_ARG(bias - bias == 0.0, "project_rows: bias=%g is not finite", bias);
    PSN_CHECK_ARG(cos_min - cos_min == 0.0, "project_rows: cos_min=%g is not finite", cos_min);
    PSN_CHECK_ARG(views != nullptr, "project_rows: null view table");
    if (n_rows == 0) return PSN_OK;
    PSN_CHECK_ARG(points && normals && weight && n_seen && best_view, "project_rows: null row / output pointer");
    PSN_CHECK_ARG(C == 0 || (sum && sum_sq && best_value), "project_rows: null sum / sum_sq / best_value with C=%d", C);
    const dim3 blocks(md_blocks(n_rows)), threads(256);
    const size_t lds = (size_t)n_views * 16 * sizeof(double);
    auto kernel = C == 0 ? project_rows_kernel<0> : C == 1 ? project_rows_kernel<1> : C == 2 ? project_rows_kernel<2>
                : C == 3 ? project_rows_kernel<3> : project_rows_kernel<4>;
    hipLaunchKernelGGL(kernel, blocks, threads, lds, (hipStream_t)stream, *index, points, normals, n_rows, views, n_views, images,
                       image_type == PSN_IMG_U8 ? 1 : 0, H, W, masks, bias, cos_min, weight_mode == PSN_PROJECT_WEIGHT_UNIFORM ? 1 : 0,
                       frame_mode == PSN_PROJECT_FRAME_CAMERA_NORMAL ? 1 : 0, sum, sum_sq, weight, n_seen, best_view, best_value, words,
                       reinterpret_cast<unsigned long long*>(n_tests));
    PSN_CHECK_LAUNCH("project_rows");
    return PSN_OK;
}
