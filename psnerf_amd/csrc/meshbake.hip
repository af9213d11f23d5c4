// Baking a per-point field onto a triangle mesh: the texel <-> surface maps of the two-faces-per-cell atlas.  The numpy definition is
// psnerf_amd/meshbake.py (Atlas, host_atlas_points, host_atlas_scatter, host_atlas_sample); everything about the layout is integer
// arithmetic, and every float64 operation here is the definition's, in the definition's order (-ffp-contract=off: each product and sum
// a separate operation; IEEE division and square root), so all four entries equal the definition bit for bit.
//
// The atlas (T, c, F): G = T / c cells per side, n = c - 3, K = (n + 2)(n + 3) / 2 rows per face.  Face f lies in cell q = f / 2, whose
// origin is (X0, Y0) = ((q % G) c, (q / G) c), half h = f % 2.  Local texel (i, j), i, j >= 0, i + j <= n + 1, of half 0 is the texel
// (X0 + i, Y0 + j), of half 1 (X0 + c - 1 - i, Y0 + c - 1 - j); its row is f K + k, k = j (n + 2) - j (j - 1) / 2 + i.  The corners of
// the face are the local texels (0, 0), (n, 0), (0, n); the line i + j = n + 1 is the gutter.  The cell diagonal, the second half of
// a last cell that holds one face, the cells beyond it and the margin beyond G c belong to no face.
//
//   psn_atlas_points   rows [f0 K, f1 K) -> the surface point (v0 + (i / n) e1) + (j / n) e2 (float64, and rounded once to float32: the
//                      networks' input) and the unit normal of the row.
//   psn_atlas_scatter  rows float [(f1 - f0) K, C] -> the texels of the faces f0 .. f1 - 1 of a [T, T, C] texture, float or bytes.
//   psn_atlas_fill     the texels NO face owns := fill (every other texel is left alone): with it, chunks of faces compose.
//   psn_atlas_sample   (face, barycentrics) -> the bilinear lookup at sum b_k (x_k, y_k), float64 [Q, C].
//
// Launch shapes, and why.  All four are pure data movement with a little integer arithmetic: what matters is that the wave's 64
// addresses on the LARGER side of each kernel are consecutive.
//   scatter / fill  one thread per texture ELEMENT (y, x, channel): the texture (c^2 texels per cell) is larger than the rows
//                   ((c - 1) c per cell), so the stores are the side to coalesce -- consecutive lanes store consecutive floats (or
//                   bytes) of one texture row, whatever C is.  The loads then come in runs of up to (c - 1) C consecutive floats (one
//                   j-line of a face), ascending in half 0 and descending in half 1.  grid.y = the texture row within the band of cell
//                   rows the face range touches, grid.x x 256 = the element (x C + channel) within the row: every division is 32-bit
//                   and by a launch constant; only the final addresses are int64.  The diagonal lanes (1 in c) idle.
//   points          one thread per row: 9 doubles + 3 floats out, the face's 3 indices and 9 (+ 9) doubles in, which the K rows of a
//                   face share through the cache.  A wave stores 64 consecutive rows = 1536 consecutive bytes per output array.
//                   k -> (i, j) by walking the j-lines (at most n + 2 steps; n is 1 .. 6 for meshes worth baking).
//   sample          one thread per output element (q, channel): consecutive lanes store consecutive doubles and read C consecutive
//                   floats of four texels; the three barycentrics of a query are read by its C lanes from one cache line.
// 256 threads per workgroup throughout, no LDS, no barrier: nothing here is limited by occupancy.
#include "common.h"
#include <math.h>

namespace psn {

struct MbAtlas {
    int T, c, G, n;
    int64_t K, F;
};

__device__ __forceinline__ int64_t mb_k(int n, int i, int j) { return (int64_t)j * (n + 2) - (int64_t)j * (j - 1) / 2 + i; }

// texel-centre coordinates of local (i, j) of face f
__device__ __forceinline__ void mb_texel(const MbAtlas& A, int64_t f, int i, int j, int& x, int& y) {
    const int64_t q = f >> 1;
    const int X0 = (int)(q % A.G) * A.c, Y0 = (int)(q / A.G) * A.c;
    if ((f & 1) == 0) { x = X0 + i; y = Y0 + j; }
    else { x = X0 + A.c - 1 - i; y = Y0 + A.c - 1 - j; }
}

// (x, y) -> the owning face and its row k, or false (unowned)
__device__ __forceinline__ bool mb_owner(const MbAtlas& A, int x, int y, int64_t& f, int64_t& k) {
    const int cx = x / A.c, cy = y / A.c;
    if (cx >= A.G || cy >= A.G) return false;
    int i = x - cx * A.c, j = y - cy * A.c;
    const int s = i + j;
    if (s == A.c - 1) return false;
    const int64_t q = (int64_t)cy * A.G + cx;
    int h = 0;
    if (s > A.c - 1) { h = 1; i = A.c - 1 - i; j = A.c - 1 - j; }
    f = 2 * q + h;
    if (f >= A.F) return false;
    k = mb_k(A.n, i, j);
    return true;
}

// the to_img rule in float32: clip to [0, 1], x 255, round half to even; NaN -> 0
__device__ __forceinline__ unsigned char mb_to_img(float x) {
    if (!(x == x)) return 0;
    x = x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x);
    return (unsigned char)(int)rintf(x * 255.0f);
}

__device__ __forceinline__ void mb_unit(double m0, double m1, double m2, double* __restrict__ out) {
    const double len = sqrt((m0 * m0 + m1 * m1) + m2 * m2);
    const bool ok = len > 0.0;   // (a zero vector, and one whose length is NaN, stay zero)
    out[0] = ok ? m0 / len : 0.0;
    out[1] = ok ? m1 / len : 0.0;
    out[2] = ok ? m2 / len : 0.0;
}

__global__ __launch_bounds__(256) void atlas_points_kernel(MbAtlas A, const double* __restrict__ vertices, int64_t n_vertices,
                                                           const int64_t* __restrict__ faces, const double* __restrict__ vnormals, int64_t f0,
                                                           int64_t n_rows, double* __restrict__ points, float* __restrict__ points_f32,
                                                           double* __restrict__ normals) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n_rows) return;
    const int64_t df = r / A.K, f = f0 + df;
    int k = (int)(r - df * A.K), j = 0;
    for (int line = A.n + 2; k >= line; --line) { k -= line; ++j; }   // line j holds n + 2 - j texels
    const int i = k;
    const int64_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    const double nan = __builtin_nan("");
    if (a < 0 || a >= n_vertices || b < 0 || b >= n_vertices || c < 0 || c >= n_vertices) {   // (the wrapper refuses such a mesh)
#pragma unroll
        for (int d = 0; d < 3; ++d) { points[3 * r + d] = nan; points_f32[3 * r + d] = (float)nan; normals[3 * r + d] = nan; }
        return;
    }
    const double nd = (double)A.n, u = (double)i / nd, v = (double)j / nd;
    double e1[3], e2[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const double v0 = vertices[3 * a + d];
        e1[d] = vertices[3 * b + d] - v0;
        e2[d] = vertices[3 * c + d] - v0;
        const double p = (v0 + u * e1[d]) + v * e2[d];
        points[3 * r + d] = p;
        points_f32[3 * r + d] = (float)p;
    }
    if (vnormals != nullptr) {
        const double b0 = 1.0 - (double)(i + j) / nd;
        double m[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) m[d] = (b0 * vnormals[3 * a + d] + u * vnormals[3 * b + d]) + v * vnormals[3 * c + d];
        mb_unit(m[0], m[1], m[2], normals + 3 * r);
    } else {
        mb_unit(e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0], normals + 3 * r);
    }
}

// grid.y = texture row - y_first, grid.x x 256 = x C + channel.  FILL: the unowned texels := fill; otherwise the texels of f0 .. f1 - 1.
template <bool FILL, typename TexT>
__global__ __launch_bounds__(256) void atlas_scatter_kernel(MbAtlas A, int C, int y_first, const float* __restrict__ rows, int64_t f0, int64_t f1,
                                                            float fill, TexT* __restrict__ tex) {
    const unsigned e = blockIdx.x * 256u + threadIdx.x;
    if (e >= (unsigned)A.T * (unsigned)C) return;
    const int x = (int)(e / (unsigned)C), ch = (int)(e - (unsigned)x * (unsigned)C), y = y_first + (int)blockIdx.y;
    int64_t f, k;
    const bool owned = mb_owner(A, x, y, f, k);
    float value;
    if (FILL) {
        if (owned) return;
        value = fill;
    } else {
        if (!owned || f < f0 || f >= f1) return;
        value = rows[((f - f0) * A.K + k) * C + ch];
    }
    const int64_t at = ((int64_t)y * A.T + x) * C + ch;
    if (sizeof(TexT) == 1) tex[at] = (TexT)mb_to_img(value);
    else tex[at] = (TexT)value;
}

__global__ __launch_bounds__(256) void atlas_sample_kernel(MbAtlas A, int C, const int64_t* __restrict__ face, const double* __restrict__ bary,
                                                           const float* __restrict__ tex, int64_t n_out, double* __restrict__ out) {
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= n_out) return;
    const int64_t q = o / C;
    const int ch = (int)(o - q * C);
    const int64_t f = face[q];
    const double nan = __builtin_nan("");
    if (f < 0 || f >= A.F) { out[o] = nan; return; }
    int x0, y0, x1, y1, x2, y2;
    mb_texel(A, f, 0, 0, x0, y0);
    mb_texel(A, f, A.n, 0, x1, y1);
    mb_texel(A, f, 0, A.n, x2, y2);
    const double b0 = bary[3 * q], b1 = bary[3 * q + 1], b2 = bary[3 * q + 2];
    const double x = (b0 * (double)x0 + b1 * (double)x1) + b2 * (double)x2;
    const double y = (b0 * (double)y0 + b1 * (double)y1) + b2 * (double)y2;
    if (!(x - x == 0.0 && y - y == 0.0)) { out[o] = nan; return; }   // (not finite: no texel to look at)
    const double top = (double)(A.T - 1);
    const double flx = floor(x), fly = floor(y);
    const double cx = fmin(fmax(flx, 0.0), top), cy = fmin(fmax(fly, 0.0), top);
    const int64_t ix0 = (int64_t)cx, iy0 = (int64_t)cy;
    const int64_t ix1 = ix0 + 1 < A.T ? ix0 + 1 : A.T - 1, iy1 = iy0 + 1 < A.T ? iy0 + 1 : A.T - 1;
    const double fx = x - flx, fy = y - fly;
    const double t00 = (double)tex[(iy0 * A.T + ix0) * C + ch], t10 = (double)tex[(iy0 * A.T + ix1) * C + ch];
    const double t01 = (double)tex[(iy1 * A.T + ix0) * C + ch], t11 = (double)tex[(iy1 * A.T + ix1) * C + ch];
    out[o] = (1.0 - fy) * ((1.0 - fx) * t00 + fx * t10) + fy * ((1.0 - fx) * t01 + fx * t11);
}

// The checks every entry shares; fills A.
static int mb_atlas(const char* what, int T, int c, int64_t F, MbAtlas& A) {
    PSN_CHECK_ARG(T >= 4 && T <= PSN_ATLAS_MAX_SIZE, "%s: T=%d (4 .. %d)", what, T, PSN_ATLAS_MAX_SIZE);
    PSN_CHECK_ARG(c >= 4 && c <= T, "%s: cell=%d (4 .. T=%d)", what, c, T);
    PSN_CHECK_ARG(F >= 1, "%s: n_faces=%lld", what, (long long)F);
    A.T = T; A.c = c; A.G = T / c; A.n = c - 3;
    A.K = (int64_t)(A.n + 2) * (A.n + 3) / 2;
    A.F = F;
    PSN_CHECK_ARG((int64_t)A.G * A.G >= (F + 1) / 2, "%s: %lld faces do not fit %d x %d cells of %d texels", what, (long long)F, A.G, A.G, c);
    return PSN_OK;
}

template <bool FILL>
static int mb_launch_scatter(const char* what, const MbAtlas& A, int C, int type, const float* rows, int64_t f0, int64_t f1, float fill, void* tex,
                             void* stream) {
    // the band of texture rows to visit: everything (fill), or the cell rows of the face range
    const int y_first = FILL ? 0 : (int)((f0 / 2) / A.G) * A.c;
    const int y_end = FILL ? A.T : ((int)(((f1 - 1) / 2) / A.G) + 1) * A.c;
    const dim3 grid((unsigned)(((int64_t)A.T * C + 255) / 256), (unsigned)(y_end - y_first));
    if (type == PSN_IMG_U8)
        hipLaunchKernelGGL((atlas_scatter_kernel<FILL, unsigned char>), grid, dim3(256), 0, (hipStream_t)stream, A, C, y_first, rows, f0, f1, fill,
                           reinterpret_cast<unsigned char*>(tex));
    else
        hipLaunchKernelGGL((atlas_scatter_kernel<FILL, float>), grid, dim3(256), 0, (hipStream_t)stream, A, C, y_first, rows, f0, f1, fill,
                           reinterpret_cast<float*>(tex));
    PSN_CHECK_LAUNCH(what);
    return PSN_OK;
}

static int mb_check_texture(const char* what, int C, int type) {
    PSN_CHECK_ARG(C >= 1 && C <= PSN_ATLAS_MAX_CHANNELS, "%s: %d channels (1 .. %d)", what, C, PSN_ATLAS_MAX_CHANNELS);
    PSN_CHECK_ARG(type == PSN_IMG_F32 || type == PSN_IMG_U8, "%s: texture_type=%d (PSN_IMG_F32, PSN_IMG_U8)", what, type);
    return PSN_OK;
}

}  // namespace psn

extern "C" int psn_atlas_points(const double* vertices, int64_t n_vertices, const int64_t* faces, int64_t n_faces, const double* vertex_normals,
                                int T, int cell, int64_t f0, int64_t f1, double* points, float* points_f32, double* normals, void* stream) {
    using namespace psn;
    MbAtlas A;
    if (int rc = mb_atlas("atlas_points", T, cell, n_faces, A)) return rc;
    PSN_CHECK_ARG(n_vertices >= 1, "atlas_points: n_vertices=%lld", (long long)n_vertices);
    PSN_CHECK_ARG(f0 >= 0 && f0 <= f1 && f1 <= n_faces, "atlas_points: face range [%lld, %lld) of %lld faces", (long long)f0, (long long)f1,
                  (long long)n_faces);
    if (f0 == f1) return PSN_OK;
    PSN_CHECK_ARG(vertices && faces && points && points_f32 && normals, "atlas_points: null pointer");
    const int64_t n_rows = (f1 - f0) * A.K, blocks = (n_rows + 255) / 256;
    PSN_CHECK_ARG(blocks < (1ll << 31), "atlas_points: %lld rows exceed one launch (bake in chunks of faces)", (long long)n_rows);
    hipLaunchKernelGGL(atlas_points_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, A, vertices, n_vertices, faces, vertex_normals,
                       f0, n_rows, points, points_f32, normals);
    PSN_CHECK_LAUNCH("atlas_points");
    return PSN_OK;
}

extern "C" int psn_atlas_scatter(const float* rows, int C, int T, int cell, int64_t n_faces, int64_t f0, int64_t f1, void* texture, int texture_type,
                                 void* stream) {
    using namespace psn;
    MbAtlas A;
    if (int rc = mb_atlas("atlas_scatter", T, cell, n_faces, A)) return rc;
    if (int rc = mb_check_texture("atlas_scatter", C, texture_type)) return rc;
    PSN_CHECK_ARG(f0 >= 0 && f0 <= f1 && f1 <= n_faces, "atlas_scatter: face range [%lld, %lld) of %lld faces", (long long)f0, (long long)f1,
                  (long long)n_faces);
    if (f0 == f1) return PSN_OK;
    PSN_CHECK_ARG(rows && texture, "atlas_scatter: null pointer");
    return mb_launch_scatter<false>("atlas_scatter", A, C, texture_type, rows, f0, f1, 0.0f, texture, stream);
}

extern "C" int psn_atlas_fill(float fill, int C, int T, int cell, int64_t n_faces, void* texture, int texture_type, void* stream) {
    using namespace psn;
    MbAtlas A;
    if (int rc = mb_atlas("atlas_fill", T, cell, n_faces, A)) return rc;
    if (int rc = mb_check_texture("atlas_fill", C, texture_type)) return rc;
    PSN_CHECK_ARG(texture, "atlas_fill: null pointer");
    return mb_launch_scatter<true>("atlas_fill", A, C, texture_type, nullptr, 0, n_faces, fill, texture, stream);
}

extern "C" int psn_atlas_sample(const int64_t* face, const double* bary, int64_t n_queries, const float* texture, int C, int T, int cell,
                                int64_t n_faces, double* out, void* stream) {
    using namespace psn;
    MbAtlas A;
    if (int rc = mb_atlas("atlas_sample", T, cell, n_faces, A)) return rc;
    PSN_CHECK_ARG(C >= 1 && C <= PSN_ATLAS_MAX_CHANNELS, "atlas_sample: %d channels (1 .. %d)", C, PSN_ATLAS_MAX_CHANNELS);
    PSN_CHECK_ARG(n_queries >= 0, "atlas_sample: n_queries=%lld", (long long)n_queries);
    if (n_queries == 0) return PSN_OK;
    PSN_CHECK_ARG(face && bary && texture && out, "atlas_sample: null pointer");
    const int64_t n_out = n_queries * C, blocks = (n_out + 255) / 256;
    PSN_CHECK_ARG(blocks < (1ll << 31), "atlas_sample: %lld outputs exceed one launch", (long long)n_out);
    hipLaunchKernelGGL(atlas_sample_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, A, C, face, bary, texture, n_out, out);
    PSN_CHECK_LAUNCH("atlas_sample");
    return PSN_OK;
}
