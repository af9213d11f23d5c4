// Mesh registration on the device: the similarity transform of a point array (psn_align_transform), the row distances the trim's
// quantile is taken of (psn_align_dist) and the normal-equation sums of one trimmed point-to-plane ICP iteration (psn_align_sums).
// The float64 numpy definition is psnerf_amd/meshalign.py:host_*; its module docstring states every step and every operation order,
// and the arithmetic here is float64 in exactly that order (-ffp-contract=off: every product and sum a separate operation; IEEE
// division and square root), so transformed points, distances and the four counts equal the definition bit for bit, and every term of
// the sums does; only the ORDER in which the rows' terms are added differs from numpy's.
//
// psn_align_sums carries no floating-point atomics: workgroup ``chunk`` adds its 1024 rows (four per thread, in ascending row order)
// by wave shuffles and a fixed 4-wave sum and writes ONE partial row of 37 doubles and four int64 counts (every row on every call);
// align_reduce_kernel adds the partial rows in a fixed order.  Two calls on the same input give the same bits.  The scheme is
// ps_intensity_kernel / ps_intensity_reduce_kernel's (csrc/photostereo.hip).
// Every index read from memory is checked before it is used: a triangle id outside 0 .. F - 1, or a face with a vertex index outside
// 0 .. V - 1, makes the row a "no triangle" row.
#include "common.h"
#include <math.h>

namespace psn {

constexpr int AL_CHUNK = PSN_ALIGN_CHUNK;   // rows per workgroup of align_sums_kernel (4 per thread)
constexpr int AL_S = PSN_ALIGN_SUMS;        // 37 doubles: 28 + 7 + 1 + 1
constexpr int AL_C = PSN_ALIGN_COUNTS;      // used, no triangle / not finite, zero normal, beyond max_dist
constexpr int AL_W = AL_S + AL_C;           // 8-byte words of one partial row
static_assert(AL_CHUNK == 1024 && AL_S == 37 && AL_C == 4, "the kernels below are written for these sizes");

struct AlignTransform {
    double s, R[9], t[3];
};

// T(x) = s (R x) + t; row i of R x is (R[i,0] x0 + R[i,1] x1) + R[i,2] x2
__global__ __launch_bounds__(256) void align_transform_kernel(const double* __restrict__ points, int64_t n, AlignTransform T,
                                                              double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double x0 = points[i * 3], x1 = points[i * 3 + 1], x2 = points[i * 3 + 2];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double rx = (T.R[r * 3] * x0 + T.R[r * 3 + 1] * x1) + T.R[r * 3 + 2] * x2;
        out[i * 3 + r] = T.s * rx + T.t[r];
    }
}

// d = sqrt((dx dx + dy dy) + dz dz), (dx, dy, dz) = Y - P
__device__ __forceinline__ double al_dist2(const double* __restrict__ P, const double* __restrict__ Y, int64_t i, double (&e)[3]) {
    e[0] = Y[i * 3] - P[i * 3];
    e[1] = Y[i * 3 + 1] - P[i * 3 + 1];
    e[2] = Y[i * 3 + 2] - P[i * 3 + 2];
    return (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
}

__global__ __launch_bounds__(256) void align_dist_kernel(const double* __restrict__ P, const double* __restrict__ Y, int64_t n,
                                                         double* __restrict__ dist) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double e[3];
    dist[i] = sqrt(al_dist2(P, Y, i, e));
}

struct AlignSums {
    const double* P;           // [n, 3]
    const double* Y;           // [n, 3]
    const int64_t* tri;        // [n]
    const double* vertices;    // [V, 3]
    const int64_t* faces;      // [F, 3]
    int64_t n, n_vertices, n_faces;
    double R[9];               // the rotation applied to the normal (has_R)
    double max_dist;
    int has_R;
};

// One row: its status (0 used, 1 no triangle / not finite, 2 zero normal, 3 beyond max_dist) and, when used, J (7), r and d^2.
__device__ __forceinline__ int al_row(const AlignSums& A, int64_t i, double (&J)[7], double& r, double& d2) {
    const int64_t t = A.tri[i];
    if (t < 0 || t >= A.n_faces) return 1;
    const double p0 = A.P[i * 3], p1 = A.P[i * 3 + 1], p2 = A.P[i * 3 + 2];
    const double y0 = A.Y[i * 3], y1 = A.Y[i * 3 + 1], y2 = A.Y[i * 3 + 2];
    if (!(__builtin_isfinite(p0) && __builtin_isfinite(p1) && __builtin_isfinite(p2) && __builtin_isfinite(y0) && __builtin_isfinite(y1) &&
          __builtin_isfinite(y2)))
        return 1;
    const int64_t ia = A.faces[t * 3], ib = A.faces[t * 3 + 1], ic = A.faces[t * 3 + 2];
    if (ia < 0 || ia >= A.n_vertices || ib < 0 || ib >= A.n_vertices || ic < 0 || ic >= A.n_vertices) return 1;
    const double ax = A.vertices[ia * 3], ay = A.vertices[ia * 3 + 1], az = A.vertices[ia * 3 + 2];
    const double abx = A.vertices[ib * 3] - ax, aby = A.vertices[ib * 3 + 1] - ay, abz = A.vertices[ib * 3 + 2] - az;
    const double acx = A.vertices[ic * 3] - ax, acy = A.vertices[ic * 3 + 1] - ay, acz = A.vertices[ic * 3 + 2] - az;
    const double nx = aby * acz - abz * acy, ny = abz * acx - abx * acz, nz = abx * acy - aby * acx;   // meshcore.face_cross
    const double len = sqrt((nx * nx + ny * ny) + nz * nz);
    if (!(len > 0.0)) return 2;
    double N0 = nx / len, N1 = ny / len, N2 = nz / len;
    if (A.has_R) {
        const double m0 = (A.R[0] * N0 + A.R[1] * N1) + A.R[2] * N2;
        const double m1 = (A.R[3] * N0 + A.R[4] * N1) + A.R[5] * N2;
        const double m2 = (A.R[6] * N0 + A.R[7] * N1) + A.R[8] * N2;
        N0 = m0; N1 = m1; N2 = m2;
    }
    const double dx = y0 - p0, dy = y1 - p1, dz = y2 - p2;
    d2 = (dx * dx + dy * dy) + dz * dz;
    if (!(sqrt(d2) <= A.max_dist)) return 3;
    J[0] = p1 * N2 - p2 * N1;
    J[1] = p2 * N0 - p0 * N2;
    J[2] = p0 * N1 - p1 * N0;
    J[3] = N0; J[4] = N1; J[5] = N2;
    J[6] = (p0 * N0 + p1 * N1) + p2 * N2;
    r = (N0 * dx + N1 * dy) + N2 * dz;
    return 0;
}

__device__ __forceinline__ double al_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;   // (lane 0)
}
__device__ __forceinline__ int al_wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;   // (lane 0)
}

// partial row of chunk blockIdx.x: the 37 sums over its used rows, then the four counts as int64
__global__ __launch_bounds__(256) void align_sums_kernel(AlignSums A, double* __restrict__ partial) {
    __shared__ double s_red[4][AL_S];
    __shared__ int s_cnt[4][AL_C];
    double acc[AL_S];
    int cnt[AL_C] = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < AL_S; ++k) acc[k] = 0.0;
    for (int j = 0; j < AL_CHUNK / 256; ++j) {
        const int64_t i = (int64_t)blockIdx.x * AL_CHUNK + j * 256 + threadIdx.x;
        if (i < A.n) {
            double J[7], r = 0.0, d2 = 0.0;
            const int status = al_row(A, i, J, r, d2);
            cnt[status] += 1;
            if (status == 0) {
                int k = 0;
#pragma unroll
                for (int a = 0; a < 7; ++a) {
#pragma unroll
                    for (int b = a; b < 7; ++b) acc[k++] += J[a] * J[b];
                }
#pragma unroll
                for (int a = 0; a < 7; ++a) acc[28 + a] += J[a] * r;
                acc[35] += r * r;
                acc[36] += d2;
            }
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < AL_S; ++k) {
        const double v = al_wave_sum(acc[k]);
        if (lane == 0) s_red[wave][k] = v;
    }
#pragma unroll
    for (int k = 0; k < AL_C; ++k) {
        const int v = al_wave_sum(cnt[k]);
        if (lane == 0) s_cnt[wave][k] = v;
    }
    __syncthreads();
    double* row = partial + (int64_t)blockIdx.x * AL_W;
    if (threadIdx.x < AL_S)
        row[threadIdx.x] = ((s_red[0][threadIdx.x] + s_red[1][threadIdx.x]) + s_red[2][threadIdx.x]) + s_red[3][threadIdx.x];
    else if (threadIdx.x < AL_W) {
        const int k = threadIdx.x - AL_S;
        reinterpret_cast<long long*>(row)[threadIdx.x] = (long long)((s_cnt[0][k] + s_cnt[1][k]) + (s_cnt[2][k] + s_cnt[3][k]));
    }
}

// The second, fixed-order step over the T partial rows: thread (g, k) adds rows g, g + 4, ... of column k in that order; thread k then
// adds the four group sums in order.  Columns 0 .. 36 are doubles, 37 .. 40 int64 counts.
__global__ __launch_bounds__(256) void align_reduce_kernel(const double* __restrict__ partial, int T, double* __restrict__ sums,
                                                           long long* __restrict__ counts) {
    __shared__ double s_d[4][64];
    __shared__ long long s_i[4][64];
    const int k = threadIdx.x & 63, g = threadIdx.x >> 6;
    double acc = 0.0;
    long long cnt = 0;
    if (k < AL_S) {
        for (int t = g; t < T; t += 4) acc += partial[(int64_t)t * AL_W + k];
    } else if (k < AL_W) {
        for (int t = g; t < T; t += 4) cnt += reinterpret_cast<const long long*>(partial)[(int64_t)t * AL_W + k];
    }
    s_d[g][k] = acc;
    s_i[g][k] = cnt;
    __syncthreads();
    if (threadIdx.x < AL_S)
        sums[threadIdx.x] = ((s_d[0][threadIdx.x] + s_d[1][threadIdx.x]) + s_d[2][threadIdx.x]) + s_d[3][threadIdx.x];
    else if (threadIdx.x < AL_W)
        counts[threadIdx.x - AL_S] = (s_i[0][threadIdx.x] + s_i[1][threadIdx.x]) + (s_i[2][threadIdx.x] + s_i[3][threadIdx.x]);
}

static inline int al_chunks(int64_t n) { return n <= 0 ? 1 : (int)((n + AL_CHUNK - 1) / AL_CHUNK); }

}  // namespace psn

// Number of 8-byte words of psn_align_sums' partial rows for n rows: 41 per 1024-row chunk, at least one chunk.  -1 on a bad argument.
extern "C" int64_t psn_align_workspace(int64_t n) {
    using namespace psn;
    if (n < 0 || n > PSN_ALIGN_MAX_ROWS) return -1;
    return (int64_t)al_chunks(n) * AL_W;
}

extern "C" int psn_align_transform(const double* points, int64_t n, double scale, const double* rotation, const double* translation,
                                   double* out, void* stream) {
    using namespace psn;
    PSN_CHECK_ARG(n >= 0 && n <= PSN_ALIGN_MAX_ROWS, "align_transform: n=%lld (0 .. %lld)", (long long)n, (long long)PSN_ALIGN_MAX_ROWS);
    PSN_CHECK_ARG(points && rotation && translation && out, "align_transform: null pointer");
    if (n == 0) return PSN_OK;
    AlignTransform T;
    T.s = scale;
    for (int i = 0; i < 9; ++i) T.R[i] = rotation[i];
    for (int i = 0; i < 3; ++i) T.t[i] = translation[i];
    hipLaunchKernelGGL(align_transform_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, points, n, T, out);
    PSN_CHECK_LAUNCH("align_transform");
    return PSN_OK;
}

extern "C" int psn_align_dist(const double* P, const double* Y, int64_t n, double* dist, void* stream) {
    using namespace psn;
    PSN_CHECK_ARG(n >= 0 && n <= PSN_ALIGN_MAX_ROWS, "align_dist: n=%lld (0 .. %lld)", (long long)n, (long long)PSN_ALIGN_MAX_ROWS);
    PSN_CHECK_ARG(P && Y && dist, "align_dist: null pointer");
    if (n == 0) return PSN_OK;
    hipLaunchKernelGGL(align_dist_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, P, Y, n, dist);
    PSN_CHECK_LAUNCH("align_dist");
    return PSN_OK;
}

extern "C" int psn_align_sums(const double* P, const double* Y, const int64_t* tri, int64_t n, const double* vertices, int64_t n_vertices,
                              const int64_t* faces, int64_t n_faces, const double* rotation, double max_dist, double* partial, double* sums,
                              int64_t* counts, void* stream) {
    using namespace psn;
    PSN_CHECK_ARG(n >= 0 && n <= PSN_ALIGN_MAX_ROWS, "align_sums: n=%lld (0 .. %lld)", (long long)n, (long long)PSN_ALIGN_MAX_ROWS);
    PSN_CHECK_ARG(P && Y && tri && vertices && faces && partial && sums && counts, "align_sums: null pointer");
    PSN_CHECK_ARG(n_vertices >= 1 && n_faces >= 1, "align_sums: %lld vertices, %lld faces (at least one of each)", (long long)n_vertices,
                  (long long)n_faces);
    PSN_CHECK_ARG(max_dist >= 0.0, "align_sums: max_dist=%g (not negative, not NaN)", max_dist);
    AlignSums a;
    a.P = P; a.Y = Y; a.tri = tri; a.vertices = vertices; a.faces = faces;
    a.n = n; a.n_vertices = n_vertices; a.n_faces = n_faces;
    a.max_dist = max_dist;
    a.has_R = rotation != nullptr ? 1 : 0;
    for (int i = 0; i < 9; ++i) a.R[i] = rotation != nullptr ? rotation[i] : 0.0;
    const int chunks = al_chunks(n);
    hipLaunchKernelGGL(align_sums_kernel, dim3(chunks), dim3(256), 0, (hipStream_t)stream, a, partial);
    PSN_CHECK_LAUNCH("align_sums");
    hipLaunchKernelGGL(align_reduce_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)partial, chunks, sums,
                       reinterpret_cast<long long*>(counts));
    PSN_CHECK_LAUNCH("align_sums (reduce)");
    return PSN_OK;
}
