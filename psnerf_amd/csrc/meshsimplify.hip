// Mesh simplification on the device: quadric vertex clustering on a uniform grid (after Lindstrom's out-of-core simplification).  All
// vertices of one grid cell become one vertex at the minimiser of the cell's regularised quadric error.  The numpy definition -- the
// grid, the order of every sum and the written-out LDL^T solve -- is psnerf_amd/meshsimplify.py:host_*; these kernels repeat it
// operation for operation in float64 (the build's -ffp-contract=off keeps every product and sum a separate IEEE operation), so
// the positions equal numpy's bit for bit.  The sorts and scans between the kernels are torch's (meshsimplify.py:_DeviceGrid).
//   psn_vc_cell_keys   a thread per vertex: the key of its grid cell
//   psn_vc_face_keys   a thread per face: the faces re-indexed through cluster[], three corner keys cluster * 3F + 3f + k (sorted,
//                      they give each cluster its run of (face, corner) pairs in ascending order) and the rotated 3 x 21-bit face
//                      key (equal keys = duplicates; -1 = degenerate)
//   psn_vc_solve       a wave per cluster: centroid over its vertex run, quadric over its corner run, solve, clamp
//   psn_vc_face_flags  a thread per face: vertex keep flags from the kept faces, and the flipped flag
// No floating-point atomics anywhere: two runs give the same bits.
//
// psn_vc_solve.  The definition adds a cluster's terms one after the other, so one thread owns each accumulator -- but the terms
// themselves are independent.  A wave takes 64 entries of the run at a time: every lane loads one entry and forms its products
// (3 coordinates for the centroid; 6 of n n^T and 3 of n (n . (a - x0)) for the quadric) into LDS, then lane q adds column q of the
// 64 rows in row order.  The nine dependent chains of additions run side by side, and the gathers (corner key -> face -> three
// vertices) are 64 wide.  A coarse grid with a few clusters of hundreds of thousands of corners costs 64 additions per 64 entries
// and wave instead of 576; a fine grid with a dozen entries per cluster costs one pass.  Lane 0 solves and clamps.
// The layout is chosen for the order of the sums and for the long runs of a coarse grid, NOT tuned for the common fine grid: there
// a run is about a dozen entries, so a dozen lanes gather, 9 of 64 add and 1 solves.  Measured at 683 k faces / 54.9 k clusters the
// launch takes 0.066 ms of a 1.04 ms call whose time is in the sorts (profiles/mesh_simplify.json), so it was left at that.
// The workgroup IS the wave (64 threads), so __syncthreads() orders the LDS hand-offs at the price of a one-wave barrier.
// Every loop runs over a run [start, end) whose ends are clamped into the array they index: the static bound is the array length.
#include "common.h"

namespace psn {

#define VC_ID_BITS 21

static inline unsigned vc_blocks(int64_t n, int per_block, int64_t cap) {
    int64_t b = (n + per_block - 1) / per_block;
    return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

__device__ __forceinline__ int64_t vc_cell(double x, double origin, double h, int dim) {
    double q = floor((x - origin) / h);
    q = q < 0.0 ? 0.0 : q;                       // (a NaN fails both comparisons; the caller refused non-finite vertices already,
    q = q > (double)(dim - 1) ? (double)(dim - 1) : q;
    return q >= 0.0 ? (int64_t)q : 0;            //  and this keeps the key in range whatever arrives)
}

__global__ __launch_bounds__(256) void vc_cell_keys_kernel(const double* __restrict__ vertices, int64_t n_vertices, double ox, double oy, double oz,
                                                           double h, int dx, int dy, int dz, int64_t* __restrict__ keys) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n_vertices; v += stride) {
        const int64_t cx = vc_cell(vertices[3 * v], ox, h, dx), cy = vc_cell(vertices[3 * v + 1], oy, h, dy), cz = vc_cell(vertices[3 * v + 2], oz, h, dz);
        keys[v] = (cz * dy + cy) * dx + cx;
    }
}

__global__ __launch_bounds__(256) void vc_face_keys_kernel(const int64_t* __restrict__ faces, int64_t n_faces, int64_t n_vertices,
                                                           const int64_t* __restrict__ cluster, int64_t* __restrict__ corner_keys,
                                                           int64_t* __restrict__ face_keys, int64_t* __restrict__ g, int* __restrict__ status) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    const int64_t three_f = 3 * n_faces;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n_faces; t += stride) {
        const int64_t i = faces[3 * t], j = faces[3 * t + 1], k = faces[3 * t + 2];
        int64_t g0 = 0, g1 = 0, g2 = 0;
        bool ok = true;
        if (i < 0 || j < 0 || k < 0 || i >= n_vertices || j >= n_vertices || k >= n_vertices) {
            atomicOr(status, PSN_VC_E_INDEX);
            ok = false;
        } else {
            g0 = cluster[i]; g1 = cluster[j]; g2 = cluster[k];
            if (g0 < 0 || g1 < 0 || g2 < 0 || g0 >= PSN_VC_MAX_CLUSTERS || g1 >= PSN_VC_MAX_CLUSTERS || g2 >= PSN_VC_MAX_CLUSTERS) {
                atomicOr(status, PSN_VC_E_CLUSTER);
                ok = false;
                g0 = g1 = g2 = 0;
            }
        }
        g[3 * t] = g0; g[3 * t + 1] = g1; g[3 * t + 2] = g2;
        if (corner_keys != nullptr) {   // a skipped face sorts behind every cluster's run
            const int64_t past = (int64_t)PSN_VC_MAX_CLUSTERS + 1;
            corner_keys[3 * t] = (ok ? g0 : past) * three_f + 3 * t;
            corner_keys[3 * t + 1] = (ok ? g1 : past) * three_f + 3 * t + 1;
            corner_keys[3 * t + 2] = (ok ? g2 : past) * three_f + 3 * t + 2;
        }
        int64_t key = -1;
        if (ok && g0 != g1 && g1 != g2 && g0 != g2) {
            int64_t r0 = g0, r1 = g1, r2 = g2;                     // rotate the smallest id to the front, orientation kept
            if (!(g0 < g1 && g0 < g2)) {
                if (g1 < g2) { r0 = g1; r1 = g2; r2 = g0; }
                else { r0 = g2; r1 = g0; r2 = g1; }
            }
            key = (((r0 << VC_ID_BITS) + r1) << VC_ID_BITS) + r2;
        }
        face_keys[t] = key;
    }
}

__device__ __forceinline__ void vc_cross(const double* __restrict__ p, int64_t i, int64_t j, int64_t k, double& nx, double& ny, double& nz) {
    const double ax = p[3 * i], ay = p[3 * i + 1], az = p[3 * i + 2];
    const double abx = p[3 * j] - ax, aby = p[3 * j + 1] - ay, abz = p[3 * j + 2] - az;
    const double acx = p[3 * k] - ax, acy = p[3 * k + 1] - ay, acz = p[3 * k + 2] - az;
    nx = aby * acz - abz * acy; ny = abz * acx - abx * acz; nz = abx * acy - aby * acx;
}

__device__ __forceinline__ double vc_clamp(double x, double lo, double hi) {
    x = x < lo ? lo : x;
    return x > hi ? hi : x;
}

__global__ __launch_bounds__(64) void vc_solve_kernel(const double* __restrict__ vertices, const int64_t* __restrict__ faces, int64_t n_faces,
                                                      int64_t n_vertices, const int64_t* __restrict__ vertex_order,
                                                      const int64_t* __restrict__ vertex_start, const int64_t* __restrict__ cell_key_sorted,
                                                      const int64_t* __restrict__ corner_sorted, const int64_t* __restrict__ corner_start,
                                                      int64_t n_clusters, double ox, double oy, double oz, double h, int dx, int dy,
                                                      double regularisation, double* __restrict__ positions, unsigned char* __restrict__ clamped) {
    __shared__ double prod[64 * 9];
    __shared__ double acc[12];       // x0 [3], A00 A01 A02 A11 A12 A22, r [3]
    const int lane = threadIdx.x;
    const int64_t three_f = 3 * n_faces;
    for (int64_t c = blockIdx.x; c < n_clusters; c += gridDim.x) {
        int64_t vs = vertex_start[c], ve = vertex_start[c + 1];
        vs = vs < 0 ? 0 : vs;
        ve = ve > n_vertices ? n_vertices : ve;
        if (ve <= vs) {   // (no cluster is empty; a table that is not this module's must not divide by zero)
            if (lane < 3) positions[3 * c + lane] = 0.0;
            if (lane == 0) clamped[c] = 0;
            continue;
        }
        // ---- centroid: the cluster's vertices in ascending vertex index
        double sum = 0.0;
        for (int64_t base = vs; base < ve; base += 64) {
            const int64_t at = base + lane;
            double px = 0.0, py = 0.0, pz = 0.0;
            if (at < ve) {
                const int64_t v = vertex_order[at];
                if (v >= 0 && v < n_vertices) { px = vertices[3 * v]; py = vertices[3 * v + 1]; pz = vertices[3 * v + 2]; }
            }
            prod[lane * 9] = px; prod[lane * 9 + 1] = py; prod[lane * 9 + 2] = pz;
            __syncthreads();
            const int count = (int)(ve - base < 64 ? ve - base : 64);
            if (lane < 3)
                for (int j = 0; j < count; ++j) sum += prod[j * 9 + lane];
            __syncthreads();
        }
        if (lane < 3) acc[lane] = sum / (double)(ve - vs);
        __syncthreads();
        const double x0 = acc[0], y0 = acc[1], z0 = acc[2];
        // ---- quadric: the cluster's (face, corner) pairs in ascending order
        int64_t cs = corner_start[c], ce = corner_start[c + 1];
        cs = cs < 0 ? 0 : cs;
        ce = ce > three_f ? three_f : ce;
        sum = 0.0;
        for (int64_t base = cs; base < ce; base += 64) {
            const int64_t at = base + lane;
            double p[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            if (at < ce) {
                const int64_t fc = corner_sorted[at] - c * three_f;   // 3 f + corner
                if (fc >= 0 && fc < three_f) {
                    const int64_t f = fc / 3;
                    const int64_t i = faces[3 * f], j = faces[3 * f + 1], k = faces[3 * f + 2];
                    if (i >= 0 && j >= 0 && k >= 0 && i < n_vertices && j < n_vertices && k < n_vertices) {
                        double nx, ny, nz;
                        vc_cross(vertices, i, j, k, nx, ny, nz);
                        const double d = (nx * (vertices[3 * i] - x0) + ny * (vertices[3 * i + 1] - y0)) + nz * (vertices[3 * i + 2] - z0);
                        p[0] = nx * nx; p[1] = nx * ny; p[2] = nx * nz; p[3] = ny * ny; p[4] = ny * nz; p[5] = nz * nz;
                        p[6] = nx * d; p[7] = ny * d; p[8] = nz * d;
                    }
                }
            }
#pragma unroll
            for (int q = 0; q < 9; ++q) prod[lane * 9 + q] = p[q];
            __syncthreads();
            const int count = (int)(ce - base < 64 ? ce - base : 64);
            if (lane < 9)
                for (int j = 0; j < count; ++j) sum += prod[j * 9 + lane];
            __syncthreads();
        }
        if (lane < 9) acc[3 + lane] = sum;
        __syncthreads();
        if (lane == 0) {
            const double A00 = acc[3], A01 = acc[4], A02 = acc[5], A11 = acc[6], A12 = acc[7], A22 = acc[8];
            const double rx = acc[9], ry = acc[10], rz = acc[11];
            const double t = (A00 + A11) + A22;
            double x = x0, y = y0, z = z0;
            if (t != 0.0) {
                const double lam = regularisation * t;
                const double m00 = A00 + lam, m11 = A11 + lam, m22 = A22 + lam;
                const double l10 = A01 / m00;
                const double l20 = A02 / m00;
                const double d1 = m11 - l10 * A01;
                const double e21 = A12 - l20 * A01;
                const double l21 = e21 / d1;
                const double d2 = (m22 - l20 * A02) - l21 * e21;
                const double y1 = ry - l10 * rx;
                const double y2 = (rz - l20 * rx) - l21 * y1;
                const double ddz = y2 / d2;
                const double ddy = y1 / d1 - l21 * ddz;
                const double ddx = (rx / m00 - l10 * ddy) - l20 * ddz;
                x = x0 + ddx; y = y0 + ddy; z = z0 + ddz;
            }
            const int64_t key = cell_key_sorted[vs];
            const int64_t cx = key % dx, rest = key / dx;
            const int64_t cy = rest % dy, cz = rest / dy;
            const double qx = vc_clamp(x, ox + (double)cx * h, ox + ((double)cx + 1.0) * h);
            const double qy = vc_clamp(y, oy + (double)cy * h, oy + ((double)cy + 1.0) * h);
            const double qz = vc_clamp(z, oz + (double)cz * h, oz + ((double)cz + 1.0) * h);
            positions[3 * c] = qx; positions[3 * c + 1] = qy; positions[3 * c + 2] = qz;
            clamped[c] = (qx != x || qy != y || qz != z) ? 1 : 0;
        }
        __syncthreads();   // acc[] is rewritten by the next cluster
    }
}

__global__ __launch_bounds__(256) void vc_face_flags_kernel(const double* __restrict__ vertices, const int64_t* __restrict__ faces, int64_t n_faces,
                                                            int64_t n_vertices, const int64_t* __restrict__ g, const double* __restrict__ positions,
                                                            int64_t n_clusters, const unsigned char* __restrict__ face_keep,
                                                            unsigned char* __restrict__ vertex_keep, unsigned char* __restrict__ flipped) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n_faces; t += stride) {
        unsigned char flip = 0;
        if (face_keep[t]) {
            const int64_t i = faces[3 * t], j = faces[3 * t + 1], k = faces[3 * t + 2];
            const int64_t g0 = g[3 * t], g1 = g[3 * t + 1], g2 = g[3 * t + 2];
            if (i >= 0 && j >= 0 && k >= 0 && i < n_vertices && j < n_vertices && k < n_vertices && g0 >= 0 && g1 >= 0 && g2 >= 0 &&
                g0 < n_clusters && g1 < n_clusters && g2 < n_clusters) {
                vertex_keep[g0] = vertex_keep[g1] = vertex_keep[g2] = 1;   // (every writer stores the same byte)
                double nx, ny, nz, mx, my, mz;
                vc_cross(vertices, i, j, k, nx, ny, nz);
                vc_cross(positions, g0, g1, g2, mx, my, mz);
                flip = ((nx * mx + ny * my) + nz * mz) < 0.0 ? 1 : 0;
            }
        }
        flipped[t] = flip;
    }
}

static int vc_check_sizes(int64_t n_faces, int64_t n_vertices, const char* what) {
    PSN_CHECK_ARG(n_vertices >= 0 && n_faces >= 0, "%s: n_vertices=%lld, n_faces=%lld", what, (long long)n_vertices, (long long)n_faces);
    if (n_vertices > PSN_CC_MAX_VERTICES || n_faces > PSN_VC_MAX_FACES) {
        set_error("%s: n_vertices=%lld (0 .. %lld), n_faces=%lld (0 .. %lld)", what, (long long)n_vertices, (long long)PSN_CC_MAX_VERTICES,
                  (long long)n_faces, (long long)PSN_VC_MAX_FACES);
        return PSN_E_UNSUPPORTED;
    }
    return PSN_OK;
}

static int vc_check_grid(double ox, double oy, double oz, double h, int dx, int dy, int dz, const char* what) {
    PSN_CHECK_ARG(ox == ox && oy == oy && oz == oz && h > 0.0 && h <= 1.79e308, "%s: origin (%g, %g, %g), cell edge %g", what, ox, oy, oz, h);
    PSN_CHECK_ARG(dx >= 1 && dy >= 1 && dz >= 1, "%s: dims %d x %d x %d", what, dx, dy, dz);
    if (dx > PSN_VC_MAX_RESOLUTION + 1 || dy > PSN_VC_MAX_RESOLUTION + 1 || dz > PSN_VC_MAX_RESOLUTION + 1) {
        set_error("%s: dims %d x %d x %d (at most %d per axis)", what, dx, dy, dz, PSN_VC_MAX_RESOLUTION + 1);
        return PSN_E_UNSUPPORTED;
    }
    return PSN_OK;
}

}  // namespace psn

extern "C" int psn_vc_cell_keys(const double* vertices, int64_t n_vertices, double ox, double oy, double oz, double h, int dx, int dy, int dz,
                                int64_t* keys, void* stream) {
    using namespace psn;
    if (int rc = vc_check_sizes(0, n_vertices, "vc_cell_keys")) return rc;
    if (int rc = vc_check_grid(ox, oy, oz, h, dx, dy, dz, "vc_cell_keys")) return rc;
    if (n_vertices == 0) return PSN_OK;
    PSN_CHECK_ARG(vertices && keys, "vc_cell_keys: null pointer");
    hipLaunchKernelGGL(vc_cell_keys_kernel, dim3(vc_blocks(n_vertices, 256, 65536)), dim3(256), 0, (hipStream_t)stream, vertices, n_vertices, ox, oy,
                       oz, h, dx, dy, dz, keys);
    PSN_CHECK_LAUNCH("vc_cell_keys");
    return PSN_OK;
}

extern "C" int psn_vc_face_keys(const int64_t* faces, int64_t n_faces, int64_t n_vertices, const int64_t* cluster, int64_t* corner_keys,
                                int64_t* face_keys, int64_t* g, int* status, void* stream) {
    using namespace psn;
    if (int rc = vc_check_sizes(n_faces, n_vertices, "vc_face_keys")) return rc;
    PSN_CHECK_ARG(status != nullptr, "vc_face_keys: null status word");
    if (n_faces == 0) return PSN_OK;
    PSN_CHECK_ARG(faces && face_keys && g && (cluster || n_vertices == 0), "vc_face_keys: null pointer");
    hipLaunchKernelGGL(vc_face_keys_kernel, dim3(vc_blocks(n_faces, 256, 65536)), dim3(256), 0, (hipStream_t)stream, faces, n_faces, n_vertices,
                       cluster, corner_keys, face_keys, g, status);
    PSN_CHECK_LAUNCH("vc_face_keys");
    return PSN_OK;
}

extern "C" int psn_vc_solve(const double* vertices, const int64_t* faces, int64_t n_faces, int64_t n_vertices, const int64_t* vertex_order,
                            const int64_t* vertex_start, const int64_t* cell_key_sorted, const int64_t* corner_sorted,
                            const int64_t* corner_start, int64_t n_clusters, double ox, double oy, double oz, double h, int dx, int dy, int dz,
                            double regularisation, double* positions, unsigned char* clamped, void* stream) {
    using namespace psn;
    if (int rc = vc_check_sizes(n_faces, n_vertices, "vc_solve")) return rc;
    if (int rc = vc_check_grid(ox, oy, oz, h, dx, dy, dz, "vc_solve")) return rc;
    PSN_CHECK_ARG(n_clusters >= 0 && n_clusters <= n_vertices, "vc_solve: %lld clusters of %lld vertices", (long long)n_clusters,
                  (long long)n_vertices);
    if (n_clusters > PSN_VC_MAX_CLUSTERS) {
        set_error("vc_solve: %lld clusters (at most %lld)", (long long)n_clusters, (long long)PSN_VC_MAX_CLUSTERS);
        return PSN_E_UNSUPPORTED;
    }
    PSN_CHECK_ARG(regularisation > 0.0 && regularisation <= 1.79e308, "vc_solve: regularisation=%g (must be > 0)", regularisation);
    if (n_clusters == 0) return PSN_OK;
    PSN_CHECK_ARG(vertices && vertex_order && vertex_start && cell_key_sorted && corner_start && positions && clamped &&
                      ((faces && corner_sorted) || n_faces == 0),
                  "vc_solve: null pointer");
    hipLaunchKernelGGL(vc_solve_kernel, dim3(vc_blocks(n_clusters, 1, 65536)), dim3(64), 0, (hipStream_t)stream, vertices, faces, n_faces, n_vertices,
                       vertex_order, vertex_start, cell_key_sorted, corner_sorted, corner_start, n_clusters, ox, oy, oz, h, dx, dy, regularisation,
                       positions, clamped);
    PSN_CHECK_LAUNCH("vc_solve");
    return PSN_OK;
}

extern "C" int psn_vc_face_flags(const double* vertices, const int64_t* faces, int64_t n_faces, int64_t n_vertices, const int64_t* g,
                                 const double* positions, int64_t n_clusters, const unsigned char* face_keep, unsigned char* vertex_keep,
                                 unsigned char* flipped, void* stream) {
    using namespace psn;
    if (int rc = vc_check_sizes(n_faces, n_vertices, "vc_face_flags")) return rc;
    PSN_CHECK_ARG(n_clusters >= 0 && n_clusters <= n_vertices, "vc_face_flags: %lld clusters of %lld vertices", (long long)n_clusters,
                  (long long)n_vertices);
    PSN_CHECK_ARG(vertex_keep != nullptr || n_clusters == 0, "vc_face_flags: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (n_clusters > 0 && hipMemsetAsync(vertex_keep, 0, n_clusters, s) != hipSuccess) {
        set_error("vc_face_flags: hipMemsetAsync failed");
        return PSN_E_LAUNCH;
    }
    if (n_faces == 0) return PSN_OK;
    PSN_CHECK_ARG(vertices && faces && g && face_keep && flipped && (positions || n_clusters == 0), "vc_face_flags: null pointer");
    hipLaunchKernelGGL(vc_face_flags_kernel, dim3(vc_blocks(n_faces, 256, 65536)), dim3(256), 0, s, vertices, faces, n_faces, n_vertices, g, positions,
                       n_clusters, face_keep, vertex_keep, flipped);
    PSN_CHECK_LAUNCH("vc_face_flags");
    return PSN_OK;
}
