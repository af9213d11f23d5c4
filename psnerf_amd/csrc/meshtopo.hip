// Mesh connectivity on the device: the edge table of a triangle mesh, what follows from it (closedness, orientation, vertex rings),
// vertex normals over per-vertex corner runs, the lambda | mu smoothing step and the area / volume sums.  The numpy definition is
// psnerf_amd/meshtopo.py:host_* and psnerf_amd/meshsmooth.py:host_smooth; every output but the two sums equals it bit for bit (the
// build's -ffp-contract=off keeps every product and sum a separate IEEE operation).  The pattern is meshsimplify.hip's: key kernels,
// a stable torch.sort, run bounds, then a kernel that walks each run in a fixed order.
//   psn_topo_edge_keys       a thread per face: the undirected key min(a, b) V + max(a, b) of its three half-edges h = 3 f + k
//   psn_topo_edges           a thread per sorted half-edge: its edge's rank; the head of each run walks it (count, forward) and
//                            writes the edge, the vertex flags and the class counters
//   psn_topo_ring_keys       a thread per edge: the two directed keys u V + w
//   psn_topo_corner_keys     a thread per face: its three vertex ids into the corner-major list j = k F + f
//   psn_topo_runs            a thread per sorted key: start[x] = the first position whose key / div is >= x (the run bounds), and the
//                            remainders key % div (the ring's neighbours)
//   psn_topo_vertex_normals  a thread per vertex: its corner run in ascending (k, f), from +0.0, then the normalisation
//   psn_topo_smooth_step     a thread per vertex: the mean of its ring in ascending neighbour index, x + s (m - x)
//   psn_topo_measures        area and signed volume: a fixed grid of per-workgroup partial sums and a fixed-order second step
// No floating-point atomics anywhere: two runs give the same bits.  Integer counters: ballot + popcount per wave, one integer atomic
// per workgroup and counter.  Vector memory instructions only.
//
// psn_topo_smooth_step is a gather of 24-byte rows behind one index load: no LDS, no scratch.  Vertices stay [V, 3] (rows of three
// doubles): a neighbour's three coordinates then share one 64-byte sector three times out of four, where three planes [3, V] would
// touch three sectors per neighbour; the index loads ring[start .. end) of neighbouring lanes are consecutive runs.  Marching cubes
// emits vertices lattice point by lattice point, so the rows a wave gathers lie within a few lattice planes of each other and are
// served by L2.  The sums are dependent chains in the definition's order, one thread per accumulator triple.
// Every loop runs over a run [start, end) whose ends are clamped into the array they index: the static bound is the array length.
#include "common.h"

namespace psn {

#define TOPO_SENTINEL 0x7fffffffffffffffLL

static inline unsigned topo_blocks(int64_t n, int64_t cap) {
    int64_t b = (n + 255) / 256;
    return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

__device__ __forceinline__ bool topo_in(int64_t i, int64_t n) { return i >= 0 && i < n; }

__global__ __launch_bounds__(256) void topo_edge_keys_kernel(const int64_t* __restrict__ faces, int64_t n_faces, int64_t n_vertices,
                                                             int64_t* __restrict__ keys, int* __restrict__ status) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n_faces; t += stride) {
        const int64_t i = faces[3 * t], j = faces[3 * t + 1], k = faces[3 * t + 2];
        int64_t k0 = TOPO_SENTINEL, k1 = TOPO_SENTINEL, k2 = TOPO_SENTINEL;
        if (!topo_in(i, n_vertices) || !topo_in(j, n_vertices) || !topo_in(k, n_vertices)) {
            atomicOr(status, PSN_TOPO_E_INDEX);
        } else if (i != j && j != k && i != k) {
            k0 = (i < j ? i : j) * n_vertices + (i < j ? j : i);
            k1 = (j < k ? j : k) * n_vertices + (j < k ? k : j);
            k2 = (k < i ? k : i) * n_vertices + (k < i ? i : k);
        }
        keys[3 * t] = k0; keys[3 * t + 1] = k1; keys[3 * t + 2] = k2;
    }
}

// counters: boundary, non-manifold, inconsistent edges; degenerate (or skipped) faces
__global__ __launch_bounds__(256) void topo_edges_kernel(const int64_t* __restrict__ sorted_keys, const int64_t* __restrict__ order,
                                                         const int64_t* __restrict__ rank_incl, int64_t n_half,
                                                         const int64_t* __restrict__ faces, int64_t n_vertices, int64_t n_edges,
                                                         int64_t* __restrict__ edges, int* __restrict__ count, int* __restrict__ forward,
                                                         int64_t* __restrict__ halfedge_edge, unsigned char* __restrict__ vertex_used,
                                                         unsigned char* __restrict__ vertex_open, unsigned long long* __restrict__ counters) {
    __shared__ unsigned long long in_wave[4][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t stride = (int64_t)gridDim.x * 256;
    const int64_t key_end = n_vertices * n_vertices;
    unsigned long long total[4] = {0ull, 0ull, 0ull, 0ull};       // (lane 0 of each wave)
    for (int64_t base = (int64_t)blockIdx.x * 256; base < n_half; base += stride) {   // workgroup-uniform: every lane votes
        const int64_t at = base + threadIdx.x;
        bool flag[4] = {false, false, false, false};
        if (at < n_half) {
            const int64_t key = sorted_keys[at], h = order[at];
            if (topo_in(h, n_half)) {
                if (!topo_in(key, key_end)) {
                    halfedge_edge[h] = -1;
                    flag[3] = h % 3 == 0;
                } else {
                    const int64_t e = rank_incl[at] - 1;
                    halfedge_edge[h] = topo_in(e, n_edges) ? e : -1;
                    if (topo_in(e, n_edges) && (at == 0 || sorted_keys[at - 1] != key)) {
                        int64_t cnt = 0, fwd = 0;
                        for (int64_t j = at; j < n_half && sorted_keys[j] == key; ++j) {
                            const int64_t hh = order[j];
                            if (topo_in(hh, n_half)) {
                                const int64_t f = hh / 3, k = hh - 3 * f;
                                fwd += faces[hh] < faces[3 * f + (k + 1) % 3] ? 1 : 0;
                            }
                            ++cnt;
                        }
                        const int64_t lo = key / n_vertices, hi = key - lo * n_vertices;
                        edges[2 * e] = lo; edges[2 * e + 1] = hi;
                        count[e] = (int)(cnt > 0x7fffffffLL ? 0x7fffffffLL : cnt);
                        forward[e] = (int)(fwd > 0x7fffffffLL ? 0x7fffffffLL : fwd);
                        vertex_used[lo] = vertex_used[hi] = 1;                    // (every writer stores the same byte)
                        if (cnt != 2) vertex_open[lo] = vertex_open[hi] = 1;
                        flag[0] = cnt == 1;
                        flag[1] = cnt > 2;
                        flag[2] = cnt == 2 && fwd != 1;
                    }
                }
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) total[q] += (unsigned long long)__popcll(__ballot(flag[q] ? 1 : 0));
    }
    if (lane == 0)
        for (int q = 0; q < 4; ++q) in_wave[wave][q] = total[q];
    __syncthreads();
    if (threadIdx.x < 4) {
        const unsigned long long sum = (in_wave[0][threadIdx.x] + in_wave[1][threadIdx.x]) + (in_wave[2][threadIdx.x] + in_wave[3][threadIdx.x]);
        if (sum) atomicAdd(counters + threadIdx.x, sum);
    }
}

__global__ __launch_bounds__(256) void topo_ring_keys_kernel(const int64_t* __restrict__ edges, int64_t n_edges, int64_t n_vertices,
                                                             int64_t* __restrict__ keys) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n_edges; e += stride) {
        const int64_t lo = edges[2 * e], hi = edges[2 * e + 1];
        const bool ok = topo_in(lo, n_vertices) && topo_in(hi, n_vertices);      // (an edge table that is not this module's sorts last)
        keys[2 * e] = ok ? lo * n_vertices + hi : TOPO_SENTINEL;
        keys[2 * e + 1] = ok ? hi * n_vertices + lo : TOPO_SENTINEL;
    }
}

__global__ __launch_bounds__(256) void topo_corner_keys_kernel(const int64_t* __restrict__ faces, int64_t n_faces, int64_t n_vertices,
                                                               int64_t* __restrict__ keys, int* __restrict__ status) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n_faces; t += stride) {
        const int64_t i = faces[3 * t], j = faces[3 * t + 1], k = faces[3 * t + 2];
        const bool ok = topo_in(i, n_vertices) && topo_in(j, n_vertices) && topo_in(k, n_vertices);
        if (!ok) atomicOr(status, PSN_TOPO_E_INDEX);
        keys[t] = ok ? i : n_vertices;                    // a skipped face sorts behind every vertex's run
        keys[n_faces + t] = ok ? j : n_vertices;
        keys[2 * n_faces + t] = ok ? k : n_vertices;
    }
}

__device__ __forceinline__ int64_t topo_owner(int64_t key, int64_t div, int64_t n_vertices) {
    if (key < 0) return n_vertices;
    const int64_t u = key / div;
    return u > n_vertices ? n_vertices : u;
}

__global__ __launch_bounds__(256) void topo_runs_kernel(const int64_t* __restrict__ sorted_keys, int64_t n, int64_t div, int64_t n_vertices,
                                                        int64_t* __restrict__ start, int64_t* __restrict__ rem) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t at = (int64_t)blockIdx.x * 256 + threadIdx.x; at < n; at += stride) {
        const int64_t key = sorted_keys[at];
        const int64_t u = topo_owner(key, div, n_vertices);
        const int64_t prev = at == 0 ? -1 : topo_owner(sorted_keys[at - 1], div, n_vertices);
        for (int64_t x = prev + 1; x <= u; ++x) start[x] = at;                   // (prev + 1 >= 0, u <= n_vertices: inside start[V + 1])
        if (at == n - 1)
            for (int64_t x = u + 1; x <= n_vertices; ++x) start[x] = n;
        if (rem != nullptr) rem[at] = u < n_vertices ? key - u * div : -1;
    }
}

__device__ __forceinline__ void topo_cross(const double* __restrict__ p, int64_t i, int64_t j, int64_t k, double& nx, double& ny, double& nz) {
    const double ax = p[3 * i], ay = p[3 * i + 1], az = p[3 * i + 2];
    const double abx = p[3 * j] - ax, aby = p[3 * j + 1] - ay, abz = p[3 * j + 2] - az;
    const double acx = p[3 * k] - ax, acy = p[3 * k + 1] - ay, acz = p[3 * k + 2] - az;
    nx = aby * acz - abz * acy; ny = abz * acx - abx * acz; nz = abx * acy - aby * acx;
}

__global__ __launch_bounds__(256) void topo_vertex_normals_kernel(const double* __restrict__ vertices, const int64_t* __restrict__ faces,
                                                                  int64_t n_faces, int64_t n_vertices, const int64_t* __restrict__ corner_start,
                                                                  const int64_t* __restrict__ corner, int uniform, double* __restrict__ normals) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    const int64_t three_f = 3 * n_faces;
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n_vertices; v += stride) {
        int64_t s = corner_start[v], e = corner_start[v + 1];
        s = s < 0 ? 0 : s;
        e = e > three_f ? three_f : e;
        double mx = 0.0, my = 0.0, mz = 0.0;
        for (int64_t at = s; at < e; ++at) {
            const int64_t c = corner[at];                 // k F + f
            if (!topo_in(c, three_f)) continue;
            const int64_t f = c % n_faces;
            const int64_t i = faces[3 * f], j = faces[3 * f + 1], k = faces[3 * f + 2];
            if (!topo_in(i, n_vertices) || !topo_in(j, n_vertices) || !topo_in(k, n_vertices)) continue;
            double nx, ny, nz;
            topo_cross(vertices, i, j, k, nx, ny, nz);
            if (uniform) {
                const double len = sqrt((nx * nx + ny * ny) + nz * nz);
                const bool has = len > 0.0;
                const double d = has ? len : 1.0;
                nx = has ? nx / d : 0.0; ny = has ? ny / d : 0.0; nz = has ? nz / d : 0.0;
            }
            mx += nx; my += ny; mz += nz;
        }
        const double length = sqrt((mx * mx + my * my) + mz * mz);
        const bool has = length > 0.0;                    // (false for a NaN)
        const double d = has ? length : 1.0;
        normals[3 * v] = has ? mx / d : 0.0;
        normals[3 * v + 1] = has ? my / d : 0.0;
        normals[3 * v + 2] = has ? mz / d : 0.0;
    }
}

__global__ __launch_bounds__(256) void topo_smooth_step_kernel(const double* __restrict__ x, int64_t n_vertices, const int64_t* __restrict__ ring_start,
                                                               const int64_t* __restrict__ ring, int64_t n_ring,
                                                               const unsigned char* __restrict__ pinned, double s, double* __restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n_vertices; v += stride) {
        int64_t b = ring_start[v], e = ring_start[v + 1];
        b = b < 0 ? 0 : b;
        e = e > n_ring ? n_ring : e;
        const double px = x[3 * v], py = x[3 * v + 1], pz = x[3 * v + 2];
        double ox = px, oy = py, oz = pz;
        if (e > b && !(pinned != nullptr && pinned[v])) {
            double ax = 0.0, ay = 0.0, az = 0.0;
            for (int64_t at = b; at < e; ++at) {
                const int64_t w = ring[at];
                if (!topo_in(w, n_vertices)) continue;   // (a ring that is not this module's must not read out of bounds)
                ax += x[3 * w]; ay += x[3 * w + 1]; az += x[3 * w + 2];
            }
            const double n = (double)(e - b);
            const double mx = ax / n, my = ay / n, mz = az / n;
            ox = px + s * (mx - px); oy = py + s * (my - py); oz = pz + s * (mz - pz);
        }
        out[3 * v] = ox; out[3 * v + 1] = oy; out[3 * v + 2] = oz;
    }
}

__device__ __forceinline__ double topo_wave_sum(double value) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) value += __shfl_down(value, o, 64);
    return value;                                         // (lane 0 holds the wave's sum)
}

__global__ __launch_bounds__(256) void topo_measures_kernel(const double* __restrict__ vertices, const int64_t* __restrict__ faces, int64_t n_faces,
                                                            int64_t n_vertices, double* __restrict__ partial) {
    __shared__ double in_wave[4][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t stride = (int64_t)gridDim.x * 256;
    double area = 0.0, volume = 0.0;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n_faces; t += stride) {
        const int64_t i = faces[3 * t], j = faces[3 * t + 1], k = faces[3 * t + 2];
        if (!topo_in(i, n_vertices) || !topo_in(j, n_vertices) || !topo_in(k, n_vertices)) continue;
        double nx, ny, nz;
        topo_cross(vertices, i, j, k, nx, ny, nz);
        area += 0.5 * sqrt((nx * nx + ny * ny) + nz * nz);
        const double ax = vertices[3 * i], ay = vertices[3 * i + 1], az = vertices[3 * i + 2];
        const double bx = vertices[3 * j], by = vertices[3 * j + 1], bz = vertices[3 * j + 2];
        const double cx = vertices[3 * k], cy = vertices[3 * k + 1], cz = vertices[3 * k + 2];
        volume += ((ax * (by * cz - bz * cy) + ay * (bz * cx - bx * cz)) + az * (bx * cy - by * cx)) / 6.0;
    }
    area = topo_wave_sum(area);
    volume = topo_wave_sum(volume);
    if (lane == 0) { in_wave[wave][0] = area; in_wave[wave][1] = volume; }
    __syncthreads();
    if (threadIdx.x < 2)
        partial[2 * blockIdx.x + threadIdx.x] = (in_wave[0][threadIdx.x] + in_wave[1][threadIdx.x]) + (in_wave[2][threadIdx.x] + in_wave[3][threadIdx.x]);
}

// one wave: lane l adds the partial sums l, l + 64, ... in that order, then the wave's tree
__global__ __launch_bounds__(64) void topo_measures_final_kernel(const double* __restrict__ partial, int n_partial, double* __restrict__ out) {
    double area = 0.0, volume = 0.0;
    for (int b = threadIdx.x; b < n_partial; b += 64) { area += partial[2 * b]; volume += partial[2 * b + 1]; }
    area = topo_wave_sum(area);
    volume = topo_wave_sum(volume);
    if (threadIdx.x == 0) { out[0] = area; out[1] = volume; }
}

static int topo_check_sizes(int64_t n_faces, int64_t n_vertices, const char* what) {
    PSN_CHECK_ARG(n_vertices >= 0 && n_faces >= 0, "%s: n_vertices=%lld, n_faces=%lld", what, (long long)n_vertices, (long long)n_faces);
    if (n_vertices > PSN_CC_MAX_VERTICES || n_faces > PSN_CC_MAX_FACES) {
        set_error("%s: n_vertices=%lld (0 .. %lld), n_faces=%lld (0 .. %lld)", what, (long long)n_vertices, (long long)PSN_CC_MAX_VERTICES,
                  (long long)n_faces, (long long)PSN_CC_MAX_FACES);
        return PSN_E_UNSUPPORTED;
    }
    return PSN_OK;
}

}  // namespace psn

extern "C" int psn_topo_edge_keys(const int64_t* faces, int64_t n_faces, int64_t n_vertices, int64_t* keys, int* status, void* stream) {
    using namespace psn;
    if (int rc = topo_check_sizes(n_faces, n_vertices, "topo_edge_keys")) return rc;
    PSN_CHECK_ARG(status != nullptr, "topo_edge_keys: null status word");
    if (n_faces == 0) return PSN_OK;
    PSN_CHECK_ARG(faces && keys, "topo_edge_keys: null pointer");
    hipLaunchKernelGGL(topo_edge_keys_kernel, dim3(topo_blocks(n_faces, 65536)), dim3(256), 0, (hipStream_t)stream, faces, n_faces, n_vertices, keys,
                       status);
    PSN_CHECK_LAUNCH("topo_edge_keys");
    return PSN_OK;
}

extern "C" int psn_topo_edges(const int64_t* sorted_keys, const int64_t* order, const int64_t* rank_incl, const int64_t* faces, int64_t n_faces,
                              int64_t n_vertices, int64_t n_edges, int64_t* edges, int* count, int* forward, int64_t* halfedge_edge,
                              unsigned char* vertex_used, unsigned char* vertex_open, long long* counters, void* stream) {
    using namespace psn;
    if (int rc = topo_check_sizes(n_faces, n_vertices, "topo_edges")) return rc;
    PSN_CHECK_ARG(n_edges >= 0 && n_edges <= 3 * n_faces, "topo_edges: %lld edges of %lld faces", (long long)n_edges, (long long)n_faces);
    PSN_CHECK_ARG(counters != nullptr, "topo_edges: null counters");
    PSN_CHECK_ARG((vertex_used && vertex_open) || n_vertices == 0, "topo_edges: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(counters, 0, 4 * sizeof(long long), s) != hipSuccess ||
        (n_vertices > 0 && (hipMemsetAsync(vertex_used, 0, n_vertices, s) != hipSuccess || hipMemsetAsync(vertex_open, 0, n_vertices, s) != hipSuccess))) {
        set_error("topo_edges: hipMemsetAsync failed");
        return PSN_E_LAUNCH;
    }
    if (n_faces == 0) return PSN_OK;
    PSN_CHECK_ARG(sorted_keys && order && rank_incl && faces && halfedge_edge && ((edges && count && forward) || n_edges == 0), "topo_edges: null pointer");
    hipLaunchKernelGGL(topo_edges_kernel, dim3(topo_blocks(3 * n_faces, 65536)), dim3(256), 0, s, sorted_keys, order, rank_incl, 3 * n_faces, faces,
                       n_vertices, n_edges, edges, count, forward, halfedge_edge, vertex_used, vertex_open,
                       reinterpret_cast<unsigned long long*>(counters));
    PSN_CHECK_LAUNCH("topo_edges");
    return PSN_OK;
}

extern "C" int psn_topo_ring_keys(const int64_t* edges, int64_t n_edges, int64_t n_vertices, int64_t* keys, void* stream) {
    using namespace psn;
    if (int rc = topo_check_sizes(0, n_vertices, "topo_ring_keys")) return rc;
    PSN_CHECK_ARG(n_edges >= 0 && n_edges <= 3 * PSN_CC_MAX_FACES, "topo_ring_keys: n_edges=%lld", (long long)n_edges);
    if (n_edges == 0) return PSN_OK;
    PSN_CHECK_ARG(edges && keys, "topo_ring_keys: null pointer");
    hipLaunchKernelGGL(topo_ring_keys_kernel, dim3(topo_blocks(n_edges, 65536)), dim3(256), 0, (hipStream_t)stream, edges, n_edges, n_vertices, keys);
    PSN_CHECK_LAUNCH("topo_ring_keys");
    return PSN_OK;
}

extern "C" int psn_topo_corner_keys(const int64_t* faces, int64_t n_faces, int64_t n_vertices, int64_t* keys, int* status, void* stream) {
    using namespace psn;
    if (int rc = topo_check_sizes(n_faces, n_vertices, "topo_corner_keys")) return rc;
    PSN_CHECK_ARG(status != nullptr, "topo_corner_keys: null status word");
    if (n_faces == 0) return PSN_OK;
    PSN_CHECK_ARG(faces && keys, "topo_corner_keys: null pointer");
    hipLaunchKernelGGL(topo_corner_keys_kernel, dim3(topo_blocks(n_faces, 65536)), dim3(256), 0, (hipStream_t)stream, faces, n_faces, n_vertices, keys,
                       status);
    PSN_CHECK_LAUNCH("topo_corner_keys");
    return PSN_OK;
}

extern "C" int psn_topo_runs(const int64_t* sorted_keys, int64_t n_keys, int64_t div, int64_t n_vertices, int64_t* start, int64_t* rem,
                             void* stream) {
    using namespace psn;
    if (int rc = topo_check_sizes(0, n_vertices, "topo_runs")) return rc;
    PSN_CHECK_ARG(n_keys >= 0 && n_keys <= 6 * PSN_CC_MAX_FACES, "topo_runs: n_keys=%lld", (long long)n_keys);
    PSN_CHECK_ARG(div >= 1, "topo_runs: div=%lld (at least 1)", (long long)div);
    PSN_CHECK_ARG(start != nullptr, "topo_runs: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(start, 0, sizeof(int64_t) * (n_vertices + 1), s) != hipSuccess) {
        set_error("topo_runs: hipMemsetAsync failed");
        return PSN_E_LAUNCH;
    }
    if (n_keys == 0) return PSN_OK;
    PSN_CHECK_ARG(sorted_keys != nullptr, "topo_runs: null pointer");
    hipLaunchKernelGGL(topo_runs_kernel, dim3(topo_blocks(n_keys, 65536)), dim3(256), 0, s, sorted_keys, n_keys, div, n_vertices, start, rem);
    PSN_CHECK_LAUNCH("topo_runs");
    return PSN_OK;
}

extern "C" int psn_topo_vertex_normals(const double* vertices, const int64_t* faces, int64_t n_faces, int64_t n_vertices,
                                       const int64_t* corner_start, const int64_t* corner, int weight, double* normals, void* stream) {
    using namespace psn;
    if (int rc = topo_check_sizes(n_faces, n_vertices, "topo_vertex_normals")) return rc;
    PSN_CHECK_ARG(weight == PSN_TOPO_WEIGHT_AREA || weight == PSN_TOPO_WEIGHT_UNIFORM, "topo_vertex_normals: weight=%d (PSN_TOPO_WEIGHT_*)", weight);
    if (n_vertices == 0) return PSN_OK;
    PSN_CHECK_ARG(vertices && corner_start && normals && ((faces && corner) || n_faces == 0), "topo_vertex_normals: null pointer");
    hipLaunchKernelGGL(topo_vertex_normals_kernel, dim3(topo_blocks(n_vertices, 65536)), dim3(256), 0, (hipStream_t)stream, vertices, faces, n_faces,
                       n_vertices, corner_start, corner, weight == PSN_TOPO_WEIGHT_UNIFORM ? 1 : 0, normals);
    PSN_CHECK_LAUNCH("topo_vertex_normals");
    return PSN_OK;
}

extern "C" int psn_topo_smooth_step(const double* x, int64_t n_vertices, const int64_t* ring_start, const int64_t* ring, int64_t n_ring,
                                    const unsigned char* pinned, double s, double* out, void* stream) {
    using namespace psn;
    if (int rc = topo_check_sizes(0, n_vertices, "topo_smooth_step")) return rc;
    PSN_CHECK_ARG(n_ring >= 0 && n_ring <= 6 * PSN_CC_MAX_FACES, "topo_smooth_step: n_ring=%lld", (long long)n_ring);
    PSN_CHECK_ARG(s == s && s >= -1.79e308 && s <= 1.79e308, "topo_smooth_step: factor %g", s);
    if (n_vertices == 0) return PSN_OK;
    PSN_CHECK_ARG(x && ring_start && out && x != out && (ring || n_ring == 0), "topo_smooth_step: null pointer, or out == x");
    hipLaunchKernelGGL(topo_smooth_step_kernel, dim3(topo_blocks(n_vertices, 65536)), dim3(256), 0, (hipStream_t)stream, x, n_vertices, ring_start, ring,
                       n_ring, pinned, s, out);
    PSN_CHECK_LAUNCH("topo_smooth_step");
    return PSN_OK;
}

extern "C" int psn_topo_measures(const double* vertices, const int64_t* faces, int64_t n_faces, int64_t n_vertices, double* partial, double* out,
                                 void* stream) {
    using namespace psn;
    if (int rc = topo_check_sizes(n_faces, n_vertices, "topo_measures")) return rc;
    PSN_CHECK_ARG(out != nullptr, "topo_measures: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (n_faces == 0 || n_vertices == 0) {
        if (hipMemsetAsync(out, 0, 2 * sizeof(double), s) != hipSuccess) {
            set_error("topo_measures: hipMemsetAsync failed");
            return PSN_E_LAUNCH;
        }
        return PSN_OK;
    }
    PSN_CHECK_ARG(vertices && faces && partial, "topo_measures: null pointer");
    const unsigned blocks = topo_blocks(n_faces, PSN_TOPO_MEASURE_BLOCKS);
    hipLaunchKernelGGL(topo_measures_kernel, dim3(blocks), dim3(256), 0, s, vertices, faces, n_faces, n_vertices, partial);
    hipLaunchKernelGGL(topo_measures_final_kernel, dim3(1), dim3(64), 0, s, (const double*)partial, (int)blocks, out);
    PSN_CHECK_LAUNCH("topo_measures");
    return PSN_OK;
}
