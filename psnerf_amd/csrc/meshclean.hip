// Mesh clean-up on the device: connected components of a triangle mesh, per-component statistics and compaction -- what users of
// the reference pipeline ask of trimesh's split() on the host to separate the object from the floaters and inner shells that marching
// cubes also returns (the reference itself only has --clip).  The numpy definition is psnerf_amd/meshclean.py:host_*.
//   psn_cc_label    labels[v] = the smallest vertex index reachable from v (two vertices are adjacent when one face names both)
//   psn_cc_stats    per component (indexed by its label): vertices, faces, area; a face belongs to the component of its first index
//   psn_cc_flag     face keep flags from a per-label keep table, vertex keep flags from the kept faces
//   psn_cc_compact  the kept vertices (and normals) and the re-indexed kept faces, both in their original order
//
// Labelling is a lock-free union-find in ONE pass over the faces (no rounds, no host read), then a flatten launch.
// parent[] is a forest with parent[x] <= x everywhere and parent[r] == r exactly at the roots.  The only way a root changes is
// atomicCAS(parent + hi, hi, lo) with lo < hi (device scope, carried out at the memory side: valid across the eight XCDs), and the only
// other write is path halving, parent[x] = an ancestor of x, on an x that was read as a non-root.  From these two rules:
//   * a non-root never becomes a root again, so a compare-and-swap on it can never succeed and halving cannot undo a link;
//   * every value parent[x] ever held is x or a smaller node of x's own tree (trees only ever merge), so a STALE read -- a plain store
//     by one workgroup is not reliably seen by another XCD within a launch -- still walks up the same tree, only from further down;
//   * every step of a walk goes to a strictly smaller index: a find takes at most n_vertices steps whatever it reads;
//   * the read that decides a link (parent[hi] == hi) is confirmed by the compare-and-swap itself; a failed swap returns the true
//     parent, which is < hi, and the link re-finds from it: a link retries only with a strictly smaller root;
//   * the larger root goes under the smaller one, so the root of a tree is the smallest index in it: the result does not depend on the
//     order in which the faces were processed (bitwise reproducible).
// Nothing waits for another workgroup.  Both loops carry their static bound explicitly; running into it (impossible by the argument
// above) sets PSN_CC_E_BOUND in the status word instead of spinning.  The flatten launch reads the forest only after the kernel
// boundary made every link visible, and writes the labels to an array of their own.
// Reads of parent[] are relaxed agent-scope atomic loads (L1 is bypassed: fewer stale values, and no torn or cached-in-register reads);
// halving stores are relaxed agent-scope atomic stores.  Vector memory instructions only.
#include "common.h"

namespace psn {

__device__ __forceinline__ int cc_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void cc_store(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The root of x's tree as far as this thread can see it, with path halving; -1 if the static bound ran out.
__device__ __forceinline__ int cc_find(int* __restrict__ parent, int x, int64_t bound) {
    int cur = x;
    for (int64_t step = 0; step <= bound; ++step) {
        const int p = cc_load(parent + cur);
        if (p == cur) return cur;
        const int gp = cc_load(parent + p);
        if (gp != p) cc_store(parent + cur, gp);   // cur is a non-root for good: no compare-and-swap on it can succeed any more
        cur = gp;
    }
    return -1;
}

// Unite the trees of u and v.  Returns false if a static bound ran out.
__device__ __forceinline__ bool cc_link(int* __restrict__ parent, int u, int v, int64_t bound) {
    int a = cc_find(parent, u, bound), b = cc_find(parent, v, bound);
    for (int64_t tries = 0; tries <= bound; ++tries) {
        if (a < 0 || b < 0) return false;
        if (a == b) return true;
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        const int seen = atomicCAS(parent + hi, hi, lo);
        if (seen == hi) return true;
        // hi had been linked already; seen < hi is its parent: go on from there (strictly smaller than hi)
        a = cc_find(parent, seen, bound);
        b = lo;
    }
    return false;
}

__global__ __launch_bounds__(256) void cc_init_kernel(int* __restrict__ parent, int64_t n_vertices) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v < n_vertices) parent[v] = (int)v;
}

__global__ __launch_bounds__(256) void cc_link_kernel(const int64_t* __restrict__ faces, int64_t n_faces, int64_t n_vertices, int* __restrict__ parent,
                                                      int* __restrict__ status) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_faces) return;
    const int64_t i = faces[3 * t], j = faces[3 * t + 1], k = faces[3 * t + 2];
    if (i < 0 || j < 0 || k < 0 || i >= n_vertices || j >= n_vertices || k >= n_vertices) {
        atomicOr(status, PSN_CC_E_INDEX);
        return;
    }
    bool ok = true;
    if (i != j) ok = cc_link(parent, (int)i, (int)j, n_vertices);
    if (ok && j != k) ok = cc_link(parent, (int)j, (int)k, n_vertices);
    if (!ok) atomicOr(status, PSN_CC_E_BOUND);
}

// After the kernel boundary: the forest is final and read-only here.
__global__ __launch_bounds__(256) void cc_flatten_kernel(const int* __restrict__ parent, int64_t n_vertices, int* __restrict__ labels,
                                                         int* __restrict__ status) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= n_vertices) return;
    int cur = (int)v;
    bool found = false;
    for (int64_t step = 0; step <= n_vertices; ++step) {
        const int p = parent[cur];
        if (p == cur) { found = true; break; }
        if (p < 0 || p > cur) break;   // not a forest of this module's making
        cur = p;
    }
    labels[v] = found ? cur : (int)v;
    if (!found) atomicOr(status, PSN_CC_E_BOUND);
}

// ---- per-component sums: one global atomic per run of equal keys within a wave --------------------------------------------------
// Marching cubes emits faces cell by cell and vertices lattice point by lattice point, so neighbouring lanes mostly share a label.
// run = number of run heads at or before the lane (a lane is a head when its key differs from its predecessor's); after the
// log-step sweep the head lane of every run holds the run's sum.  Every lane of the wave takes part (key < 0: nothing to add).
__device__ __forceinline__ int cc_lane() { return threadIdx.x & 63; }

__device__ __forceinline__ int cc_runs(int key, bool& head) {
    const int lane = cc_lane();
    const int prev = __shfl_up(key, 1, 64);
    head = lane == 0 || prev != key;
    const unsigned long long heads = __ballot(head);
    return __popcll(heads & ((2ull << lane) - 1ull));
}

template <typename T>
__device__ __forceinline__ T cc_run_sum(T value, int run) {
    const int lane = cc_lane();
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T other = __shfl_down(value, o, 64);
        const int other_run = __shfl_down(run, o, 64);
        if (lane + o < 64 && other_run == run) value += other;
    }
    return value;
}

__global__ __launch_bounds__(256) void cc_vertex_stats_kernel(const int* __restrict__ labels, int64_t n_vertices,
                                                              unsigned long long* __restrict__ vcount) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int key = -1;
    if (v < n_vertices) {
        key = labels[v];
        if (key < 0 || key >= n_vertices) key = -1;
    }
    bool head;
    const int run = cc_runs(key, head);
    const unsigned long long n = cc_run_sum<unsigned long long>(key >= 0 ? 1ull : 0ull, run);
    if (head && key >= 0) atomicAdd(vcount + key, n);
}

__global__ __launch_bounds__(256) void cc_face_stats_kernel(const double* __restrict__ vertices, const int64_t* __restrict__ faces, int64_t n_faces,
                                                            int64_t n_vertices, const int* __restrict__ labels,
                                                            unsigned long long* __restrict__ fcount, double* __restrict__ area,
                                                            int* __restrict__ status) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int key = -1;
    double a = 0.0;
    if (t < n_faces) {
        const int64_t i = faces[3 * t], j = faces[3 * t + 1], k = faces[3 * t + 2];
        if (i < 0 || j < 0 || k < 0 || i >= n_vertices || j >= n_vertices || k >= n_vertices) {
            atomicOr(status, PSN_CC_E_INDEX);
        } else {
            key = labels[i];
            if (key < 0 || key >= n_vertices) key = -1;
            const double ax = vertices[3 * i], ay = vertices[3 * i + 1], az = vertices[3 * i + 2];
            const double abx = vertices[3 * j] - ax, aby = vertices[3 * j + 1] - ay, abz = vertices[3 * j + 2] - az;
            const double acx = vertices[3 * k] - ax, acy = vertices[3 * k + 1] - ay, acz = vertices[3 * k + 2] - az;
            const double nx = aby * acz - abz * acy, ny = abz * acx - abx * acz, nz = abx * acy - aby * acx;
            a = 0.5 * sqrt(nx * nx + ny * ny + nz * nz);
        }
    }
    bool head;
    const int run = cc_runs(key, head);
    const unsigned long long n = cc_run_sum<unsigned long long>(key >= 0 ? 1ull : 0ull, run);
    const double s = cc_run_sum<double>(key >= 0 ? a : 0.0, run);
    if (head && key >= 0) {
        atomicAdd(fcount + key, n);
        unsafeAtomicAdd(area + key, s);   // (the hardware float64 add, not a compare-and-swap loop)
    }
}

__global__ __launch_bounds__(256) void cc_flag_kernel(const int64_t* __restrict__ faces, int64_t n_faces, int64_t n_vertices,
                                                      const int* __restrict__ labels, const unsigned char* __restrict__ keep_label,
                                                      unsigned char* __restrict__ face_keep, unsigned char* __restrict__ vertex_keep) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_faces) return;
    const int64_t i = faces[3 * t], j = faces[3 * t + 1], k = faces[3 * t + 2];
    bool keep = false;
    if (i >= 0 && j >= 0 && k >= 0 && i < n_vertices && j < n_vertices && k < n_vertices) {
        const int l = labels[i];
        keep = l >= 0 && l < n_vertices && keep_label[l] != 0;
    }
    face_keep[t] = keep ? 1 : 0;
    if (keep) vertex_keep[i] = vertex_keep[j] = vertex_keep[k] = 1;   // (every writer stores the same byte)
}

template <typename N>
__global__ __launch_bounds__(256) void cc_compact_kernel(const double* __restrict__ vertices, const N* __restrict__ normals,
                                                         const int64_t* __restrict__ faces, int64_t n_faces, int64_t n_vertices,
                                                         const unsigned char* __restrict__ face_keep, const unsigned char* __restrict__ vertex_keep,
                                                         const int64_t* __restrict__ face_pos, const int64_t* __restrict__ vertex_pos,
                                                         int64_t n_out_faces, int64_t n_out_vertices, double* __restrict__ out_vertices,
                                                         N* __restrict__ out_normals, int64_t* __restrict__ out_faces) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t < n_vertices && vertex_keep[t]) {
        const int64_t at = vertex_pos[t];
        if (at >= 0 && at < n_out_vertices) {   // (a scan that does not belong to these flags must not write out of bounds)
            out_vertices[3 * at] = vertices[3 * t]; out_vertices[3 * at + 1] = vertices[3 * t + 1]; out_vertices[3 * at + 2] = vertices[3 * t + 2];
            if (normals != nullptr) {
                out_normals[3 * at] = normals[3 * t]; out_normals[3 * at + 1] = normals[3 * t + 1]; out_normals[3 * at + 2] = normals[3 * t + 2];
            }
        }
    }
    if (t < n_faces && face_keep[t]) {
        const int64_t at = face_pos[t];
        if (at >= 0 && at < n_out_faces) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int64_t v = faces[3 * t + c];
                out_faces[3 * at + c] = (v >= 0 && v < n_vertices) ? vertex_pos[v] : -1;
            }
        }
    }
}

static inline unsigned cc_blocks(int64_t n) { return (unsigned)((n + 255) / 256); }

static int cc_check_sizes(int64_t n_faces, int64_t n_vertices, const char* what) {
    PSN_CHECK_ARG(n_vertices >= 0 && n_vertices <= PSN_CC_MAX_VERTICES, "%s: n_vertices=%lld (0 .. %lld)", what, (long long)n_vertices,
                  (long long)PSN_CC_MAX_VERTICES);
    PSN_CHECK_ARG(n_faces >= 0 && n_faces <= PSN_CC_MAX_FACES, "%s: n_faces=%lld (0 .. %lld)", what, (long long)n_faces, (long long)PSN_CC_MAX_FACES);
    return PSN_OK;
}

}  // namespace psn

extern "C" int psn_cc_label(const int64_t* faces, int64_t n_faces, int64_t n_vertices, int* parent, int* labels, int* status, void* stream) {
    using namespace psn;
    if (int rc = cc_check_sizes(n_faces, n_vertices, "cc_label")) return rc;
    PSN_CHECK_ARG(status != nullptr, "cc_label: null status word");
    PSN_CHECK_ARG((faces || n_faces == 0) && ((parent && labels) || n_vertices == 0), "cc_label: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(status, 0, sizeof(int), s) != hipSuccess) {
        set_error("cc_label: hipMemsetAsync failed");
        return PSN_E_LAUNCH;
    }
    if (n_vertices == 0) {
        if (n_faces > 0) {   // every face is out of range: flagged like any other
            hipLaunchKernelGGL(cc_link_kernel, dim3(cc_blocks(n_faces)), dim3(256), 0, s, faces, n_faces, n_vertices, parent, status);
            PSN_CHECK_LAUNCH("cc_label");
        }
        return PSN_OK;
    }
    hipLaunchKernelGGL(cc_init_kernel, dim3(cc_blocks(n_vertices)), dim3(256), 0, s, parent, n_vertices);
    if (n_faces > 0) hipLaunchKernelGGL(cc_link_kernel, dim3(cc_blocks(n_faces)), dim3(256), 0, s, faces, n_faces, n_vertices, parent, status);
    hipLaunchKernelGGL(cc_flatten_kernel, dim3(cc_blocks(n_vertices)), dim3(256), 0, s, (const int*)parent, n_vertices, labels, status);
    PSN_CHECK_LAUNCH("cc_label");
    return PSN_OK;
}

extern "C" int psn_cc_stats(const double* vertices, const int64_t* faces, int64_t n_faces, int64_t n_vertices, const int* labels,
                            long long* vertex_count, long long* face_count, double* area, int* status, void* stream) {
    using namespace psn;
    if (int rc = cc_check_sizes(n_faces, n_vertices, "cc_stats")) return rc;
    PSN_CHECK_ARG(status != nullptr, "cc_stats: null status word");
    if (n_vertices == 0) return PSN_OK;
    PSN_CHECK_ARG(vertices && labels && vertex_count && face_count && area && (faces || n_faces == 0), "cc_stats: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(vertex_count, 0, sizeof(long long) * n_vertices, s) != hipSuccess ||
        hipMemsetAsync(face_count, 0, sizeof(long long) * n_vertices, s) != hipSuccess ||
        hipMemsetAsync(area, 0, sizeof(double) * n_vertices, s) != hipSuccess) {
        set_error("cc_stats: hipMemsetAsync failed");
        return PSN_E_LAUNCH;
    }
    hipLaunchKernelGGL(cc_vertex_stats_kernel, dim3(cc_blocks(n_vertices)), dim3(256), 0, s, labels, n_vertices,
                       reinterpret_cast<unsigned long long*>(vertex_count));
    if (n_faces > 0)
        hipLaunchKernelGGL(cc_face_stats_kernel, dim3(cc_blocks(n_faces)), dim3(256), 0, s, vertices, faces, n_faces, n_vertices, labels,
                           reinterpret_cast<unsigned long long*>(face_count), area, status);
    PSN_CHECK_LAUNCH("cc_stats");
    return PSN_OK;
}

extern "C" int psn_cc_flag(const int64_t* faces, int64_t n_faces, int64_t n_vertices, const int* labels, const unsigned char* keep_label,
                           unsigned char* face_keep, unsigned char* vertex_keep, void* stream) {
    using namespace psn;
    if (int rc = cc_check_sizes(n_faces, n_vertices, "cc_flag")) return rc;
    hipStream_t s = (hipStream_t)stream;
    PSN_CHECK_ARG(vertex_keep != nullptr || n_vertices == 0, "cc_flag: null pointer");
    PSN_CHECK_ARG(n_faces == 0 || (faces && face_keep && (n_vertices == 0 || (labels && keep_label))), "cc_flag: null pointer");
    if (n_vertices > 0 && hipMemsetAsync(vertex_keep, 0, n_vertices, s) != hipSuccess) {
        set_error("cc_flag: hipMemsetAsync failed");
        return PSN_E_LAUNCH;
    }
    if (n_faces == 0) return PSN_OK;
    hipLaunchKernelGGL(cc_flag_kernel, dim3(cc_blocks(n_faces)), dim3(256), 0, s, faces, n_faces, n_vertices, labels, keep_label, face_keep,
                       vertex_keep);
    PSN_CHECK_LAUNCH("cc_flag");
    return PSN_OK;
}

extern "C" int psn_cc_compact(const double* vertices, const void* normals, int normal_bytes, const int64_t* faces, int64_t n_faces,
                              int64_t n_vertices, const unsigned char* face_keep, const unsigned char* vertex_keep, const int64_t* face_pos,
                              const int64_t* vertex_pos, int64_t n_out_faces, int64_t n_out_vertices, double* out_vertices, void* out_normals,
                              int64_t* out_faces, void* stream) {
    using namespace psn;
    if (int rc = cc_check_sizes(n_faces, n_vertices, "cc_compact")) return rc;
    PSN_CHECK_ARG(n_out_faces >= 0 && n_out_faces <= n_faces && n_out_vertices >= 0 && n_out_vertices <= n_vertices,
                  "cc_compact: %lld of %lld faces, %lld of %lld vertices", (long long)n_out_faces, (long long)n_faces, (long long)n_out_vertices,
                  (long long)n_vertices);
    PSN_CHECK_ARG(normal_bytes == 0 || normal_bytes == 4 || normal_bytes == 8, "cc_compact: normal_bytes=%d (0, 4 or 8)", normal_bytes);
    PSN_CHECK_ARG((normal_bytes == 0) == (normals == nullptr) || n_vertices == 0, "cc_compact: normals and normal_bytes do not agree");
    if (n_out_vertices == 0 && n_out_faces == 0) return PSN_OK;
    PSN_CHECK_ARG(vertices && vertex_keep && vertex_pos && out_vertices && (n_out_faces == 0 || (faces && face_keep && face_pos && out_faces)) &&
                      (normals == nullptr || out_normals != nullptr),
                  "cc_compact: null pointer");
    const int64_t n = n_faces > n_vertices ? n_faces : n_vertices;
    hipStream_t s = (hipStream_t)stream;
    if (normal_bytes == 4)
        hipLaunchKernelGGL(cc_compact_kernel<float>, dim3(cc_blocks(n)), dim3(256), 0, s, vertices, (const float*)normals, faces, n_faces, n_vertices,
                           face_keep, vertex_keep, face_pos, vertex_pos, n_out_faces, n_out_vertices, out_vertices, (float*)out_normals, out_faces);
    else
        hipLaunchKernelGGL(cc_compact_kernel<double>, dim3(cc_blocks(n)), dim3(256), 0, s, vertices, (const double*)normals, faces, n_faces, n_vertices,
                           face_keep, vertex_keep, face_pos, vertex_pos, n_out_faces, n_out_vertices, out_vertices, (double*)out_normals, out_faces);
    PSN_CHECK_LAUNCH("cc_compact");
    return PSN_OK;
}
