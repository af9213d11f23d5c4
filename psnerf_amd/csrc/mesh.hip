// Stage-1 mesh extraction on the device (stage1/model/extracting.py:75-206 with utils/libmise/mise.pyx and
// utils/libmcubes/marchingcubes.h:23-193): multi-resolution iso-surface refinement over an octree of voxels, the hole filling
// of its dense output, and marching cubes over the (virtually padded) value grid.
//   psn_mise_collect   mise.pyx:107-129 (query) + extracting.py:105-108: the pending grid points as a compact list
//   psn_mise_refine    mise.pyx:185-282 (subdivide_voxels / subdivide_voxel): one refinement round over all leaves
//   psn_grid_ffill     mise.pyx:143-164 (to_dense): forward fill of the holes along x, then y, then z
//   psn_mc_count       marchingcubes.h:59-72: cube index, vertex ownership and triangle count per cell
//   psn_mc_emit        marchingcubes.h:74-187 + extracting.py:175-181: vertices in world units and faces, in a defined order
// State: the value grid [n^3] float32 (n = resolution + 1 points per axis, x-major, NaN = hole), one flag byte per grid point
// (0 = no grid point yet, 1 = pending, 2 = known) and one state byte per voxel of every level < depth (0 = absent, 1 = leaf,
// 2 = split).  All of it streaming or latency-bound work: a thread per point / voxel / cell, a wave per line where a scan
// along the contiguous axis is needed.  Counters are integer atomics aggregated per wave; nothing depends on their order.
#include "common.h"
#define PSN_MC_TABLE_ATTR __device__
#include "mc_table.h"

namespace psn {

#define PSN_CHECK_SUPPORTED(cond, ...)     \
    do {                                   \
        if (!(cond)) {                     \
            psn::set_error(__VA_ARGS__);   \
            return PSN_E_UNSUPPORTED;      \
        }                                  \
    } while (0)

__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }

// linear x-major index -> (i, j, k) of an m^3 array.  Every index decomposed here is below 2^31 (PSN_MESH_MAX_RESOLUTION: at most
// 1026^3 cells), so the divisions are 32-bit ones (far fewer instructions than the expansion of a 64-bit division; the passes
// over 135 M cells were not measurably faster for it, though).
__device__ __forceinline__ void cell_coords(int64_t c, int m, int& i, int& j, int& k) {
    const unsigned int u = (unsigned int)c, um = (unsigned int)m;
    const unsigned int t = u / um;
    k = (int)(u - t * um);
    i = (int)(t / um);
    j = (int)(t - (unsigned int)i * um);
}

// inclusive prefix sum over the 64 lanes of a wave (every lane must take part)
__device__ __forceinline__ int wave_scan_incl(int v) {
    const int lane = lane_id();
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    return v;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return __shfl(v, 0, 64);
}
// exclusive prefix of v over a 256-thread block and the block total (every thread must take part)
__device__ __forceinline__ int block_scan_excl(int v, int& total) {
    __shared__ int wsum[4];
    const int incl = wave_scan_incl(v);
    const int wave = threadIdx.x >> 6;
    __syncthreads();   // (a previous use of wsum is over)
    if (lane_id() == 63) wsum[wave] = incl;
    __syncthreads();
    int base = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        if (w < wave) base += wsum[w];
        total += wsum[w];
    }
    return base + incl - v;
}

// ---- MISE -------------------------------------------------------------------------------------------------------------------
// One thread per aligned word of four flag bytes.  Pending points (1) become known (2) -- they are evaluated right after --
// and are appended to the list: rows[] = linear grid index, points[] = box_size * ((float)i / (float)R - 0.5f) per axis.
__global__ __launch_bounds__(256) void mise_collect_kernel(unsigned int* __restrict__ flag_words, int64_t n_words, int64_t n3, int n, float res_f,
                                                           float box_size, int64_t capacity, int64_t* __restrict__ rows,
                                                           float* __restrict__ points, unsigned long long* __restrict__ count) {
    const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
    unsigned int word = w < n_words ? flag_words[w] : 0u;
    int cnt = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) cnt += (((word >> (8 * b)) & 0xffu) == 1u && 4 * w + b < n3) ? 1 : 0;
    const int incl = wave_scan_incl(cnt);
    const int total = __shfl(incl, 63, 64);
    if (total == 0) return;   // wave-uniform
    unsigned long long base = 0;
    if (lane_id() == 63) base = atomicAdd(count, (unsigned long long)total);
    base = __shfl(base, 63, 64);
    if (cnt == 0) return;
    int64_t at = (int64_t)base + incl - cnt;
    unsigned int out = word;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        if (((word >> (8 * b)) & 0xffu) != 1u || 4 * w + b >= n3) continue;
        out = (out & ~(0xffu << (8 * b))) | (2u << (8 * b));
        if (at < capacity) {
            const int64_t idx = 4 * w + b;
            int i, j, k;
            cell_coords(idx, n, i, j, k);
            rows[at] = idx;
            points[3 * at + 0] = box_size * ((float)i / res_f - 0.5f);
            points[3 * at + 1] = box_size * ((float)j / res_f - 0.5f);
            points[3 * at + 2] = box_size * ((float)k / res_f - 0.5f);
        }
        ++at;
    }
    flag_words[w] = out;
}

// One thread per voxel of level `level` (m voxels per axis, edge s = 2^(depth - level) grid units).  A leaf is active iff the
// known grid points of its closed cube hold a value >= thr and a value <= thr (mise.pyx:216-219, in double); a leaf has no
// grid points in its interior, so only the shell is visited.  An active leaf is split: its children become leaves, the points
// of its half-edge lattice that are no grid points yet become pending (counted once, whoever marks them first).
__global__ __launch_bounds__(256) void mise_refine_kernel(const float* __restrict__ grid, unsigned char* __restrict__ flags,
                                                          unsigned char* __restrict__ vox, unsigned char* __restrict__ vox_child, int m, int s,
                                                          int n, double thr, unsigned long long* __restrict__ pending) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t m3 = (int64_t)m * m * m;
    int marked = 0;
    if (v < m3 && vox[v] == 1) {
        int vx, vy, vz;
        cell_coords(v, m, vx, vy, vz);
        const int x0 = vx * s, y0 = vy * s, z0 = vz * s;
        bool pos = false, neg = false;
        for (int a = 0; a <= s && !(pos && neg); ++a) {
            const bool ia = a > 0 && a < s;
            for (int b = 0; b <= s && !(pos && neg); ++b) {
                const bool ib = ia && b > 0 && b < s;
                const int64_t line = ((int64_t)(x0 + a) * n + (y0 + b)) * n + z0;
                for (int c = 0; c <= s; c += (ib && c == 0) ? s : 1) {   // interior of the cube: only c = 0 and c = s
                    if (flags[line + c] != 2) continue;
                    const double val = (double)grid[line + c];
                    pos |= val >= thr;
                    neg |= val <= thr;
                }
            }
        }
        if (pos && neg) {
            vox[v] = 2;
            if (vox_child != nullptr) {
                const int m2 = 2 * m;
#pragma unroll
                for (int c = 0; c < 8; ++c)
                    vox_child[((int64_t)(2 * vx + (c >> 2)) * m2 + (2 * vy + ((c >> 1) & 1))) * m2 + (2 * vz + (c & 1))] = 1;
            }
            const int h = s >> 1;
            for (int c = 0; c < 27; ++c) {
                const int64_t idx = ((int64_t)(x0 + (c / 9) * h) * n + (y0 + ((c / 3) % 3) * h)) * n + (z0 + (c % 3) * h);
                if (flags[idx] != 0) continue;
                const int sh = 8 * (int)(idx & 3);
                const unsigned int old = atomicOr(reinterpret_cast<unsigned int*>(flags) + (idx >> 2), 1u << sh);
                marked += ((old >> sh) & 0xffu) == 0u ? 1 : 0;
            }
        }
    }
    const int total = wave_sum(marked);
    if (lane_id() == 0 && total > 0) atomicAdd(pending, (unsigned long long)total);
}

// ---- to_dense: forward fill -------------------------------------------------------------------------------------------------
// along x (stride n^2) or y (stride n): one thread per line, consecutive threads on consecutive z
__global__ __launch_bounds__(256) void ffill_strided_kernel(float* __restrict__ grid, int n, int along_y) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t nn = (int64_t)n * n;
    if (t >= nn) return;
    const unsigned int ty = (unsigned int)t / (unsigned int)n;
    const int64_t base = along_y ? (int64_t)ty * nn + ((unsigned int)t - ty * (unsigned int)n) : t;
    const int64_t stride = along_y ? n : nn;
    float carry = grid[base];
    // eight loads in flight per thread: the stores of a batch go to addresses of that batch only, so its loads may all go first
    for (int q0 = 1; q0 < n; q0 += 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = q0 + u < n ? grid[base + (q0 + u) * stride] : 0.0f;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (q0 + u >= n) break;
            if (v[u] != v[u]) {
                if (carry == carry) grid[base + (q0 + u) * stride] = carry;   // (a hole behind a hole stays one: the next pass fills it)
            } else {
                carry = v[u];
            }
        }
    }
}
// along z (contiguous): a wave per line, 64 points at a time; every point takes the value of the last non-hole at or before it
__global__ __launch_bounds__(256) void ffill_z_kernel(float* __restrict__ grid, int n) {
    const int64_t line = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (line >= (int64_t)n * n) return;   // wave-uniform
    float* p = grid + line * n;
    const int lane = lane_id();
    float carry = __builtin_nanf("");
    for (int z0 = 0; z0 < n; z0 += 64) {
        const int z = z0 + lane;
        const bool valid = z < n;
        const float v = valid ? p[z] : __builtin_nanf("");
        int src = (v == v) ? lane : -1;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(src, o, 64);
            if (lane >= o) src = t > src ? t : src;
        }
        const float g = __shfl(v, src < 0 ? 0 : src, 64);
        const float f = src >= 0 ? g : carry;
        if (valid && v != v && f == f) p[z] = f;
        carry = __shfl(f, 63, 64);
    }
}

// ---- marching cubes ---------------------------------------------------------------------------------------------------------
// Padded lattice: N = n + 2 points per axis, value -1e6 on the outer layer (extracting.py:170-171), M = N - 1 cells per axis.
__device__ __forceinline__ double mc_value(const float* __restrict__ grid, int n, int i, int j, int k) {
    if (i < 1 || j < 1 || k < 1 || i > n || j > n || k > n) return -1e6;
    return (double)grid[((int64_t)(i - 1) * n + (j - 1)) * n + (k - 1)];
}
__device__ __forceinline__ int mc_cube_index(const float* __restrict__ grid, int n, int i, int j, int k, double thr) {
    int idx = 0;
    idx |= mc_value(grid, n, i, j, k) <= thr ? 1 : 0;
    idx |= mc_value(grid, n, i + 1, j, k) <= thr ? 2 : 0;
    idx |= mc_value(grid, n, i + 1, j + 1, k) <= thr ? 4 : 0;
    idx |= mc_value(grid, n, i, j + 1, k) <= thr ? 8 : 0;
    idx |= mc_value(grid, n, i, j, k + 1) <= thr ? 16 : 0;
    idx |= mc_value(grid, n, i + 1, j, k + 1) <= thr ? 32 : 0;
    idx |= mc_value(grid, n, i + 1, j + 1, k + 1) <= thr ? 64 : 0;
    idx |= mc_value(grid, n, i, j + 1, k + 1) <= thr ? 128 : 0;
    return idx;
}
// the lattice edge that cube edge e lies on: owning point = cell corner + (dx, dy, dz), direction = axis
__device__ static const signed char MC_EDGE_OWNER[12][4] = {{0, 0, 0, 0}, {1, 0, 0, 1}, {0, 1, 0, 0}, {0, 0, 0, 1}, {0, 0, 1, 0}, {1, 0, 1, 1},
                                                            {0, 1, 1, 0}, {0, 0, 1, 1}, {0, 0, 0, 2}, {1, 0, 0, 2}, {1, 1, 0, 2}, {0, 1, 0, 2}};

// code[c] = (which of the three lattice edges leaving the cell's lower corner along +x, +y, +z carry a vertex) | triangles << 3
__global__ __launch_bounds__(256) void mc_count_kernel(const float* __restrict__ grid, int n, double thr, int64_t n_cells,
                                                       unsigned char* __restrict__ code, int* __restrict__ block_v, int* __restrict__ block_t) {
    const int M = n + 1;
    // four runs of 256 cells per workgroup (half a million workgroups of one run each were bound by their dispatch)
    for (int r = 0; r < 4; ++r) {
        const int64_t run = (int64_t)blockIdx.x * 4 + r;
        const int64_t c = run * 256 + threadIdx.x;
        if (run * 256 >= n_cells) break;   // block-uniform
        int nv = 0, nt = 0;
        if (c < n_cells) {
            int i, j, k;
            cell_coords(c, M, i, j, k);
            const int idx = mc_cube_index(grid, n, i, j, k, thr);
            const int b0 = idx & 1;
            const int vmask = (((idx >> 1) & 1) != b0 ? 1 : 0) | (((idx >> 3) & 1) != b0 ? 2 : 0) | (((idx >> 4) & 1) != b0 ? 4 : 0);
            nv = __popc(vmask);
            nt = PSN_MC_NTRI[idx];
            code[c] = (unsigned char)(vmask | (nt << 3));
        }
        int tv, tt;
        block_scan_excl(nv, tv);
        block_scan_excl(nt, tt);
        if (threadIdx.x == 0) { block_v[run] = tv; block_t[run] = tt; }
    }
}

// vertices of the lattice edges a cell's lower corner owns, ascending by (cell, axis); the iso crossing in double as
// marchingcubes.cpp:290-297 forms it (x edges run from the upper end, :78, y and z edges from the lower, :84,:90), then
// extracting.py:175-181 (box_size > 0) or padded-lattice units (box_size <= 0)
__global__ __launch_bounds__(256) void mc_vertices_kernel(const float* __restrict__ grid, int n, double thr, int64_t n_cells,
                                                          const unsigned char* __restrict__ code, const int64_t* __restrict__ vbase,
                                                          int64_t n_vertices, double box_size, int* __restrict__ voff,
                                                          double* __restrict__ vertices) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int M = n + 1;
    const int vmask = c < n_cells ? (code[c] & 7) : 0;
    int total;
    const int64_t off = vbase[blockIdx.x] + block_scan_excl(__popc(vmask), total);
    if (vmask == 0) return;
    voff[c] = (int)off;
    int p[3];
    cell_coords(c, M, p[0], p[1], p[2]);
    const double f0 = mc_value(grid, n, p[0], p[1], p[2]);
    int r = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (!((vmask >> a) & 1)) continue;
        const double fq = mc_value(grid, n, p[0] + (a == 0), p[1] + (a == 1), p[2] + (a == 2));
        const double lo = (double)p[a], hi = (double)(p[a] + 1);
        const double x1 = a == 0 ? hi : lo, x2 = a == 0 ? lo : hi;
        const double f1 = a == 0 ? fq : f0, f2 = a == 0 ? f0 : fq;
        const double pos = (x2 - x1) * (thr - f1) / (f2 - f1) + x1;
        const int64_t at = off + r;
        ++r;
        if (at >= n_vertices) continue;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            double g = d == a ? pos : (double)p[d];
            if (box_size > 0.0) {
                g = g - 1.0;
                g = g / (double)(n - 1);
                g = box_size * (g - 0.5);
            }
            vertices[3 * at + d] = g;
        }
    }
}

// faces ascending by (cell, table order): the vertex of cube edge e is the one its owning lattice point holds for e's axis
__global__ __launch_bounds__(256) void mc_faces_kernel(const float* __restrict__ grid, int n, double thr, int64_t n_cells,
                                                       const unsigned char* __restrict__ code, const int64_t* __restrict__ tbase,
                                                       int64_t n_faces, const int* __restrict__ voff, int64_t* __restrict__ faces) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int M = n + 1;
    const int nt = c < n_cells ? (code[c] >> 3) : 0;
    int total;
    const int64_t off = tbase[blockIdx.x] + block_scan_excl(nt, total);
    if (nt == 0) return;
    int i, j, k;
    cell_coords(c, M, i, j, k);
    const int idx = mc_cube_index(grid, n, i, j, k, thr);
    for (int t = 0; t < nt; ++t) {
        if (off + t >= n_faces) break;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const int e = PSN_MC_TRI[idx][3 * t + q];
            const signed char* o = MC_EDGE_OWNER[e];
            const int64_t oc = ((int64_t)(i + o[0]) * M + (j + o[1])) * M + (k + o[2]);   // (an edge with a vertex has its owner among the cells)
            const int vm = code[oc] & 7;
            faces[3 * (off + t) + q] = (int64_t)voff[oc] + __popc(vm & ((1 << o[3]) - 1));
        }
    }
}

static inline unsigned blocks_of(int64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace psn

// The pending grid points of the refinement (flag 1) as a compact list, and their transition to known (flag 2): rows[r] = linear
// index (x-major) into the (resolution + 1)^3 grid, points[r] = box_size * ((float)i / (float)resolution - 0.5f) per axis, in
// float32 in that order (extracting.py:105-108).  count[0] = number of pending points found (set here; it may exceed capacity,
// entries behind capacity are dropped).  The order of the list is not defined.  flags: one byte per grid point, padded with zero
// bytes to a multiple of 4 and 4-byte aligned.
extern "C" int psn_mise_collect(unsigned char* flags, int resolution, float box_size, int64_t capacity, int64_t* rows, float* points,
                                long long* count, void* stream) {
    using namespace psn;
    PSN_CHECK_ARG(flags && count && capacity >= 0 && (capacity == 0 || (rows && points)), "mise_collect: null pointer");
    PSN_CHECK_ARG(resolution >= 1, "mise_collect: resolution=%d", resolution);
    PSN_CHECK_SUPPORTED(resolution <= PSN_MESH_MAX_RESOLUTION, "mise_collect: resolution %d > %d", resolution, PSN_MESH_MAX_RESOLUTION);
    PSN_CHECK_ARG(((uintptr_t)flags & 3) == 0, "mise_collect: flags must be 4-byte aligned");
    const int n = resolution + 1;
    const int64_t n3 = (int64_t)n * n * n, n_words = (n3 + 3) / 4;
    if (hipMemsetAsync(count, 0, sizeof(long long), (hipStream_t)stream) != hipSuccess) {
        set_error("mise_collect: hipMemsetAsync failed");
        return PSN_E_LAUNCH;
    }
    hipLaunchKernelGGL(mise_collect_kernel, dim3(blocks_of(n_words)), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<unsigned int*>(flags),
                       n_words, n3, n, (float)resolution, box_size, capacity, rows, points, reinterpret_cast<unsigned long long*>(count));
    PSN_CHECK_LAUNCH("mise_collect");
    return PSN_OK;
}

// One refinement round (mise.pyx:185-282) over every leaf voxel of every level < depth, finest level first (so that voxels
// created in this round are tested in the next one: the schedule is deterministic).  grid / flags as above; vox: the voxel states
// of levels 0 .. depth - 1 back to back, level l = (resolution0 << l)^3 bytes x-major (0 absent, 1 leaf, 2 split; level 0 starts
// as all leaves).  pending[0] = number of grid points that became pending in this round (set here).
extern "C" int psn_mise_refine(const float* grid, unsigned char* flags, unsigned char* vox, int resolution0, int depth, double threshold,
                               long long* pending, void* stream) {
    using namespace psn;
    PSN_CHECK_ARG(grid && flags && vox && pending, "mise_refine: null pointer");
    PSN_CHECK_ARG(resolution0 >= 1 && depth >= 1 && depth <= 16, "mise_refine: resolution0=%d depth=%d", resolution0, depth);
    PSN_CHECK_SUPPORTED(((int64_t)resolution0 << depth) <= PSN_MESH_MAX_RESOLUTION, "mise_refine: resolution %lld > %d",
                        (long long)((int64_t)resolution0 << depth), PSN_MESH_MAX_RESOLUTION);
    PSN_CHECK_ARG(((uintptr_t)flags & 3) == 0, "mise_refine: flags must be 4-byte aligned");
    const int n = (resolution0 << depth) + 1;
    if (hipMemsetAsync(pending, 0, sizeof(long long), (hipStream_t)stream) != hipSuccess) {
        set_error("mise_refine: hipMemsetAsync failed");
        return PSN_E_LAUNCH;
    }
    int64_t off[17];
    off[0] = 0;
    for (int l = 0; l < depth; ++l) {
        const int64_t m = (int64_t)resolution0 << l;
        off[l + 1] = off[l] + m * m * m;
    }
    for (int l = depth - 1; l >= 0; --l) {
        const int m = resolution0 << l;
        hipLaunchKernelGGL(mise_refine_kernel, dim3(blocks_of((int64_t)m * m * m)), dim3(256), 0, (hipStream_t)stream, grid, flags, vox + off[l],
                           l + 1 < depth ? vox + off[l + 1] : nullptr, m, 1 << (depth - l), n, threshold,
                           reinterpret_cast<unsigned long long*>(pending));
        PSN_CHECK_LAUNCH("mise_refine");
    }
    return PSN_OK;
}

// MISE.to_dense's three passes (mise.pyx:143-164) in place on grid [n, n, n] (NaN = hole): every hole takes the value of its
// predecessor along x, then along y, then along z, pass after pass -- pure copies, so the result is bit-exact.
extern "C" int psn_grid_ffill(float* grid, int n, void* stream) {
    using namespace psn;
    PSN_CHECK_ARG(grid && n >= 1, "grid_ffill: null pointer / n=%d", n);
    PSN_CHECK_SUPPORTED(n <= PSN_MESH_MAX_RESOLUTION + 1, "grid_ffill: n %d > %d", n, PSN_MESH_MAX_RESOLUTION + 1);
    const int64_t nn = (int64_t)n * n;
    hipLaunchKernelGGL(ffill_strided_kernel, dim3(blocks_of(nn)), dim3(256), 0, (hipStream_t)stream, grid, n, 0);
    hipLaunchKernelGGL(ffill_strided_kernel, dim3(blocks_of(nn)), dim3(256), 0, (hipStream_t)stream, grid, n, 1);
    hipLaunchKernelGGL(ffill_z_kernel, dim3((unsigned)((nn + 3) / 4)), dim3(256), 0, (hipStream_t)stream, grid, n);
    PSN_CHECK_LAUNCH("grid_ffill");
    return PSN_OK;
}

// Marching cubes, first pass (marchingcubes.h:59-72 on the grid padded by one layer of -1e6, extracting.py:170-171; the padding
// is virtual).  Cells: (n + 1)^3, x-major.  code[c] = bit a set iff the lattice edge from the cell's lower corner along axis a
// carries a vertex (its ends differ in `value <= threshold`), | number of triangles << 3.  block_v / block_t
// [psn_mc_blocks(n)]: vertices / triangles per run of 256 consecutive cells (the caller's exclusive scan of them is what
// psn_mc_emit takes).
extern "C" int64_t psn_mc_blocks(int n) {
    if (n < 1 || n > PSN_MESH_MAX_RESOLUTION + 1) return 0;
    const int64_t M = (int64_t)n + 1;
    return (M * M * M + 255) / 256;
}
extern "C" int psn_mc_count(const float* grid, int n, double threshold, unsigned char* code, int* block_v, int* block_t, void* stream) {
    using namespace psn;
    PSN_CHECK_ARG(grid && code && block_v && block_t, "mc_count: null pointer");
    PSN_CHECK_ARG(n >= 2, "mc_count: n=%d (at least 2 points per axis)", n);
    PSN_CHECK_SUPPORTED(n <= PSN_MESH_MAX_RESOLUTION + 1, "mc_count: n %d > %d", n, PSN_MESH_MAX_RESOLUTION + 1);
    const int64_t M = (int64_t)n + 1, n_cells = M * M * M;
    hipLaunchKernelGGL(mc_count_kernel, dim3((blocks_of(n_cells) + 3) / 4), dim3(256), 0, (hipStream_t)stream, grid, n, threshold, n_cells, code, block_v,
                       block_t);
    PSN_CHECK_LAUNCH("mc_count");
    return PSN_OK;
}

// Marching cubes, second pass (marchingcubes.h:74-187, extracting.py:175-181).  v_base / t_base [psn_mc_blocks(n)]: exclusive
// scans of psn_mc_count's block sums; n_vertices / n_faces: their totals.  vertices [n_vertices, 3] float64: the iso crossing
// x1 + (x2 - x1) (thr - f1) / (f2 - f1) in double on its lattice edge, in world units box_size * ((v - 1) / (n - 1) - 0.5)
// (box_size <= 0: in units of the padded lattice), ascending by (owning grid point x-major, axis).  faces [n_faces, 3] int64,
// ascending by (cell x-major, order of mc_table.h).  v_off: scratch, int32 [(n + 1)^3] (need not be initialised).
extern "C" int psn_mc_emit(const float* grid, int n, double threshold, const unsigned char* code, const int64_t* v_base, const int64_t* t_base,
                           int64_t n_vertices, int64_t n_faces, double box_size, int* v_off, double* vertices, int64_t* faces, void* stream) {
    using namespace psn;
    PSN_CHECK_ARG(grid && code && v_base && t_base && v_off, "mc_emit: null pointer");
    PSN_CHECK_ARG(n >= 2 && n_vertices >= 0 && n_faces >= 0, "mc_emit: n=%d n_vertices=%lld n_faces=%lld", n, (long long)n_vertices,
                  (long long)n_faces);
    PSN_CHECK_ARG((n_vertices == 0 || vertices) && (n_faces == 0 || faces), "mc_emit: null output");
    PSN_CHECK_SUPPORTED(n <= PSN_MESH_MAX_RESOLUTION + 1, "mc_emit: n %d > %d", n, PSN_MESH_MAX_RESOLUTION + 1);
    PSN_CHECK_SUPPORTED(n_vertices < ((int64_t)1 << 31), "mc_emit: %lld vertices do not fit the 32-bit vertex offsets", (long long)n_vertices);
    const int64_t M = (int64_t)n + 1, n_cells = M * M * M;
    if (n_vertices > 0) {
        hipLaunchKernelGGL(mc_vertices_kernel, dim3(blocks_of(n_cells)), dim3(256), 0, (hipStream_t)stream, grid, n, threshold, n_cells, code,
                           v_base, n_vertices, box_size, v_off, vertices);
        PSN_CHECK_LAUNCH("mc_emit (vertices)");
    }
    if (n_faces > 0) {
        hipLaunchKernelGGL(mc_faces_kernel, dim3(blocks_of(n_cells)), dim3(256), 0, (hipStream_t)stream, grid, n, threshold, n_cells, code, t_base,
                           n_faces, v_off, faces);
        PSN_CHECK_LAUNCH("mc_emit (faces)");
    }
    return PSN_OK;
}
