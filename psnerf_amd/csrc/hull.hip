// Silhouette carving: dilation of object masks by a row-convex footprint, and the visual-hull test of points and of the lattice of a
// value grid.  The numpy definition is psnerf_amd/hull.py (host_dilate, host_project, host_carve_points, host_carve_grid); every float64
// operation of the projection here is the definition's, in the definition's order (-ffp-contract=off: each product and sum a separate
// operation; IEEE division), so floor(u + 0.5), floor(v + 0.5) and with them every output equal the definition's exactly.
//
//   psn_mask_dilate  two launches over bit-packed rows.
//     pack    one wave per 64-pixel word of a row: 64 consecutive bytes in, __ballot, one 8-byte word out.  Pixels beyond W take the
//             border value, so the later launch never looks at W again when it reads.
//     dilate  one wave per OUTPUT word.  out(y) = OR over dy of (row y + dy dilated horizontally by w[dy]); lane l takes dy = l - r (and
//             l + 64 - r, ... while that is <= r): it reads the three words (left, centre, right) of row y + dy -- words and rows outside
//             the image are all-border -- forms the OR of the 2 w + 1 shifts of that 192-bit window by doubling (OR with itself shifted by
//             1, 2, 4, ..., then once by the remainder: log2(2 w + 1) + 1 steps instead of 2 w + 1), and takes the 64 bits that belong to
//             the centre word.  The lanes' words are OR-reduced across the wave with six xor-shuffles; lane i then stores bit i as a byte:
//             64 consecutive bytes per wave, 256 per workgroup.  Per output pixel the work is (2 r + 1)(log2(2 r + 1) + c) / 64 word
//             operations: it grows with r log r, not with r^2.  A half-width is at most r <= PSN_HULL_MAX_RADIUS = 64, which is what
//             lets three words suffice.  The packed image (H W / 8 bytes per view) stays in the cache; its loads are strided by one row
//             between lanes, the byte loads of pack and the byte stores of dilate are consecutive.
//   psn_hull_points  one thread per point, views ascending, stop at the first view that carves.  The view table (16 doubles per view:
//             R row-major, o, K[0, 0], K[0, 2], K[1, 2], 0) is staged into LDS PSN_HULL_VIEW_CHUNK views at a time, once per workgroup
//             and chunk; the chunks are chained inside the kernel (a workgroup whose points are all settled leaves the chain), so V
//             has no upper bound.
//   psn_hull_grid    the same per lattice point, in place.  One WAVE per run of 64 consecutive z of one (x, y) line: its stores (only
//             where the point is carved) are consecutive floats, and neighbouring lanes project to neighbouring pixels, so the mask
//             bytes they read share cache lines.  The carved count: __ballot + popcount per wave, summed over the workgroup's four
//             waves in LDS, one 64-bit integer atomic per workgroup (an integer sum: the order does not matter).
// The masks are read as bytes: 20 views of 512 x 612 are 6 MB, resident in the L2, and the gather is per point whatever the packing.
// 256 threads per workgroup, 4 KB (dilate: none) of LDS, 14 - 51 VGPRs, no scratch.  Plain HIP C++ throughout.
#include "common.h"
#include <math.h>

namespace psn {

// ---------------------------------------------------------------------------------------------------------------- dilation
struct HullFootprint {
    int r;
    unsigned char w[2 * PSN_HULL_MAX_RADIUS + 1];
};

struct U192 {
    unsigned long long lo, mid, hi;   // bits 0 .. 63 (the word to the left: smaller x), 64 .. 127 (the centre), 128 .. 191
};

// a >> m, 0 <= m <= 64 (bit x of the result = bit x + m of a; zeros come in from above)
__device__ __forceinline__ U192 hull_shr(const U192& a, int m) {
    if (m == 0) return a;
    if (m == 64) return U192{a.mid, a.hi, 0ull};
    return U192{(a.lo >> m) | (a.mid << (64 - m)), (a.mid >> m) | (a.hi << (64 - m)), a.hi >> m};
}

__device__ __forceinline__ U192 hull_or(const U192& a, const U192& b) { return U192{a.lo | b.lo, a.mid | b.mid, a.hi | b.hi}; }

// The centre word of the window dilated by w (0 <= w <= 64): bit x = OR of the window's bits 64 + x - w .. 64 + x + w.
__device__ __forceinline__ unsigned long long hull_dilate_word(U192 a, int w) {
    const int n = 2 * w + 1;          // the run length
    int have = 1;                     // a = OR of the shifts 0 .. have - 1
    while (2 * have <= n) {
        a = hull_or(a, hull_shr(a, have));
        have *= 2;
    }
    if (have < n) a = hull_or(a, hull_shr(a, n - have));   // (n - have < have: the two runs overlap or touch)
    return hull_shr(a, 64 - w).lo;
}

__global__ __launch_bounds__(256) void mask_pack_kernel(const unsigned char* __restrict__ masks, int64_t n_rows, int W, int n_words,
                                                        int border, int invert, unsigned long long* __restrict__ packed) {
    const int lane = threadIdx.x & 63;
    const int64_t word = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);   // wave-uniform
    if (word >= n_rows * n_words) return;
    const int64_t row = word / n_words;
    const int x = (int)(word - row * n_words) * 64 + lane;
    int bit = border;
    if (x < W) bit = (masks[row * W + x] != 0) != (invert != 0);
    const unsigned long long bits = __ballot(bit);
    if (lane == 0) packed[word] = bits;
}

__global__ __launch_bounds__(256) void mask_dilate_kernel(const unsigned long long* __restrict__ packed, int64_t n_rows, int H, int W,
                                                          int n_words, HullFootprint fp, int border, int invert,
                                                          unsigned char* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t word = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);   // wave-uniform
    if (word >= n_rows * n_words) return;
    const int64_t row = word / n_words;
    const int wi = (int)(word - row * n_words);
    const int y = (int)(row % H);
    const unsigned long long fill = border ? ~0ull : 0ull;
    unsigned long long acc = 0ull;
    for (int i = lane; i <= 2 * fp.r; i += 64) {
        const int yy = y + i - fp.r;
        U192 a{fill, fill, fill};
        if (yy >= 0 && yy < H) {
            const unsigned long long* __restrict__ line = packed + (row + (yy - y)) * n_words;
            if (wi > 0) a.lo = line[wi - 1];
            a.mid = line[wi];
            if (wi + 1 < n_words) a.hi = line[wi + 1];
        }
        acc |= hull_dilate_word(a, (int)fp.w[i]);
    }
    unsigned int lo = (unsigned int)acc, hi = (unsigned int)(acc >> 32);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        lo |= __shfl_xor(lo, off);
        hi |= __shfl_xor(hi, off);
    }
    const int x = wi * 64 + lane;
    if (x < W) {
        const unsigned int bit = ((lane < 32 ? lo >> lane : hi >> (lane - 32)) & 1u);
        out[row * W + x] = (unsigned char)(bit ^ (invert ? 1u : 0u));
    }
}

// ---------------------------------------------------------------------------------------------------------------- carving
#define HULL_VIEW_DOUBLES 16

// One view's verdict on p: 0 = the image does not contain p, 1 = it does and the mask is set there, 2 = it does and the mask is 0.
__device__ __forceinline__ int hull_view(const double* __restrict__ T, double p0, double p1, double p2, const unsigned char* __restrict__ mask,
                                         int H, int W) {
    const double d0 = p0 - T[9], d1 = p1 - T[10], d2 = p2 - T[11];
    const double x0 = (d0 * T[0] + d1 * T[3]) + d2 * T[6];
    const double x1 = (d0 * T[1] + d1 * T[4]) + d2 * T[7];
    const double x2 = (d0 * T[2] + d1 * T[5]) + d2 * T[8];
    const double u = T[13] + T[12] * (x0 / x2);
    const double v = T[14] + T[12] * (x1 / x2);
    const double fu = floor(u + 0.5), fv = floor(v + 0.5);
    // (comparisons in double: a NaN or an infinity is outside; inside them the conversions below are exact and in range)
    if (!(x2 > 0.0 && fu >= 0.0 && fu < (double)W && fv >= 0.0 && fv < (double)H)) return 0;
    return mask[(int64_t)(int)fv * W + (int)fu] != 0 ? 1 : 2;
}

// The chain over the chunks of views for one point per thread -> carved_by (-2, -1, or the view).  Every thread of the workgroup calls
// it (barriers inside); ``live`` = this thread has a point.
__device__ __forceinline__ int hull_carve(double p0, double p1, double p2, bool live, const double* __restrict__ views, int V,
                                          const unsigned char* __restrict__ masks, int H, int W, double* table) {
    int carved_by = -2;
    bool open = live;
    for (int v0 = 0; v0 < V; v0 += PSN_HULL_VIEW_CHUNK) {
        if (!__syncthreads_or(open ? 1 : 0)) break;          // (also: the previous chunk's table is no longer read)
        const int nv = min(PSN_HULL_VIEW_CHUNK, V - v0);
        for (int i = threadIdx.x; i < nv * HULL_VIEW_DOUBLES; i += blockDim.x) table[i] = views[(int64_t)v0 * HULL_VIEW_DOUBLES + i];
        __syncthreads();
        if (open) {
            for (int k = 0; k < nv; ++k) {
                const int s = hull_view(table + k * HULL_VIEW_DOUBLES, p0, p1, p2, masks + (int64_t)(v0 + k) * H * W, H, W);
                if (s == 1) carved_by = -1;
                if (s == 2) { carved_by = v0 + k; open = false; break; }
            }
        }
    }
    return carved_by;
}

template <typename T>
__global__ __launch_bounds__(256) void hull_points_kernel(const T* __restrict__ points, int64_t Q, const double* __restrict__ views, int V,
                                                          const unsigned char* __restrict__ masks, int H, int W,
                                                          unsigned char* __restrict__ keep, int32_t* __restrict__ carved_by) {
    __shared__ double table[PSN_HULL_VIEW_CHUNK * HULL_VIEW_DOUBLES];
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = q < Q;
    double p0 = 0.0, p1 = 0.0, p2 = 0.0;
    if (live) { p0 = (double)points[3 * q]; p1 = (double)points[3 * q + 1]; p2 = (double)points[3 * q + 2]; }
    const int c = hull_carve(p0, p1, p2, live, views, V, masks, H, W, table);
    if (live) {
        keep[q] = c == -1 ? 1 : 0;
        carved_by[q] = c;
    }
}

__global__ __launch_bounds__(256) void hull_grid_kernel(float* __restrict__ grid, int n, int runs_per_line, int64_t n_runs,
                                                        const double* __restrict__ axis, const double* __restrict__ views, int V,
                                                        const unsigned char* __restrict__ masks, int H, int W, float value,
                                                        unsigned long long* __restrict__ count) {
    __shared__ double table[PSN_HULL_VIEW_CHUNK * HULL_VIEW_DOUBLES];
    __shared__ int carved_in_wave[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t run = (int64_t)blockIdx.x * 4 + wave;                 // wave-uniform
    const int64_t line = run / runs_per_line;                           // x n + y
    const int z = (int)(run - line * runs_per_line) * 64 + lane;
    const bool live = run < n_runs && z < n;
    double p0 = 0.0, p1 = 0.0, p2 = 0.0;
    if (live) {
        const int x = (int)(line / n);
        p0 = axis[x]; p1 = axis[(int)(line - (int64_t)x * n)]; p2 = axis[z];
    }
    const int c = hull_carve(p0, p1, p2, live, views, V, masks, H, W, table);
    const bool carved = live && c != -1;
    if (carved) grid[line * n + z] = value;
    const unsigned long long votes = __ballot(carved ? 1 : 0);
    if (lane == 0) carved_in_wave[wave] = __popcll(votes);
    __syncthreads();
    if (threadIdx.x == 0) {
        const int total = (carved_in_wave[0] + carved_in_wave[1]) + (carved_in_wave[2] + carved_in_wave[3]);
        if (total) atomicAdd(count, (unsigned long long)total);
    }
}

static int hull_check_views(const char* what, const double* views, int V, const unsigned char* masks, int H, int W) {
    PSN_CHECK_ARG(V >= 1, "%s: V=%d (at least one view)", what, V);
    PSN_CHECK_ARG(H >= 1 && W >= 1, "%s: images of H=%d x W=%d (at least 1 x 1)", what, H, W);
    PSN_CHECK_ARG(views && masks, "%s: null pointer", what);
    return PSN_OK;
}

}  // namespace psn

extern "C" int64_t psn_mask_dilate_workspace(int V, int H, int W) {
    if (V < 1 || H < 1 || W < 1) return -1;
    return (int64_t)V * H * ((W + 63) / 64);
}

extern "C" int psn_mask_dilate(const unsigned char* masks, int V, int H, int W, const int32_t* half_widths, int r, int border, int invert,
                               unsigned long long* workspace, unsigned char* out, void* stream) {
    using namespace psn;
    PSN_CHECK_ARG(V >= 1, "mask_dilate: V=%d (at least one mask)", V);
    PSN_CHECK_ARG(H >= 1 && W >= 1, "mask_dilate: images of H=%d x W=%d (at least 1 x 1)", H, W);
    PSN_CHECK_ARG(r >= 0 && r <= PSN_HULL_MAX_RADIUS, "mask_dilate: radius r=%d (0 .. %d)", r, PSN_HULL_MAX_RADIUS);
    PSN_CHECK_ARG(border == 0 || border == 1, "mask_dilate: border=%d (0 or 1)", border);
    PSN_CHECK_ARG(invert == 0 || invert == 1, "mask_dilate: invert=%d (0 or 1)", invert);
    PSN_CHECK_ARG(masks && half_widths && workspace && out, "mask_dilate: null pointer");
    HullFootprint fp;
    fp.r = r;
    for (int i = 0; i <= 2 * r; ++i) {
        PSN_CHECK_ARG(half_widths[i] >= 0, "mask_dilate: negative half-width %d at dy=%d", (int)half_widths[i], i - r);
        PSN_CHECK_ARG(half_widths[i] <= r, "mask_dilate: half-width %d at dy=%d above r=%d", (int)half_widths[i], i - r, r);
        fp.w[i] = (unsigned char)half_widths[i];
    }
    const int n_words = (W + 63) / 64;
    const int64_t n_rows = (int64_t)V * H, blocks = (n_rows * n_words + 3) / 4;
    PSN_CHECK_ARG(blocks < (1ll << 31), "mask_dilate: %lld words exceed one launch", (long long)(n_rows * n_words));
    hipLaunchKernelGGL(mask_pack_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, masks, n_rows, W, n_words, border, invert,
                       workspace);
    PSN_CHECK_LAUNCH("mask_dilate (pack)");
    hipLaunchKernelGGL(mask_dilate_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, workspace, n_rows, H, W, n_words, fp, border,
                       invert, out);
    PSN_CHECK_LAUNCH("mask_dilate");
    return PSN_OK;
}

extern "C" int psn_hull_points(const void* points, int point_type, int64_t n_points, const double* views, int V, const unsigned char* masks,
                               int H, int W, unsigned char* keep, int32_t* carved_by, void* stream) {
    using namespace psn;
    if (int rc = hull_check_views("hull_points", views, V, masks, H, W)) return rc;
    PSN_CHECK_ARG(point_type == PSN_HULL_F32 || point_type == PSN_HULL_F64, "hull_points: point_type=%d (PSN_HULL_F32, PSN_HULL_F64)", point_type);
    PSN_CHECK_ARG(n_points >= 0, "hull_points: n_points=%lld", (long long)n_points);
    if (n_points == 0) return PSN_OK;
    PSN_CHECK_ARG(points && keep && carved_by, "hull_points: null pointer");
    const int64_t blocks = (n_points + 255) / 256;
    PSN_CHECK_ARG(blocks < (1ll << 31), "hull_points: %lld points exceed one launch", (long long)n_points);
    if (point_type == PSN_HULL_F32)
        hipLaunchKernelGGL(hull_points_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const float*)points, n_points,
                           views, V, masks, H, W, keep, carved_by);
    else
        hipLaunchKernelGGL(hull_points_kernel<double>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const double*)points, n_points,
                           views, V, masks, H, W, keep, carved_by);
    PSN_CHECK_LAUNCH("hull_points");
    return PSN_OK;
}

extern "C" int psn_hull_grid(float* grid, int n, const double* axis, const double* views, int V, const unsigned char* masks, int H, int W,
                             float value, unsigned long long* count, void* stream) {
    using namespace psn;
    PSN_CHECK_ARG(n >= 2 && n <= PSN_MESH_MAX_RESOLUTION + 1, "hull_grid: n=%d points per axis (2 .. %d)", n, PSN_MESH_MAX_RESOLUTION + 1);
    if (int rc = hull_check_views("hull_grid", views, V, masks, H, W)) return rc;
    PSN_CHECK_ARG(grid && axis && count, "hull_grid: null pointer");
    const int runs_per_line = (n + 63) / 64;
    const int64_t n_runs = (int64_t)n * n * runs_per_line, blocks = (n_runs + 3) / 4;   // (at most 1025^2 x 17 / 4: far below 2^31)
    hipLaunchKernelGGL(hull_grid_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, grid, n, runs_per_line, n_runs, axis, views, V,
                       masks, H, W, value, count);
    PSN_CHECK_LAUNCH("hull_grid");
    return PSN_OK;
}
