// Calibrated photometric stereo on the device: one view's images under L known directional lights -> per pixel the normal, the
// albedo, a validity flag and the kept-light count (psn_ps_normals), the per-light intensities (psn_ps_light_intensity) and
// light_avg.py's light-averaged image (psn_ps_light_average).  The float64 numpy definition is psnerf_amd/photostereo.py:host_*;
// its module docstring states every step and every operation order, and the arithmetic here is float64 in exactly that order
// (-ffp-contract=off: every product and sum a separate operation; IEEE division and square root), so normals, albedo, validity and
// kept counts equal the definition bit for bit.
//   images [L, n_pixels, 3] uint8 (a byte u is the double u / 255.0) or float32 (converted exactly); mask bytes [n_pixels] or null.
//
// psn_ps_normals, and why it is shaped this way.  One thread per pixel, one 64-lane wave per workgroup, no barrier anywhere: a lane
// only ever touches its own pixel.
//   pass 1   g[l] = (v0 + v1) + v2 of every light, v = I / e; the lit count n_lit (g > dark) gives the trim's two ranks lo, hi.
//   pass 2   the ranking, O(L^2) comparisons per pixel and where the time goes: rank[i] = #{lit j: (g[j], j) < (g[i], i)}.  Only two
//            ranks matter: the lights of rank lo and hi - 1 bound the kept set, and a light is kept iff it is lit and
//            (g_lo, i_lo) <= (g[l], l) <= (g_hi, i_hi) in that order -- two pairs in registers instead of L flags.  PS_IB = 8 lights
//            are ranked per sweep over j, so a g[j] is read once per eight ranks; the sweep is split at the block so that its long
//            parts are one comparison and one add per rank, without a branch or an index test.
//   pass 3   A = sum l l^T and b = sum l g[l] over the kept lights in ascending index; adjugate solve; validity; normal.
//   pass 4   (valid pixels) the albedo over the kept lights, v re-formed from the images.
// Two forms of g[j] in passes 2 and 3, one result:
//   TILE     the wave's g[l][lane] tile lives in LDS (L x 64 x 8 B dynamic: 48 KB at 96 lights; lanes index consecutive pixels, so
//            the 8-byte column reads are conflict-free), an unlit light as NaN so that every comparison with it is false.
//            L <= PSN_PS_TILE_LIGHTS.
//   REFORM   g[j] is formed again from the image bytes at every use (cache hits, plus three divisions with light_int): any L.
// PSN_PS_PATH_AUTO takes TILE up to PSN_PS_TILE_LIGHTS and REFORM beyond.
//
// psn_ps_light_intensity carries no floating-point atomics: workgroup (chunk, l) adds its 2048 pixels by wave shuffles and a fixed
// 4-wave sum and writes ONE row of six partial sums (every row on every call); ps_intensity_reduce_kernel adds a light's rows in a
// fixed order and forms the quotients.  Two calls on the same input give the same bits.
#include "common.h"
#include <math.h>

namespace psn {

constexpr int PS_LANES = 64;      // pixels per workgroup of ps_normals_kernel
constexpr int PS_IB = 8;          // lights ranked per sweep
constexpr int PS_CHUNK = 2048;    // pixels per workgroup of ps_intensity_kernel (8 per thread)
constexpr int PS_K = 6;           // its partial row: sum I m per channel (3), sum m m per channel (3)

__device__ __forceinline__ double ps_load(const void* __restrict__ p, int type, int64_t i) {
    return type == PSN_IMG_U8 ? (double)reinterpret_cast<const unsigned char*>(p)[i] / 255.0 : (double)reinterpret_cast<const float*>(p)[i];
}
__device__ __forceinline__ double ps_pos(double x) { return x > 0.0 ? x : 0.0; }
// light_avg.py:64,67: (x.clip(0, 1) * 255).round().astype(uint8), half to even
__device__ __forceinline__ unsigned char ps_round_u8(double x) {
    x = x < 0.0 ? 0.0 : (x > 1.0 ? 1.0 : x);
    return (unsigned char)(int)rint(x * 255.0);
}

struct PsArgs {
    const void* images;
    const unsigned char* mask;     // null: every pixel
    const double* light_dir;       // [L, 3]
    const double* light_int;       // null or [L, 3]
    double* normal;                // [n_pixels, 3]
    double* albedo;                // [n_pixels, 3]
    unsigned char* valid;          // [n_pixels]
    int32_t* kept;                 // [n_pixels]
    int64_t n_pixels;
    double low, high, dark, cond;
    int type, L, min_lights;
};

// v[c] = I[l, p, c] / e[l, c]; -> g = (v0 + v1) + v2
__device__ __forceinline__ double ps_g(const PsArgs& A, int l, int64_t p, double (&v)[3]) {
    const int64_t e = ((int64_t)l * A.n_pixels + p) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        v[c] = ps_load(A.images, A.type, e + c);
        if (A.light_int != nullptr) v[c] = v[c] / A.light_int[l * 3 + c];
    }
    return (v[0] + v[1]) + v[2];
}

template <bool TILE>
__global__ __launch_bounds__(PS_LANES) void ps_normals_kernel(PsArgs A) {
    extern __shared__ double s_g[];   // TILE: [L][PS_LANES]
    const int lane = threadIdx.x, L = A.L;
    const int64_t p = (int64_t)blockIdx.x * PS_LANES + lane;
    if (p >= A.n_pixels) return;
    double n0 = 0.0, n1 = 0.0, n2 = 0.0, r0 = 0.0, r1 = 0.0, r2 = 0.0;
    int kept = 0;
    bool valid = false;
    if (A.mask == nullptr || A.mask[p] != 0) {
        const double quiet = __builtin_nan("");
        double v[3];
        // g of light l with an unlit light as NaN
        auto G = [&](int l) -> double {
            if constexpr (TILE) {
                return s_g[l * PS_LANES + lane];
            } else {
                double w[3];
                const double g = ps_g(A, l, p, w);
                return g > A.dark ? g : quiet;
            }
        };
        int n_lit = 0;
        for (int l = 0; l < L; ++l) {
            const double g = ps_g(A, l, p, v);
            const bool lit = g > A.dark;
            n_lit += lit ? 1 : 0;
            if constexpr (TILE) s_g[l * PS_LANES + lane] = lit ? g : quiet;
        }
        const int lo = (int)floor(A.low * (double)n_lit), hi = n_lit - (int)floor(A.high * (double)n_lit);
        kept = hi > lo ? hi - lo : 0;
        if (kept >= A.min_lights) {
            double g_lo = 0.0, g_hi = 0.0;
            int i_lo = -1, i_hi = -1;
            for (int i0 = 0; i0 < L; i0 += PS_IB) {
                double gi[PS_IB];
                int rank[PS_IB];
#pragma unroll
                for (int k = 0; k < PS_IB; ++k) {
                    gi[k] = i0 + k < L ? G(i0 + k) : quiet;
                    rank[k] = 0;
                }
                // before the block a tie counts (j < i), inside it by position, after it not: no index test in the long loops, and
                // (a NaN, an unlit light, compares false everywhere) no branch
#pragma unroll 4
                for (int j = 0; j < i0; ++j) {
                    const double gj = G(j);
#pragma unroll
                    for (int k = 0; k < PS_IB; ++k) rank[k] += gj <= gi[k] ? 1 : 0;
                }
#pragma unroll
                for (int q = 0; q < PS_IB; ++q) {
#pragma unroll
                    for (int k = 0; k < PS_IB; ++k) rank[k] += (q < k ? gi[q] <= gi[k] : gi[q] < gi[k]) ? 1 : 0;
                }
#pragma unroll 4
                for (int j = i0 + PS_IB; j < L; ++j) {
                    const double gj = G(j);
#pragma unroll
                    for (int k = 0; k < PS_IB; ++k) rank[k] += gj < gi[k] ? 1 : 0;
                }
#pragma unroll
                for (int k = 0; k < PS_IB; ++k) {
                    if (gi[k] == gi[k]) {
                        if (rank[k] == lo) { g_lo = gi[k]; i_lo = i0 + k; }
                        if (rank[k] == hi - 1) { g_hi = gi[k]; i_hi = i0 + k; }
                    }
                }
            }
            auto is_kept = [&](double g, int l) -> bool {
                return (g > g_lo || (g == g_lo && l >= i_lo)) && (g < g_hi || (g == g_hi && l <= i_hi));
            };
            double a00 = 0.0, a01 = 0.0, a02 = 0.0, a11 = 0.0, a12 = 0.0, a22 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0;
            for (int l = 0; l < L; ++l) {
                const double g = G(l);
                if (is_kept(g, l)) {
                    const double lx = A.light_dir[l * 3], ly = A.light_dir[l * 3 + 1], lz = A.light_dir[l * 3 + 2];
                    a00 = a00 + lx * lx; a01 = a01 + lx * ly; a02 = a02 + lx * lz;
                    a11 = a11 + ly * ly; a12 = a12 + ly * lz; a22 = a22 + lz * lz;
                    b0 = b0 + lx * g; b1 = b1 + ly * g; b2 = b2 + lz * g;
                }
            }
            const double c00 = a11 * a22 - a12 * a12, c01 = a02 * a12 - a01 * a22, c02 = a01 * a12 - a02 * a11;
            const double c11 = a00 * a22 - a02 * a02, c12 = a01 * a02 - a00 * a12, c22 = a00 * a11 - a01 * a01;
            const double det = (a00 * c00 + a01 * c01) + a02 * c02;
            const double m0 = (c00 * b0 + c01 * b1) + c02 * b2;
            const double m1 = (c01 * b0 + c11 * b1) + c12 * b2;
            const double m2 = (c02 * b0 + c12 * b1) + c22 * b2;
            const double t = ((a00 + a11) + a22) / 3.0;
            const double norm = sqrt((m0 * m0 + m1 * m1) + m2 * m2);
            valid = det > A.cond * ((t * t) * t) && norm > 0.0;
            if (valid) {
                n0 = m0 / norm; n1 = m1 / norm; n2 = m2 / norm;
                double num0 = 0.0, num1 = 0.0, num2 = 0.0, den = 0.0;
                for (int l = 0; l < L; ++l) {
                    const double g = ps_g(A, l, p, v);
                    if (g > A.dark && is_kept(g, l)) {
                        const double lx = A.light_dir[l * 3], ly = A.light_dir[l * 3 + 1], lz = A.light_dir[l * 3 + 2];
                        const double s = ps_pos((n0 * lx + n1 * ly) + n2 * lz);
                        num0 = num0 + v[0] * s; num1 = num1 + v[1] * s; num2 = num2 + v[2] * s;
                        den = den + s * s;
                    }
                }
                if (den != 0.0) { r0 = num0 / den; r1 = num1 / den; r2 = num2 / den; }
            }
        }
    }
    A.normal[p * 3] = n0; A.normal[p * 3 + 1] = n1; A.normal[p * 3 + 2] = n2;
    A.albedo[p * 3] = r0; A.albedo[p * 3 + 1] = r1; A.albedo[p * 3 + 2] = r2;
    A.valid[p] = valid ? 1 : 0;
    A.kept[p] = kept;
}

__device__ __forceinline__ double ps_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;   // (lane 0)
}

// partial row of (chunk, light): sum of I m per channel (3), of m m per channel (3), m = albedo[p, c] * max(n_p . l, 0), over the
// valid pixels whose I[l, p, c] lies in (dark, bright)
__global__ __launch_bounds__(256) void ps_intensity_kernel(const void* __restrict__ images, int type, const double* __restrict__ normal,
                                                           const double* __restrict__ albedo, const unsigned char* __restrict__ valid,
                                                           const double* __restrict__ light_dir, int64_t n_pixels, int chunks, double dark,
                                                           double bright, double* __restrict__ partial) {
    __shared__ double s_red[4][PS_K];
    const int l = blockIdx.y;
    const double lx = light_dir[l * 3], ly = light_dir[l * 3 + 1], lz = light_dir[l * 3 + 2];
    double acc[PS_K] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int j = 0; j < PS_CHUNK / 256; ++j) {
        const int64_t p = (int64_t)blockIdx.x * PS_CHUNK + j * 256 + threadIdx.x;
        if (p < n_pixels && valid[p] != 0) {
            const double s = ps_pos((normal[p * 3] * lx + normal[p * 3 + 1] * ly) + normal[p * 3 + 2] * lz);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double I = ps_load(images, type, ((int64_t)l * n_pixels + p) * 3 + c);
                if (I > dark && I < bright) {
                    const double m = albedo[p * 3 + c] * s;
                    acc[c] += I * m;
                    acc[3 + c] += m * m;
                }
            }
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < PS_K; ++k) {
        const double v = ps_wave_sum(acc[k]);
        if (lane == 0) s_red[wave][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < PS_K)
        partial[((int64_t)l * chunks + blockIdx.x) * PS_K + threadIdx.x] =
            ((s_red[0][threadIdx.x] + s_red[1][threadIdx.x]) + s_red[2][threadIdx.x]) + s_red[3][threadIdx.x];
}

// The second, fixed-order step: sums [l, k] = the sum over the T partial rows of light l.  Thread (g, k) adds rows g, g + 32, ... in
// that order; thread k then adds the 32 group sums in order; intensity [l, c] = 0 if sums [l, 3 + c] is 0, else sums [l, c] / it.
__global__ __launch_bounds__(256) void ps_intensity_reduce_kernel(const double* __restrict__ partial, int T, double* __restrict__ sums,
                                                                  double* __restrict__ intensity) {
    __shared__ double s[32][8];
    const int l = blockIdx.x, k = threadIdx.x & 7, g = threadIdx.x >> 3;
    double acc = 0.0;
    if (k < PS_K)
        for (int t = g; t < T; t += 32) acc += partial[((int64_t)l * T + t) * PS_K + k];
    s[g][k] = acc;
    __syncthreads();
    if (threadIdx.x < PS_K) {
        double total = s[0][threadIdx.x];
        for (int i = 1; i < 32; ++i) total += s[i][threadIdx.x];
        sums[l * PS_K + threadIdx.x] = total;
        s[0][threadIdx.x] = total;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const double num = s[0][threadIdx.x], den = s[0][3 + threadIdx.x];
        intensity[l * 3 + threadIdx.x] = den == 0.0 ? 0.0 : num / den;
    }
}

// light_avg.py:58-67, one thread per pixel-channel: limg[l] = I * mask (/ relat[l, c]); the sequential sum over l, / L
__global__ __launch_bounds__(256) void ps_light_average_kernel(const void* __restrict__ images, int type, const unsigned char* __restrict__ mask,
                                                               const double* __restrict__ relat, int L, int64_t n_pixels,
                                                               double* __restrict__ mean, unsigned char* __restrict__ mean_u8,
                                                               unsigned char* __restrict__ norm_u8) {
    const int64_t n3 = n_pixels * 3, idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n3) return;
    const int64_t p = idx / 3;
    const int c = (int)(idx - p * 3);
    const double m = (mask == nullptr || mask[p] != 0) ? 1.0 : 0.0;
    double acc = 0.0;
    for (int l = 0; l < L; ++l) {
        double v = ps_load(images, type, (int64_t)l * n3 + idx) * m;
        if (relat != nullptr) v = v / relat[l * 3 + c];
        if (norm_u8 != nullptr) norm_u8[(int64_t)l * n3 + idx] = ps_round_u8(v);
        acc = l == 0 ? v : acc + v;
    }
    const double mu = acc / (double)L;
    mean[idx] = mu;
    mean_u8[idx] = ps_round_u8(mu);
}

static int ps_check_images(const char* what, const void* images, int image_type, int L, int64_t n_pixels) {
    PSN_CHECK_ARG(images != nullptr, "%s: null image pointer", what);
    PSN_CHECK_ARG(image_type == PSN_IMG_F32 || image_type == PSN_IMG_U8, "%s: image_type=%d (PSN_IMG_F32, PSN_IMG_U8)", what, image_type);
    PSN_CHECK_ARG(L >= PSN_PS_MIN_LIGHTS && L <= PSN_PS_MAX_LIGHTS, "%s: L=%d lights (%d .. %d)", what, L, PSN_PS_MIN_LIGHTS, PSN_PS_MAX_LIGHTS);
    PSN_CHECK_ARG(n_pixels >= 1 && n_pixels <= PSN_PS_MAX_PIXELS, "%s: n_pixels=%lld (1 .. %lld)", what, (long long)n_pixels,
                  (long long)PSN_PS_MAX_PIXELS);
    return PSN_OK;
}
static inline int ps_chunks(int64_t n_pixels) { return (int)((n_pixels + PS_CHUNK - 1) / PS_CHUNK); }

}  // namespace psn

// Number of doubles of psn_ps_light_intensity's partial-sum scratch: one row of six per (2048-pixel chunk, light).  -1 on a bad argument.
extern "C" int64_t psn_ps_workspace(int L, int64_t n_pixels) {
    using namespace psn;
    if (L < PSN_PS_MIN_LIGHTS || L > PSN_PS_MAX_LIGHTS || n_pixels < 1 || n_pixels > PSN_PS_MAX_PIXELS) return -1;
    return (int64_t)L * ps_chunks(n_pixels) * PS_K;
}

extern "C" int psn_ps_normals(const void* images, int image_type, const unsigned char* mask, const double* light_dir, const double* light_int,
                              int L, int64_t n_pixels, double low, double high, double dark, int min_lights, double cond, int path,
                              double* normal, double* albedo, unsigned char* valid, int32_t* kept, void* stream) {
    using namespace psn;
    if (int rc = ps_check_images("ps_normals", images, image_type, L, n_pixels)) return rc;
    PSN_CHECK_ARG(light_dir && normal && albedo && valid && kept, "ps_normals: null pointer");
    PSN_CHECK_ARG(low >= 0.0 && low < 1.0 && high >= 0.0 && high < 1.0 && low + high < 1.0,
                  "ps_normals: low=%g high=%g (both in [0, 1), low + high < 1)", low, high);
    PSN_CHECK_ARG(min_lights >= PSN_PS_MIN_LIGHTS, "ps_normals: min_lights=%d (at least %d)", min_lights, PSN_PS_MIN_LIGHTS);
    PSN_CHECK_ARG(path == PSN_PS_PATH_AUTO || path == PSN_PS_PATH_TILE || path == PSN_PS_PATH_REFORM, "ps_normals: unknown path %d", path);
    PSN_CHECK_ARG(path != PSN_PS_PATH_TILE || L <= PSN_PS_TILE_LIGHTS, "ps_normals: the LDS tile holds at most %d lights, L=%d", PSN_PS_TILE_LIGHTS, L);
    PsArgs a;
    a.images = images; a.mask = mask; a.light_dir = light_dir; a.light_int = light_int;
    a.normal = normal; a.albedo = albedo; a.valid = valid; a.kept = kept;
    a.n_pixels = n_pixels; a.low = low; a.high = high; a.dark = dark; a.cond = cond;
    a.type = image_type; a.L = L; a.min_lights = min_lights;
    const unsigned blocks = (unsigned)((n_pixels + PS_LANES - 1) / PS_LANES);
    const bool tile = path == PSN_PS_PATH_TILE || (path == PSN_PS_PATH_AUTO && L <= PSN_PS_TILE_LIGHTS);
    if (tile)
        hipLaunchKernelGGL(ps_normals_kernel<true>, dim3(blocks), dim3(PS_LANES), (size_t)L * PS_LANES * sizeof(double), (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(ps_normals_kernel<false>, dim3(blocks), dim3(PS_LANES), 0, (hipStream_t)stream, a);
    PSN_CHECK_LAUNCH("ps_normals");
    return PSN_OK;
}

extern "C" int psn_ps_light_intensity(const void* images, int image_type, const double* normal, const double* albedo, const unsigned char* valid,
                                      const double* light_dir, int L, int64_t n_pixels, double dark, double bright, double* partial,
                                      double* sums, double* intensity, void* stream) {
    using namespace psn;
    if (int rc = ps_check_images("ps_light_intensity", images, image_type, L, n_pixels)) return rc;
    PSN_CHECK_ARG(normal && albedo && valid && light_dir && partial && sums && intensity, "ps_light_intensity: null pointer");
    const int chunks = ps_chunks(n_pixels);
    hipLaunchKernelGGL(ps_intensity_kernel, dim3(chunks, L), dim3(256), 0, (hipStream_t)stream, images, image_type, normal, albedo, valid, light_dir,
                       n_pixels, chunks, dark, bright, partial);
    PSN_CHECK_LAUNCH("ps_light_intensity");
    hipLaunchKernelGGL(ps_intensity_reduce_kernel, dim3(L), dim3(256), 0, (hipStream_t)stream, (const double*)partial, chunks, sums, intensity);
    PSN_CHECK_LAUNCH("ps_light_intensity (reduce)");
    return PSN_OK;
}

extern "C" int psn_ps_light_average(const void* images, int image_type, const unsigned char* mask, const double* relat_int, int L,
                                    int64_t n_pixels, double* mean, unsigned char* mean_u8, unsigned char* norm_u8, void* stream) {
    using namespace psn;
    if (int rc = ps_check_images("ps_light_average", images, image_type, L, n_pixels)) return rc;
    PSN_CHECK_ARG(mean && mean_u8, "ps_light_average: null output pointer");
    const unsigned blocks = (unsigned)((n_pixels * 3 + 255) / 256);
    hipLaunchKernelGGL(ps_light_average_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, images, image_type, mask, relat_int, L, n_pixels,
                       mean, mean_u8, norm_u8);
    PSN_CHECK_LAUNCH("ps_light_average");
    return PSN_OK;
}
