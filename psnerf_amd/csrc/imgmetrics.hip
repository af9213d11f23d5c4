// Image evaluation on the device: what the reference's evaluation.py computes per (view, light) image pair and per view --
// the white-background compositing under mask_pred & mask_gt, the optional least-squares intensity scale (scale_img,
// evaluation.py:15-24), PSNR over the masked pixels, SSIM (skimage.metrics.structural_similarity as stage2/utils/metrics.py:53-62
// calls it: 11-tap Gaussian, sigma 1.5, reflected border, population covariance, data range 1) and the normal MAE
// (stage2/utils/metrics.py:17-37).
//   psn_img_scale_sums   per image and channel: the masked sums of pred * gt and pred * pred, and the masked pixel count
//   psn_img_metrics      the fused pass: prologue (scale + clip, white background), SSIM map, cropped SSIM sums, masked squared error
//   psn_normal_mae       per image: the masked sum of angular errors and the count (optionally the per-pixel map)
// Arithmetic is float64 throughout (-ffp-contract=off: every product and sum rounds as in the numpy definition
// psnerf_amd/imgmetrics.py:host_*, and the filter adds its taps in the definition's order, tap 0 first, axis 0 before axis 1).
// Images are [B, H, W, 3] float32 or uint8 (a byte u is the float32 value (float)u / 255.0f, the reference's astype(float32) / 255.);
// masks are bytes [B, H, W] or [1, H, W] (one view's mask for all of its lights), or null = every pixel.
//
// The fused pass, and why it is shaped this way.  One 256-thread workgroup owns a tile of 16 x 32 pixels, all three channels.
//   load        the tile with its 5-pixel halo (26 x 42 pixels; the reflected border and the tile's overhang are resolved here, so
//               nothing later tests a border) goes to LDS once, as the float32 values the images hold + one mask byte per pixel:
//               2 x 3 x 26 x 43 x 4 B + 1.1 KB = 27.9 KB.  The prologue (widen, scale, clip, white background) is applied when a
//               value is read back: it is four operations against the 110 of the filter, and float64 copies of the inputs would
//               double the tile's footprint.
//   per channel vertical pass: 42 columns x 4 row segments = 168 threads, each reads its 14 input rows once and forms the five
//               moment planes x, y, xx, yy, xy of its 4 output rows (lanes walk columns: conflict-free 4-byte LDS reads, 8-byte
//               writes) -> 5 x 16 x 43 x 8 B = 27.5 KB of float64 planes, reused by the three channels in turn;
//               horizontal pass: 2 outputs per thread (rows r and r + 8; lanes walk columns, 8-byte reads), S formed in registers.
// LDS per workgroup 55.6 KB -> two workgroups (8 waves) per CU, what __launch_bounds__(256, 2) asks of the registers as well.  A
// 32 x 32 tile would cut the halo overhead from 2.1 to 1.7 loaded pixels per output but needs 86 KB: one workgroup per CU.  The
// kernel is bound by float64 vector arithmetic (about 250 operations per pixel and channel against 27 bytes of compulsory
// traffic), not by memory: the halo re-reads are served by L2.
//
// Reductions carry no floating-point atomics: a workgroup adds its threads' values by wave shuffles and a fixed 4-wave sum and
// writes ONE row of partial sums per tile (every row is written on every call); img_reduce_kernel then adds the rows of an image
// in a fixed order.  Two calls on the same input give the same bits in the partial rows, the outputs and the map.
#include "common.h"
#include <math.h>

namespace psn {

constexpr int IM_R = 5;                    // radius = int(3.5 * 1.5 + 0.5)
constexpr int IM_TH = 16, IM_TW = 32;      // output tile
constexpr int IM_LH = IM_TH + 2 * IM_R;    // 26 loaded rows
constexpr int IM_LW = IM_TW + 2 * IM_R;    // 42 loaded columns
constexpr int IM_K = 7;                    // partial row of the image kernels; psn_normal_mae: 2
constexpr int IM_CHUNK = 2048;             // pixels per workgroup of the two streaming kernels (8 per thread)
constexpr double IM_C1 = 1e-4, IM_C2 = 9e-4;   // (0.01 * 1)^2, (0.03 * 1)^2

// exp(-x^2 / (2 * 1.5^2)), x = -5 .. 5, divided by their sum: the float64 values numpy gives for the definition's formula
// (tests/test_imgmetrics_cpu.py compares this table with psnerf_amd.imgmetrics.WEIGHTS bit for bit)
#define IM_WEIGHTS                                                                                                     \
    {0x1.0d956b52a1d70p-10, 0x1.f1fe01ae5a5b8p-8, 0x1.26eb175d83f67p-5, 0x1.bff0fe8e98418p-4, 0x1.b43c3f52b19f2p-3, \
     0x1.106560aa892c0p-2, 0x1.b43c3f52b19f2p-3, 0x1.bff0fe8e98418p-4, 0x1.26eb175d83f67p-5, 0x1.f1fe01ae5a5b8p-8, \
     0x1.0d956b52a1d70p-10}

// scipy's 'reflect' (d c b a | a b c d | d c b a), then clamped: the clamp only ever acts on the halo of rows / columns of a tile
// that hang over the image, whose outputs are not used (n >= 11 > 2 * IM_R keeps every used index inside after one reflection)
__device__ __forceinline__ int im_reflect(int i, int n) {
    if (i < 0) i = -1 - i;
    if (i >= n) i = 2 * n - 1 - i;
    return i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
}

__device__ __forceinline__ float im_load(const void* __restrict__ p, int type, int64_t i) {
    return type == PSN_IMG_U8 ? (float)reinterpret_cast<const unsigned char*>(p)[i] / 255.0f : reinterpret_cast<const float*>(p)[i];
}

// evaluation.py:23 + :26 for the prediction: (img * scale).clip(0, 1) when a scale is given, then white outside the mask
__device__ __forceinline__ double im_pred(float v, bool inside, bool has_scale, double scale) {
    double a = (double)v;
    if (has_scale) {
        a = a * scale;
        a = a < 0.0 ? 0.0 : (a > 1.0 ? 1.0 : a);
    }
    return inside ? a : 1.0;
}
__device__ __forceinline__ double im_gt(float v, bool inside) { return inside ? (double)v : 1.0; }

__device__ __forceinline__ double im_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;   // (lane 0)
}

// K values per thread -> one row of K partial sums: lanes by shuffles, the four waves in order.  Every thread must call it.
template <int K>
__device__ __forceinline__ void im_block_row(const double (&acc)[K], double (*s_red)[K], double* __restrict__ row) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double v = im_wave_sum(acc[k]);
        if (lane == 0) s_red[wave][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < K) row[threadIdx.x] = ((s_red[0][threadIdx.x] + s_red[1][threadIdx.x]) + s_red[2][threadIdx.x]) + s_red[3][threadIdx.x];
}

struct ImArgs {
    const void* pred;
    const void* gt;
    const unsigned char* mask;   // null: every pixel
    const double* scale;         // null: no scale, no clip
    double* partial;             // [B, tiles, IM_K]
    double* map;                 // null or [B, H, W, 3]
    int type, mask_batch, H, W, tiles_x, tiles_y;
};

// partial row of a tile: sum of S over the cropped area per channel (3), masked sum of (a - b)^2 per channel (3), masked pixels (1)
__global__ __launch_bounds__(256, 2) void img_metrics_kernel(ImArgs A) {
    __shared__ float s_a[3][IM_LH][IM_LW + 1];
    __shared__ float s_b[3][IM_LH][IM_LW + 1];
    __shared__ unsigned char s_m[IM_LH][IM_LW + 2];
    __shared__ double s_p[5][IM_TH][IM_LW + 1];
    __shared__ double s_red[4][IM_K];
    constexpr double w[11] = IM_WEIGHTS;
    const int tid = threadIdx.x, b = blockIdx.z;
    const int x0 = blockIdx.x * IM_TW, y0 = blockIdx.y * IM_TH;
    const int H = A.H, W = A.W;
    const int64_t img0 = (int64_t)b * H * W, mask0 = A.mask_batch == 1 ? 0 : img0;
    const bool has_scale = A.scale != nullptr;
    const double scale = has_scale ? A.scale[b] : 1.0;

    for (int i = tid; i < IM_LH * IM_LW; i += 256) {
        const int r = i / IM_LW, q = i - r * IM_LW;
        const int64_t pix = (int64_t)im_reflect(y0 - IM_R + r, H) * W + im_reflect(x0 - IM_R + q, W);
        const int64_t e = (img0 + pix) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            s_a[c][r][q] = im_load(A.pred, A.type, e + c);
            s_b[c][r][q] = im_load(A.gt, A.type, e + c);
        }
        s_m[r][q] = A.mask == nullptr ? 1 : (A.mask[mask0 + pix] != 0);
    }
    __syncthreads();

    double acc[IM_K] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const int hx = tid & 31, hr = tid >> 5;   // horizontal pass: column, and rows hr / hr + 8
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (tid < 4 * IM_LW) {
            const int seg = tid / IM_LW, q = tid - seg * IM_LW, r0 = seg * 4;
            double x[14], y[14];
#pragma unroll
            for (int j = 0; j < 14; ++j) {
                const bool inside = s_m[r0 + j][q] != 0;
                x[j] = im_pred(s_a[c][r0 + j][q], inside, has_scale, scale);
                y[j] = im_gt(s_b[c][r0 + j][q], inside);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                double ux = w[0] * x[j], uy = w[0] * y[j], uxx = w[0] * (x[j] * x[j]), uyy = w[0] * (y[j] * y[j]), uxy = w[0] * (x[j] * y[j]);
#pragma unroll
                for (int k = 1; k < 11; ++k) {
                    const double xv = x[j + k], yv = y[j + k];
                    ux = ux + w[k] * xv;
                    uy = uy + w[k] * yv;
                    uxx = uxx + w[k] * (xv * xv);
                    uyy = uyy + w[k] * (yv * yv);
                    uxy = uxy + w[k] * (xv * yv);
                }
                s_p[0][r0 + j][q] = ux; s_p[1][r0 + j][q] = uy; s_p[2][r0 + j][q] = uxx; s_p[3][r0 + j][q] = uyy; s_p[4][r0 + j][q] = uxy;
            }
        }
        __syncthreads();
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int r = hr + 8 * h;
            double u[5];
#pragma unroll
            for (int p = 0; p < 5; ++p) {
                double s = w[0] * s_p[p][r][hx];
#pragma unroll
                for (int k = 1; k < 11; ++k) s = s + w[k] * s_p[p][r][hx + k];
                u[p] = s;
            }
            const double ux = u[0], uy = u[1];
            const double vx = u[2] - ux * ux, vy = u[3] - uy * uy, vxy = u[4] - ux * uy;
            const double a1 = 2.0 * ux * uy + IM_C1, a2 = 2.0 * vxy + IM_C2;
            const double b1 = ux * ux + uy * uy + IM_C1, b2 = vx + vy + IM_C2;
            const double S = (a1 * a2) / (b1 * b2);
            const int gy = y0 + r, gx = x0 + hx;
            if (gy < H && gx < W) {
                if (A.map != nullptr) A.map[((img0 + (int64_t)gy * W + gx)) * 3 + c] = S;
                if (gy >= IM_R && gy < H - IM_R && gx >= IM_R && gx < W - IM_R) acc[c] += S;
                if (s_m[r + IM_R][hx + IM_R] != 0) {
                    const double d = im_pred(s_a[c][r + IM_R][hx + IM_R], true, has_scale, scale) - im_gt(s_b[c][r + IM_R][hx + IM_R], true);
                    acc[3 + c] += d * d;
                    if (c == 0) acc[6] += 1.0;
                }
            }
        }
        __syncthreads();   // the planes are rewritten by the next channel
    }
    const int64_t tile = ((int64_t)b * A.tiles_y + blockIdx.y) * A.tiles_x + blockIdx.x;
    im_block_row<IM_K>(acc, s_red, A.partial + tile * IM_K);
}

// partial row of a chunk: masked sum of pred * gt per channel (3), of pred * pred per channel (3), masked pixels (1)
__global__ __launch_bounds__(256) void img_scale_sums_kernel(const void* __restrict__ pred, const void* __restrict__ gt, int type,
                                                             const unsigned char* __restrict__ mask, int mask_batch, int64_t n_pixels,
                                                             int chunks, double* __restrict__ partial) {
    __shared__ double s_red[4][IM_K];
    const int b = blockIdx.y;
    const int64_t img0 = (int64_t)b * n_pixels, mask0 = mask_batch == 1 ? 0 : img0;
    double acc[IM_K] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int j = 0; j < IM_CHUNK / 256; ++j) {
        const int64_t p = (int64_t)blockIdx.x * IM_CHUNK + j * 256 + threadIdx.x;
        if (p < n_pixels && (mask == nullptr || mask[mask0 + p] != 0)) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double xh = (double)im_load(pred, type, (img0 + p) * 3 + c), x = (double)im_load(gt, type, (img0 + p) * 3 + c);
                acc[c] += xh * x;
                acc[3 + c] += xh * xh;
            }
            acc[6] += 1.0;
        }
    }
    im_block_row<IM_K>(acc, s_red, partial + ((int64_t)b * chunks + blockIdx.x) * IM_K);
}

// partial row of a chunk: masked sum of the angular errors in degrees (1), masked pixels (1).  stage2/utils/metrics.py:17-37 in
// the order of psnerf_amd.metrics.MAE: |v| = sqrt((x^2 + y^2) + z^2), v / (|v| + 1e-5) per component, a zero vector stays zero,
// dot = (x x' + y y') + z z' clipped to [-1, 1], acos, * (180 / pi).
__global__ __launch_bounds__(256) void normal_mae_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                         const unsigned char* __restrict__ mask, int mask_batch, int normalize, int64_t n_pixels,
                                                         int chunks, double* __restrict__ partial, double* __restrict__ err_map) {
    __shared__ double s_red[4][2];
    const int b = blockIdx.y;
    const int64_t img0 = (int64_t)b * n_pixels, mask0 = mask_batch == 1 ? 0 : img0;
    double acc[2] = {0.0, 0.0};
    for (int j = 0; j < IM_CHUNK / 256; ++j) {
        const int64_t p = (int64_t)blockIdx.x * IM_CHUNK + j * 256 + threadIdx.x;
        if (p >= n_pixels) continue;
        const bool inside = mask == nullptr || mask[mask0 + p] != 0;
        if (!inside && err_map == nullptr) continue;
        const int64_t e = (img0 + p) * 3;
        double ax = (double)pred[e], ay = (double)pred[e + 1], az = (double)pred[e + 2];
        double bx = (double)gt[e], by = (double)gt[e + 1], bz = (double)gt[e + 2];
        if (normalize) {
            const double na = sqrt((ax * ax + ay * ay) + az * az), nb = sqrt((bx * bx + by * by) + bz * bz);
            const double da = na + 1e-5, db = nb + 1e-5;
            ax = ax / da; ay = ay / da; az = az / da;
            bx = bx / db; by = by / db; bz = bz / db;
            if (na == 0.0) ax = ay = az = 0.0;
            if (nb == 0.0) bx = by = bz = 0.0;
        }
        double dot = (ax * bx + ay * by) + az * bz;
        dot = dot < -1.0 ? -1.0 : (dot > 1.0 ? 1.0 : dot);
        const double err = acos(dot) * (180.0 / 3.141592653589793238462643383279502884);
        if (err_map != nullptr) err_map[img0 + p] = err;
        if (inside) {
            acc[0] += err;
            acc[1] += 1.0;
        }
    }
    im_block_row<2>(acc, s_red, partial + ((int64_t)b * chunks + blockIdx.x) * 2);
}

// The second, fixed-order step: sums [b, k] = the sum over the T partial rows of image b.  Thread (g, k) adds rows g, g + 32, ...
// in that order; thread k then adds the 32 group sums in order.  finish = 1 (psn_img_metrics): also ssim [b] = the mean over the
// channels of (cropped sum of S / cropped pixels), psnr [b] = 100 if the masked mean square is 0 else -10 log10 of it.
__global__ __launch_bounds__(256) void img_reduce_kernel(const double* __restrict__ partial, int T, int K, double* __restrict__ sums, int finish,
                                                         double n_crop, double* __restrict__ ssim, double* __restrict__ psnr) {
    __shared__ double s[32][8];
    const int b = blockIdx.x, k = threadIdx.x & 7, g = threadIdx.x >> 3;
    double acc = 0.0;
    if (k < K)
        for (int t = g; t < T; t += 32) acc += partial[((int64_t)b * T + t) * K + k];
    s[g][k] = acc;
    __syncthreads();
    if (threadIdx.x < K) {
        double total = s[0][threadIdx.x];
        for (int i = 1; i < 32; ++i) total += s[i][threadIdx.x];
        sums[(int64_t)b * K + threadIdx.x] = total;
        s[0][threadIdx.x] = total;
    }
    __syncthreads();
    if (finish && threadIdx.x == 0) {
        ssim[b] = ((s[0][0] / n_crop + s[0][1] / n_crop) + s[0][2] / n_crop) / 3.0;
        const double mse = ((s[0][3] + s[0][4]) + s[0][5]) / (3.0 * s[0][6]);
        psnr[b] = mse == 0.0 ? 100.0 : -10.0 * log10(mse);
    }
}

static int im_check_images(const char* what, const void* pred, const void* gt, int image_type, const unsigned char* mask, int mask_batch, int B,
                           int H, int W) {
    PSN_CHECK_ARG(pred && gt, "%s: null image pointer", what);
    PSN_CHECK_ARG(image_type == PSN_IMG_F32 || image_type == PSN_IMG_U8, "%s: image_type=%d (PSN_IMG_F32, PSN_IMG_U8)", what, image_type);
    PSN_CHECK_ARG(B >= 1 && B <= 65535, "%s: B=%d (1 .. 65535)", what, B);
    PSN_CHECK_ARG(H >= PSN_IMG_MIN_EXTENT && W >= PSN_IMG_MIN_EXTENT && H <= PSN_IMG_MAX_EXTENT && W <= PSN_IMG_MAX_EXTENT,
                  "%s: image of %d x %d pixels (%d .. %d per extent: the 11-tap window must fit)", what, H, W, PSN_IMG_MIN_EXTENT,
                  PSN_IMG_MAX_EXTENT);
    PSN_CHECK_ARG(mask == nullptr || mask_batch == 1 || mask_batch == B, "%s: mask batch %d is neither 1 nor B=%d", what, mask_batch, B);
    return PSN_OK;
}
static inline int im_chunks(int64_t n_pixels) { return (int)((n_pixels + IM_CHUNK - 1) / IM_CHUNK); }
static inline int im_tiles_x(int W) { return (W + IM_TW - 1) / IM_TW; }
static inline int im_tiles_y(int H) { return (H + IM_TH - 1) / IM_TH; }

}  // namespace psn

// Number of doubles of the partial-sum scratch of one call: which = PSN_IMG_WS_SCALE_SUMS / _METRICS / _NORMAL_MAE (the latter
// with H * W = n_pixels).  -1 for an unknown ``which`` or a non-positive size.
extern "C" int64_t psn_img_workspace(int which, int B, int H, int W) {
    using namespace psn;
    if (B < 1 || H < 1 || W < 1) return -1;
    const int64_t n = (int64_t)H * W;
    switch (which) {
        case PSN_IMG_WS_SCALE_SUMS: return (int64_t)B * im_chunks(n) * IM_K;
        case PSN_IMG_WS_METRICS: return (int64_t)B * im_tiles_x(W) * im_tiles_y(H) * IM_K;
        case PSN_IMG_WS_NORMAL_MAE: return (int64_t)B * im_chunks(n) * 2;
    }
    return -1;
}

extern "C" int psn_img_scale_sums(const void* pred, const void* gt, int image_type, const unsigned char* mask, int mask_batch, int B, int H, int W,
                                  double* partial, double* sums, void* stream) {
    using namespace psn;
    if (int rc = im_check_images("img_scale_sums", pred, gt, image_type, mask, mask_batch, B, H, W)) return rc;
    PSN_CHECK_ARG(partial && sums, "img_scale_sums: null output pointer");
    const int64_t n = (int64_t)H * W;
    const int chunks = im_chunks(n);
    hipLaunchKernelGGL(img_scale_sums_kernel, dim3(chunks, B), dim3(256), 0, (hipStream_t)stream, pred, gt, image_type, mask, mask_batch, n, chunks,
                       partial);
    PSN_CHECK_LAUNCH("img_scale_sums");
    hipLaunchKernelGGL(img_reduce_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, (const double*)partial, chunks, IM_K, sums, 0, 0.0,
                       (double*)nullptr, (double*)nullptr);
    PSN_CHECK_LAUNCH("img_scale_sums (reduce)");
    return PSN_OK;
}

extern "C" int psn_img_metrics(const void* pred, const void* gt, int image_type, const unsigned char* mask, int mask_batch, const double* scale,
                               int B, int H, int W, double* partial, double* sums, double* ssim, double* psnr, double* ssim_map, void* stream) {
    using namespace psn;
    if (int rc = im_check_images("img_metrics", pred, gt, image_type, mask, mask_batch, B, H, W)) return rc;
    PSN_CHECK_ARG(partial && sums && ssim && psnr, "img_metrics: null output pointer");
    ImArgs a;
    a.pred = pred; a.gt = gt; a.mask = mask; a.scale = scale; a.partial = partial; a.map = ssim_map;
    a.type = image_type; a.mask_batch = mask_batch; a.H = H; a.W = W; a.tiles_x = im_tiles_x(W); a.tiles_y = im_tiles_y(H);
    hipLaunchKernelGGL(img_metrics_kernel, dim3(a.tiles_x, a.tiles_y, B), dim3(256), 0, (hipStream_t)stream, a);
    PSN_CHECK_LAUNCH("img_metrics");
    const double n_crop = (double)(H - 2 * IM_R) * (double)(W - 2 * IM_R);
    hipLaunchKernelGGL(img_reduce_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, (const double*)partial, a.tiles_x * a.tiles_y, IM_K, sums, 1,
                       n_crop, ssim, psnr);
    PSN_CHECK_LAUNCH("img_metrics (reduce)");
    return PSN_OK;
}

extern "C" int psn_normal_mae(const float* pred, const float* gt, const unsigned char* mask, int mask_batch, int normalize, int B, int64_t n_pixels,
                              double* partial, double* sums, double* err_map, void* stream) {
    using namespace psn;
    PSN_CHECK_ARG(pred && gt && partial && sums, "normal_mae: null pointer");
    PSN_CHECK_ARG(B >= 1 && B <= 65535, "normal_mae: B=%d (1 .. 65535)", B);
    PSN_CHECK_ARG(n_pixels >= 1 && n_pixels <= (int64_t)PSN_IMG_MAX_EXTENT * PSN_IMG_MAX_EXTENT, "normal_mae: n_pixels=%lld", (long long)n_pixels);
    PSN_CHECK_ARG(mask == nullptr || mask_batch == 1 || mask_batch == B, "normal_mae: mask batch %d is neither 1 nor B=%d", mask_batch, B);
    const int chunks = im_chunks(n_pixels);
    hipLaunchKernelGGL(normal_mae_kernel, dim3(chunks, B), dim3(256), 0, (hipStream_t)stream, pred, gt, mask, mask_batch, normalize, n_pixels, chunks,
                       partial, err_map);
    PSN_CHECK_LAUNCH("normal_mae");
    hipLaunchKernelGGL(img_reduce_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, (const double*)partial, chunks, 2, sums, 0, 0.0,
                       (double*)nullptr, (double*)nullptr);
    PSN_CHECK_LAUNCH("normal_mae (reduce)");
    return PSN_OK;
}
