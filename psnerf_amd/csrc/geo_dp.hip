// d loss / d p of the stage-1 geometry field (stage1/model/network.py:85-120 differentiated with respect to the query points;
// the reference gets it from autograd, e.g. extracting.py:283-310).  The two backward chains of ops.GeoFieldFused already dump
// the cotangents dZ_0 / dZ_sk of the two layers that read the positional encoding; what is left is
//     t    = dZ_0 W_0 + dZ_sk W_sk[:, d_a:]                       [n, d_pe]   (d loss / d pe through the value pass)
//     d_p  = J(p)^T t + H(p)[g_pe, d_grad]                        [n, 3]      (g_pe = d logit / d pe, d_grad = d loss / d grad)
// One launch: the contraction runs on v_mfma_f32_16x16x4_f32 with the stacked weight block resident in LDS, and the chain
// rule of the encoding is the epilogue on the accumulator registers -- t never exists in memory.
//
// Orientation.  The product is formed TRANSPOSED, t^T = W^T dz^T: A operand = W^T (from LDS), B operand = dz^T (from HBM).
//   B[k = lane >> 4][n = lane & 15] = dz[row lane & 15][k]: a lane owns one data row, and the eight k of a 32-wide k-step
//   that it feeds to eight successive MFMAs are CONTIGUOUS in its row (k = 8 (lane >> 4) + j): two 16-byte loads, every dz
//   element read once.  The A operand of MFMA j takes the same k from LDS (ds_read_b32; row stride 16 NT + 2 floats, so
//   the two 16-lane groups that share an LDS cycle -- rows 8 apart -- fall on disjoint banks).
//   D[m = 4 (lane >> 4) + i][n = lane & 15]: the lane holds 4 NT encoding columns of ITS row, so the chain rule needs
//   no transpose: each lane weighs its columns, and two xor-shuffles (16, 32) sum the four lanes of a row.
// Balance: a k-step of a wave is 8 NT MFMAs (32 cycles each) for 2 KB of dz, i.e. with NT = 3 and all four SIMDs busy about
// 10 B per cycle and CU -- under the CU's share of HBM, so the matrix pipe is the nearer limit.  Measured (tools/bench_refine.py,
// profiles/mesh_refine.json; 262,144 rows, h0 = hs = 256): 0.289 ms = 44.6 TF issued (0.28 of the fp32 MFMA peak) and 2.2 TB/s
// of operands -- neither limit is reached: with one workgroup of 8 waves per CU and one k-step of loads in flight per wave the
// launch is paced by the latency of the dz loads.  It is half the time of the composition it replaces and 2 % of the backward
// pass it closes; a deeper prefetch is the next step if it ever matters.
#include "common.h"

namespace psn {

constexpr int DP_KSTEP = 32;                 // k per step: 8 per lane group
constexpr int DP_LDS_BUDGET = 144 * 1024;    // of 160 KB; a stacked block beyond it is staged in k-chunks per row tile
constexpr int DP_MAX_THREADS = 512;

struct GeoDpArgs {
    const float* p; int64_t n; int n_freqs; float scale;
    const float* dz[2]; int64_t ld_dz[2]; int h[2]; int vec[2];   // vec: base and row stride 16-byte aligned
    const float* w[2]; int64_t ld_w[2];
    const float* g_pe; int64_t ld_g; const float* g_pe2; int64_t ld_g2; const float* d_grad;
    float* d_p;
    int kp0, ktot, kc;   // padded k of block 0 | of both blocks | rows per LDS chunk (all multiples of DP_KSTEP)
};

__device__ __forceinline__ void dp_load8(const float* rowp, int kl, int h, bool vec, float (&b)[8]) {
    if (rowp == nullptr) {
#pragma unroll
        for (int j = 0; j < 8; ++j) b[j] = 0.0f;
    } else if (vec && kl + 8 <= h) {
        const float4 lo = *reinterpret_cast<const float4*>(rowp + kl), hi = *reinterpret_cast<const float4*>(rowp + kl + 4);
        b[0] = lo.x; b[1] = lo.y; b[2] = lo.z; b[3] = lo.w; b[4] = hi.x; b[5] = hi.y; b[6] = hi.z; b[7] = hi.w;
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) b[j] = kl + j < h ? rowp[kl + j] : 0.0f;
    }
}

template <int NT>  // 16-column tiles of the encoding
__global__ __launch_bounds__(DP_MAX_THREADS) void geo_point_grad_kernel(GeoDpArgs a) {
    extern __shared__ __attribute__((aligned(16))) float dp_w[];
    constexpr int LDW = 16 * NT + 2, NC = 16 * NT;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
    const int r = lane & 15, g = lane >> 4;
    const int d_pe = 3 + 6 * a.n_freqs;
    const int64_t tile_rows = 16 * n_waves, n_tiles = (a.n + tile_rows - 1) / tile_rows;
    bool staged = false;  // workgroup-uniform
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t row = tile * tile_rows + wave * 16 + r;
        const bool live = row < a.n;
        const float* rowp[2] = {live ? a.dz[0] + row * a.ld_dz[0] : nullptr, live && a.dz[1] != nullptr ? a.dz[1] + row * a.ld_dz[1] : nullptr};
        floatx4 acc[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = floatx4{0.f, 0.f, 0.f, 0.f};
        for (int k0 = 0; k0 < a.ktot; k0 += a.kc) {
            const int kend = min(k0 + a.kc, a.ktot);
            if (!staged) {  // the whole block once per workgroup when it fits, else this chunk for this row tile
                __syncthreads();
                for (int e = threadIdx.x; e < (kend - k0) * NC; e += blockDim.x) {
                    const int kk = e / NC, c = e - kk * NC;
                    const int k = k0 + kk, b = k >= a.kp0, j = k - (b ? a.kp0 : 0);
                    dp_w[kk * LDW + c] = (j < a.h[b] && c < d_pe) ? a.w[b][(int64_t)j * a.ld_w[b] + c] : 0.0f;
                }
                __syncthreads();
                staged = a.kc >= a.ktot;
            }
            float b[8], nb[8];
            {
                const int s = k0 >= a.kp0;
                dp_load8(rowp[s], k0 - (s ? a.kp0 : 0) + 8 * g, a.h[s], a.vec[s], b);
            }
            for (int k = k0; k < kend; k += DP_KSTEP) {
                const int kn = k + DP_KSTEP;
                if (kn < kend) {  // the next step's rows are in flight under this step's MFMAs
                    const int s = kn >= a.kp0;
                    dp_load8(rowp[s], kn - (s ? a.kp0 : 0) + 8 * g, a.h[s], a.vec[s], nb);
                }
                const float* wl = dp_w + (k - k0 + 8 * g) * LDW + r;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
#pragma unroll
                    for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wl[j * LDW + 16 * t], b[j], acc[t], 0, 0, 0);
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) b[j] = nb[j];
            }
        }
        // chain rule of the encoding on the lane's 4 NT columns of its row; everything in units of s (J / s, H / s^2)
        float xs[3] = {0.f, 0.f, 0.f};
        if (live) {
#pragma unroll
            for (int c = 0; c < 3; ++c) xs[c] = a.p[row * 3 + c] * a.scale;
        }
        const bool second = a.g_pe != nullptr;
        float dj[3] = {0.f, 0.f, 0.f}, dh[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < NT; ++t) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int col = 16 * t + 4 * g + i;
                if (!live || col >= d_pe) continue;
                const float tv = acc[t][i];
                float vj, vh = 0.0f;
                int c;
                if (col < 3) {
                    c = col;
                    vj = tv;
                } else {
                    const int q = col - 3, f = q / 6, w = q - 6 * f;
                    c = w >= 3 ? w - 3 : w;
                    float sn, cs;
                    sincosf(ldexpf(c == 0 ? xs[0] : (c == 1 ? xs[1] : xs[2]), f), &sn, &cs);
                    vj = ldexpf((w >= 3 ? -sn : cs) * tv, f);
                    if (second) {
                        float gv = a.g_pe[row * a.ld_g + col];
                        if (a.g_pe2 != nullptr) gv += a.g_pe2[row * a.ld_g2 + col];
                        vh = -ldexpf((w >= 3 ? cs : sn) * gv, 2 * f);
                    }
                }
#pragma unroll
                for (int cc = 0; cc < 3; ++cc) {
                    dj[cc] += c == cc ? vj : 0.0f;
                    dh[cc] += c == cc ? vh : 0.0f;
                }
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {  // the four lanes of a row, in a fixed order
            dj[c] += __shfl_xor(dj[c], 16); dj[c] += __shfl_xor(dj[c], 32);
            dh[c] += __shfl_xor(dh[c], 16); dh[c] += __shfl_xor(dh[c], 32);
        }
        if (live && g == 0) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float v = dj[c] * a.scale;
                if (second) v += a.d_grad[row * 3 + c] * (dh[c] * (a.scale * a.scale));
                a.d_p[row * 3 + c] = v;
            }
        }
    }
}

template <int NT>
static int launch_geo_dp(const GeoDpArgs& a, int cus, void* stream) {
    static bool raised = false;
    const size_t lds_bytes = (size_t)(a.kc < a.ktot ? a.kc : a.ktot) * (16 * NT + 2) * sizeof(float);
    if (!raised) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&geo_point_grad_kernel<NT>), hipFuncAttributeMaxDynamicSharedMemorySize, DP_LDS_BUDGET);
        if (e != hipSuccess) {
            set_error("geo_point_grad: hipFuncSetAttribute failed: %s", hipGetErrorString(e));
            return PSN_E_LAUNCH;
        }
        raised = true;
    }
    // 8 waves (128 rows) per workgroup once that still gives every CU a tile, else 4: one workgroup per CU holds the weights
    const int n_waves = (a.n + 127) / 128 >= cus ? 8 : 4;
    const int64_t tiles = (a.n + 16 * n_waves - 1) / (16 * n_waves);
    const unsigned grid = (unsigned)(tiles < cus ? tiles : cus);
    hipLaunchKernelGGL(geo_point_grad_kernel<NT>, dim3(grid), dim3(64 * n_waves), lds_bytes, (hipStream_t)stream, a);
    PSN_CHECK_LAUNCH("geo_point_grad");
    return PSN_OK;
}

}  // namespace psn

extern "C" int psn_geo_point_grad(const float* p, int64_t n, int n_freqs, float scale, const float* dz0, int64_t ld_dz0, int h0,
                                  const float* w0, int64_t ld_w0, const float* dzs, int64_t ld_dzs, int hs, const float* ws,
                                  int64_t ld_ws, const float* g_pe, int64_t ld_g, const float* g_pe2, int64_t ld_g2,
                                  const float* d_grad, float* d_p, void* stream) {
    using namespace psn;
    const int d_pe = 3 + 6 * n_freqs;
    PSN_CHECK_ARG(p && dz0 && w0 && d_p, "geo_point_grad: null pointer");
    PSN_CHECK_ARG(n_freqs >= 0 && d_pe <= 64, "geo_point_grad: n_freqs=%d (3 + 6 n_freqs columns must fit 64)", n_freqs);
    PSN_CHECK_ARG(h0 >= 1 && h0 <= 512 && ld_dz0 >= h0 && ld_w0 >= d_pe, "geo_point_grad: h0=%d ld_dz0=%lld ld_w0=%lld", h0, (long long)ld_dz0,
                  (long long)ld_w0);
    PSN_CHECK_ARG((dzs == nullptr) == (ws == nullptr), "geo_point_grad: dzs and ws go together");
    PSN_CHECK_ARG(dzs == nullptr || (hs >= 1 && hs <= 512 && ld_dzs >= hs && ld_ws >= d_pe), "geo_point_grad: hs=%d ld_dzs=%lld ld_ws=%lld", hs,
                  (long long)ld_dzs, (long long)ld_ws);
    PSN_CHECK_ARG((g_pe == nullptr) == (d_grad == nullptr) && (g_pe2 == nullptr || g_pe != nullptr), "geo_point_grad: g_pe and d_grad go together, g_pe2 needs both");
    PSN_CHECK_ARG((g_pe == nullptr || ld_g >= d_pe) && (g_pe2 == nullptr || ld_g2 >= d_pe), "geo_point_grad: ld_g=%lld ld_g2=%lld", (long long)ld_g,
                  (long long)ld_g2);
    if (n <= 0) return PSN_OK;
    static int cus = 0;
    if (cus == 0) {
        int dev = 0, v = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v < 1) {
            set_error("geo_point_grad: cannot read the CU count");
            return PSN_E_LAUNCH;
        }
        cus = v;
    }
    GeoDpArgs a;
    a.p = p; a.n = n; a.n_freqs = n_freqs; a.scale = scale;
    a.dz[0] = dz0; a.ld_dz[0] = ld_dz0; a.h[0] = h0; a.w[0] = w0; a.ld_w[0] = ld_w0;
    a.dz[1] = dzs; a.ld_dz[1] = dzs ? ld_dzs : 0; a.h[1] = dzs ? hs : 0; a.w[1] = ws; a.ld_w[1] = dzs ? ld_ws : 0;
    for (int b = 0; b < 2; ++b) a.vec[b] = a.dz[b] != nullptr && (((uintptr_t)a.dz[b]) & 15) == 0 && (a.ld_dz[b] & 3) == 0;
    a.g_pe = g_pe; a.ld_g = ld_g; a.g_pe2 = g_pe2; a.ld_g2 = ld_g2; a.d_grad = d_grad; a.d_p = d_p;
    a.kp0 = (h0 + DP_KSTEP - 1) / DP_KSTEP * DP_KSTEP;
    a.ktot = a.kp0 + (a.h[1] + DP_KSTEP - 1) / DP_KSTEP * DP_KSTEP;
    const int nt = (d_pe + 15) / 16;
    const int fit = DP_LDS_BUDGET / ((16 * nt + 2) * (int)sizeof(float)) / DP_KSTEP * DP_KSTEP;
    a.kc = a.ktot <= fit ? a.ktot : fit;
    switch (nt) {
        case 1: return launch_geo_dp<1>(a, cus, stream);
        case 2: return launch_geo_dp<2>(a, cus, stream);
        case 3: return launch_geo_dp<3>(a, cus, stream);
        default: return launch_geo_dp<4>(a, cus, stream);
    }
}
