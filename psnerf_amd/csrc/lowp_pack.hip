// Weight and bias packers of the two reduced-precision engines (mlp_infer_bf16.hip: one bf16 plane per weight; mlp_infer_x3.hip:
// three).  An fp32 value is carried as its leading bf16 pieces, each the round-to-nearest bf16 of what the previous ones left:
// one piece is the plain bf16 rounding, three add up to the value exactly.  Layouts: include/psnerf_hip.h (psn_lowp_pack).
#include "common.h"

namespace psn {

template <int N>
__device__ __forceinline__ void lowp_split(float v, uint16_t (&p)[N]) {
    float r = v;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const __bf16 b = (__bf16)r;
        p[i] = __builtin_bit_cast(uint16_t, b);
        r -= (float)b;
    }
}

// W[rows, cols] (row-major, ldw floats per row), zero-extended, k-steps [ks0, ks0 + n_ks) -> [ks][ot][plane][lane][8] bf16:
//   lane (m = lane & 31, h = lane >> 5), element j  <-  W[32 ot + m][k],
//   k = 16 ks + 8 h + j (natural order: input block, bias columns) or
//   k = 32 (ks / 2) + 16 (ks % 2) + 8 (j / 4) + 4 h + (j % 4) (permuted: previous layer's activations).
template <int NP>
__global__ __launch_bounds__(256) void lowp_pack_kernel(const float* __restrict__ W, int64_t ldw, int rows, int cols, int permuted, int n_ot,
                                                        int ks0, int n_ks, uint16_t* __restrict__ dst) {
    const int64_t total = (int64_t)n_ks * n_ot * 512;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int j = (int)(e & 7);
        const int lane = (int)((e >> 3) & 63);
        const int64_t blk = e >> 9;  // (k-step, output tile)
        const int ot = (int)(blk % n_ot);
        const int ks = ks0 + (int)(blk / n_ot);
        const int m = lane & 31, h = lane >> 5;
        const int r = 32 * ot + m;
        const int k = permuted ? 32 * (ks >> 1) + 16 * (ks & 1) + 8 * (j >> 2) + 4 * h + (j & 3) : 16 * ks + 8 * h + j;
        float v = 0.0f;
        if (r < rows && k < cols) v = W[(int64_t)r * ldw + k];
        uint16_t p[NP];
        lowp_split(v, p);
#pragma unroll
        for (int pl = 0; pl < NP; ++pl) dst[(blk * NP + pl) * 512 + (e & 511)] = p[pl];
    }
}

// V [n, 256] fp32 -> bias k-steps [n][8 tiles][64 lanes][8] bf16 in natural K order: K slots 0 .. n_pieces - 1 (lane half 0)
// = the leading pieces of the value, every other slot 0
__global__ __launch_bounds__(256) void lowp_pack_bias_kernel(const float* __restrict__ V, int64_t n, int n_pieces, uint16_t* __restrict__ dst) {
    const int64_t total = n * 4096;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int j = (int)(e & 7);
        const int lane = (int)((e >> 3) & 63);
        const int ot = (int)((e >> 9) & 7);
        const int64_t r = e >> 12;
        const int k = 8 * (lane >> 5) + j;
        uint16_t o = 0;
        if (k < n_pieces) {
            uint16_t p[3];
            lowp_split(V[r * 256 + 32 * ot + (lane & 31)], p);
            o = p[k];
        }
        dst[e] = o;
    }
}

}  // namespace psn

extern "C" int psn_lowp_pack(const float* W, int64_t ldw, int rows, int cols, int permuted, int n_ot, int ks0, int n_ks, int n_planes,
                             uint16_t* dst, void* stream) {
    using namespace psn;
    PSN_CHECK_ARG(W && dst, "lowp_pack: null pointer");
    PSN_CHECK_ARG(n_planes == 1 || n_planes == 3, "lowp_pack: n_planes=%d", n_planes);
    PSN_CHECK_ARG((n_ot == 8 || n_ot == 1) && ks0 >= 0 && n_ks >= 1 && ks0 + n_ks <= 16, "lowp_pack: n_ot=%d ks0=%d n_ks=%d", n_ot, ks0, n_ks);
    PSN_CHECK_ARG(rows >= 1 && rows <= 32 * n_ot && cols >= 1 && cols <= 256 && ldw >= cols, "lowp_pack: %d x %d (ldw %lld) does not fit",
                  rows, cols, (long long)ldw);
    const int64_t total = (int64_t)n_ks * n_ot * 512;
    const auto kernel = n_planes == 1 ? lowp_pack_kernel<1> : lowp_pack_kernel<3>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, W, ldw, rows, cols, permuted, n_ot,
                       ks0, n_ks, dst);
    PSN_CHECK_LAUNCH("lowp_pack");
    return PSN_OK;
}

extern "C" int psn_lowp_pack_bias(const float* V, int64_t n, int n_pieces, uint16_t* dst, void* stream) {
    using namespace psn;
    PSN_CHECK_ARG(V && dst && n >= 1 && n < (1ll << 30), "lowp_pack_bias: V / dst / n=%lld", (long long)n);
    PSN_CHECK_ARG(n_pieces == 2 || n_pieces == 3, "lowp_pack_bias: n_pieces=%d", n_pieces);
    const int64_t total = n * 4096;
    const int blocks = (int)((total + 255) / 256 < 65536 ? (total + 255) / 256 : 65536);
    hipLaunchKernelGGL(lowp_pack_bias_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, V, n, n_pieces, dst);
    PSN_CHECK_LAUNCH("lowp_pack_bias");
    return PSN_OK;
}
