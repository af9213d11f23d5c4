/*
 * psnerf_hip.h -- C ABI of libpsnerf_hip.so, the MI355X (gfx950) implementation
 * of the PS-NeRF hot path.
 *
 * The reference (ywq/psnerf) has no native boundary: its hot path is PyTorch
 * eager code under nn.Module.forward().  These entry points are what a
 * ctypes/cffi binding on the reference side would call for each torch
 * expression they replace (citations are relative to /root/reference).  All
 * pointers are DEVICE pointers to contiguous fp32 (or int32 where stated)
 * buffers owned by the caller (PyTorch's allocator in our host code); the
 * library never allocates or frees device memory and keeps no global state.
 * `stream` is a hipStream_t passed as void* (0 = default stream).  Every
 * function returns 0 on success or a negative PSN_E_* code; psn_last_error()
 * returns a thread-local description of the most recent failure.  Kernels are
 * launched asynchronously on `stream`; no function synchronises the device.
 */
#ifndef PSNERF_HIP_H
#define PSNERF_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PSN_OK 0
#define PSN_E_ARG (-1)     /* bad shape / null pointer / misaligned buffer */
#define PSN_E_LAUNCH (-2)  /* hipLaunchKernel / hipGetLastError failure */
#define PSN_E_UNSUPPORTED (-3)

const char* psn_last_error(void);
int psn_version(void);

/* ------------------------------------------------------------------------
 * Alpha composite -- stage1/model/rendering.py:196-197,214-216 (and :405-406)
 *   w_i   = alpha_i * prod_{j<i} (1 - alpha_j + 1e-6)
 *   rgb   = sum_i w_i c_i (+ 1 - acc if white_bg),   acc = sum_i w_i
 * alpha [n_rays, n_samples], rgb [n_rays, n_samples, 3] (may be NULL: acc only),
 * weights [n_rays, n_samples] (saved for backward; may be NULL),
 * rgb_out [n_rays, 3] (NULL iff rgb NULL), acc_out [n_rays].
 * n_samples <= 1024.
 * ---------------------------------------------------------------------- */
int psn_composite_fwd(const float* alpha, const float* rgb, int64_t n_rays, int n_samples, int white_bg,
                      float* weights, float* rgb_out, float* acc_out, void* stream);
/* d_rgb_out [n_rays,3], d_acc_out [n_rays] (may be NULL) -> d_alpha [n_rays,n_samples], d_rgb [n_rays,n_samples,3] */
int psn_composite_bwd(const float* alpha, const float* rgb, const float* d_rgb_out, const float* d_acc_out,
                      int64_t n_rays, int n_samples, int white_bg, float* d_alpha, float* d_rgb, void* stream);

/* ------------------------------------------------------------------------
 * Positional encodings.
 *   layout 0: stage1 PositionalEncoding (stage1/model/network.py:141-150)
 *   layout 0 is also stage2 Embedder (stage2/model/embedder.py:6-54): both are
 *   [x, sin(2^0 x), cos(2^0 x), sin(2^1 x), ...] with 3-vectors per block.
 * x [n, 3] -> out [n, out_stride] (first 3+6*n_freqs columns written, the
 * rest zero-filled up to out_stride).  `scale` multiplies x first (1/rescale).
 * ---------------------------------------------------------------------- */
int psn_pe_encode(const float* x, int64_t n, int n_freqs, float scale, float* out, int out_stride, void* stream);
/* Input table of the stage-1 appearance network, stage1/model/network.py:128-138 (infer_app: cat[p, gamma(view), normal,
 * features]; gamma from :141-150 on the normalised view direction, rendering.py:185-190): out [n, 64] row r =
 * [p (3) | v / |v| (3) | sin, cos bands of v / |v| (6 n_freqs) | normal (3) | zeros].  The 256 features are not part of the
 * table: they are the fused chain's initial activations (psn_mlp_launch act_init). */
int psn_app_input(const float* p, const float* v, const float* normal, int64_t n, int n_freqs, float* out, void* stream);

/* forward-mode: t [n,3] tangent of x -> d(encoding) [n, out_stride] = J_PE(x) t  (the transpose of
 * psn_pe_encode_bwd; needed for the backward of the gradient sweep) */
int psn_pe_encode_jvp(const float* x, const float* t, int64_t n, int n_freqs, float scale, float* out, int out_stride,
                      void* stream);
/* d_out [n, out_stride] -> d_x [n,3] (chain rule through sin/cos; x is re-read).  d_out2 (or NULL): a second gradient of
 * the encoding, row stride out2_stride, added column by column first (both may be column ranges of wider tensors). */
int psn_pe_encode_bwd(const float* x, const float* d_out, int64_t n, int n_freqs, float scale, int out_stride,
                      const float* d_out2, int out2_stride, float* d_x, void* stream);

/* Gradient of the stage-1 geometry field with respect to its query points (ops.GeoField / ops.GeoFieldFused backward,
 * slot 0), ONE launch, no [n, d_pe] intermediate in memory.  With d_pe = 3 + 6 n_freqs (<= 64) and s = scale:
 *   t [n, d_pe]  = dz0 [n, h0] w0 [h0, d_pe]  (+ dzs [n, hs] ws [hs, d_pe])      fp32 MFMA, fp32 accumulation
 *   d_p[r, c]    = sum_k J_k(p_rc) t[r, k]  (+ d_grad[r, c] sum_k H_k(p_rc) (g_pe[r, k] + g_pe2[r, k]))
 * over the encoding columns k of coordinate c: J = s | 2^f s cos | -2^f s sin and H = 0 | -(2^f s)^2 sin | -(2^f s)^2 cos
 * for the identity | sin | cos column of octave f, all at 2^f s p_rc.
 * dz0 / dzs are the cotangents of the pre-activations of layer 0 / of the skip layer, w0 / ws the EFFECTIVE weights of the
 * encoding columns of those layers (ws = the column range W_sk[:, d_a:]); every matrix is row-major with a row stride in
 * floats (column ranges of wider tensors are fine), h0 and hs are 1..512.  dzs = ws = NULL: no skip block.  g_pe = d_grad
 * = NULL: no second-order term; g_pe2 may be NULL on its own.  Each d_p element is written by one lane in a fixed order:
 * the same bits in every run.  n = 0 returns PSN_OK without a launch. */
int psn_geo_point_grad(const float* p, int64_t n, int n_freqs, float scale, const float* dz0, int64_t ld_dz0, int h0,
                       const float* w0, int64_t ld_w0, const float* dzs, int64_t ld_dzs, int hs, const float* ws,
                       int64_t ld_ws, const float* g_pe, int64_t ld_g, const float* g_pe2, int64_t ld_g2,
                       const float* d_grad, float* d_p, void* stream);

/* ------------------------------------------------------------------------
 * fp32-MFMA GEMM with fused epilogues: the torch.nn.Linear / addmm / mm calls
 * of stage1/model/network.py:85-106 and stage2/model/renderer.py:17-49 and
 * their autograd backward.
 *   C[M,N] = epi( opA(A)[M,K] * opB(B)[K,N] )
 * trans_a = 0: A is [M,K] row-major (lda);  1: A is stored [K,M] row-major.
 * trans_b = 0: B is [K,N] row-major (ldb);  1: B is stored [N,K] row-major
 *              (a torch Linear weight -> y = x W^T is trans_a=0, trans_b=1).
 * split_k > 1 (only epi NONE/ACCUM): K is cut into split_k slices, partial
 * tiles go to `workspace` (>= split_k*M*N floats) and are reduced
 * deterministically by a second kernel.
 * ----------------------------------------------------------------------  * colsum_a (trans_a only, or NULL): receives sum_k A[k, m] for m < M as a by-product of staging the A tiles -- with
 * A = dZ this is the bias gradient that accompanies the weight gradient dW = dZ^T X (nn.Linear backward), so no
 * separate pass over dZ is needed.  With split_k > 1 the workspace must hold split_k * M * (N + 1) floats.
 */
enum {
    PSN_EPI_NONE = 0,          /* C = acc                                            */
    PSN_EPI_BIAS = 1,          /* C = acc + bias[n]                                  */
    PSN_EPI_BIAS_RELU = 2,     /* C = relu(acc + bias[n])                            */
    PSN_EPI_BIAS_SOFTPLUS = 3, /* C = softplus_100(z), aux_out = sigmoid(100 z), z = acc+bias */
    PSN_EPI_MUL_AUX = 4,       /* C = acc * aux_in[m,n]                              */
    PSN_EPI_MUL_POS = 5,       /* C = acc * (aux_in[m,n] > 0)   (ReLU backward)      */
    PSN_EPI_BIAS_SIGMOID = 6,  /* C = sigmoid(acc + bias[n])                         */
    PSN_EPI_ACCUM = 7,         /* C += acc                                           */
    PSN_EPI_MUL2 = 8,          /* C = acc * aux_in,  aux_out = acc * aux_in2         */
    PSN_EPI_SOFTPLUS_BWD = 9,  /* C = s * (acc + 100 * aux_in2 * (1 - s)), s = aux_in:
                                  d/dz of softplus_100 plus the sigmoid'(100 z) term of the
                                  gradient-sweep branch (double backward of network.py:108-120) */
    PSN_EPI_MUL_AUX_RAW = 10   /* C = acc * aux_in,  aux_out = acc                   */
};
int psn_gemm(int trans_a, int trans_b, int64_t M, int N, int K, const float* A, int64_t lda, const float* B,
             int64_t ldb, float* C, int64_t ldc, const float* bias, int epilogue, const float* aux_in,
             int64_t ld_aux_in, const float* aux_in2, int64_t ld_aux_in2, float* aux_out, int64_t ld_aux_out,
             int split_k, float* workspace, float* colsum_a, void* stream);
/* What psn_gemm would launch for these arguments (M > 0): a host-only query of its dispatcher, the same function the launcher
 * calls.  No device or HIP call; a pure function of the shapes, the leading dimensions, the requested split and the operand
 * addresses, which are passed as integers (only their low four bits count, and 0 = absent for the aux operands). */
typedef struct {
    int bn;                     /* tile width in columns: 128 (gemm_kernel<.,.,2>) or 256 (gemm_kernel<.,.,4>) */
    int split_k, k_chunk;       /* slices actually launched and the rows of one (a multiple of 16) */
    int64_t tiles_m; int tiles_n;
    int64_t blocks;             /* tiles_m * tiles_n * split_k workgroups */
    int a_vec, b_vec, c_vec, auxin_vec, auxin2_vec, auxout_vec;   /* 16-byte accesses allowed per operand */
    int reduce;                 /* 0: one slice, straight to C;  1: scalar split-K reduction;  2: vector reduction */
    int nt, nt_last;            /* 16-row k-tiles of the first and of the last slice */
    int last_tile_rows;         /* rows in the last k-tile of the last slice (1..16) */
} PsnGemmPlan;
int psn_gemm_plan(int64_t M, int N, int K, int64_t a_addr, int64_t lda, int64_t b_addr, int64_t ldb, int64_t c_addr,
                  int64_t ldc, int64_t aux_in_addr, int64_t ld_aux_in, int64_t aux_in2_addr, int64_t ld_aux_in2,
                  int64_t aux_out_addr, int64_t ld_aux_out, int split_k, int64_t workspace_addr, PsnGemmPlan* plan);

/* Grouped weight gradients of one backward pass (nn.Linear backward of every layer of a network at once):
 *   C_i [M_i, N_i] (+)= A_i^T B_i (+ A2_i^T B2_i),    colsum_a_i [M_i] = column sums of A_i      for i < n_items
 * with A_i = dZ_i [K, M_i], B_i = the layer input [K, N_i] (row-major, row strides lda / ldb), all sharing K = the
 * number of rows of the pass.  One launch over all items + one reduction launch; split_k slices of K per product.
 * The optional second product covers a layer that is used twice (stage1/model/network.py:108-120: value pass and
 * gradient sweep share the weights).  n_items <= PSN_GEMM_TN_MAX_ITEMS.  workspace: sum over items of
 * n_products * split_k * M * N + split_k * M floats (+ 8 floats of padding per item). */
#define PSN_GEMM_TN_MAX_ITEMS 12
typedef struct {
    const float* A; int64_t lda;
    const float* B; int64_t ldb;
    const float* A2; int64_t lda2;   /* NULL: single product */
    const float* B2; int64_t ldb2;
    float* C; int64_t ldc;
    int M, N;
    int accumulate;                  /* 0: C = ..., 1: C += ... */
    float* colsum_a;                 /* NULL or [M] */
    int64_t b_div, b_mod;            /* b_div > 0: B is a TABLE and row k of the product reads its row (k / b_div) % b_mod
                                        (the virtual input rows of psn_mlp_launch: d W_in of a layer whose input block
                                        repeats per light or per point, summed over all K rows without expanding it) */
    const float* B_tab2; int64_t ldb_tab2;   /* optional second table (needs b_div > 0): the columns b_split .. N-1 of the */
    int64_t b2_div, b2_mod;                  /* virtual B come from B_tab2[(k / b2_div) % b2_mod, n - b_split]           */
    int b_split;                             /* multiple of 4; N = b_split + columns taken from B_tab2                    */
    int64_t k_rows;                          /* 0 = K; else this product sums over the first k_rows (<= K) rows only       */
} PsnGemmTnItem;
int psn_gemm_tn_grouped(int n_items, const PsnGemmTnItem* items, int64_t K, int split_k, float* workspace,
                        int64_t workspace_floats, void* stream);
/* What psn_gemm_tn_grouped (and _x3) would launch for these items: a host-only query of its dispatcher, the same function the
 * launcher calls, with the launcher's argument checks.  No device or HIP call: the pointers of the items are looked at as
 * integers only (low four bits, null or not) and never followed, so any integers with the right low bits will do. */
#define PSN_TN_TILE 0          /* kind: 128 x 128 tiles (gemm_tn_grouped_kernel) */
#define PSN_TN_BIG 1           /*       one 256 x 256 tile per workgroup (gemm_tn256_grouped_kernel, or the x3 kernel) */
#define PSN_TN_TALL 2          /*       one 256 x 64 tile per workgroup (gemm_tn_tall_grouped_kernel) */
#define PSN_TN_INDEX_FAST 1    /* index_path bits: some slice maps k to a table row with the float reciprocal ... */
#define PSN_TN_INDEX_DIV 2     /* ... and some slice (one that ends above 2^24) with integer division */
typedef struct {
    int split_k, k_chunk;             /* slices per product and rows per slice of the 128 x 128-tile path ... */
    int split_big, k_chunk_big;       /* ... of the 256 x 256-tile path (k-tiles of 32 rows) ... */
    int split_tall, k_chunk_tall;     /* ... and of the 256 x 64-tile path (k-tiles of 16 rows) */
    int64_t workspace_floats;         /* floats of workspace the launch needs */
    int kind[PSN_GEMM_TN_MAX_ITEMS];
    int dma[PSN_GEMM_TN_MAX_ITEMS];             /* kind BIG: operand B arrives by LDS-DMA (N == 256), else through registers */
    int splits[PSN_GEMM_TN_MAX_ITEMS];          /* workgroups per tile: slices x products */
    int live_slices[PSN_GEMM_TN_MAX_ITEMS];     /* slices that hold rows (fewer than the slices of the path under k_rows) */
    int nt[PSN_GEMM_TN_MAX_ITEMS];              /* k-tiles of a full slice (0 when only one slice holds rows) */
    int nt_last[PSN_GEMM_TN_MAX_ITEMS];         /* k-tiles of the last slice that holds rows */
    int last_tile_rows[PSN_GEMM_TN_MAX_ITEMS];  /* rows in its last k-tile */
    int b_mod[PSN_GEMM_TN_MAX_ITEMS], b2_mod[PSN_GEMM_TN_MAX_ITEMS];   /* as passed to the kernel: 0 = cannot wrap */
    int index_path[PSN_GEMM_TN_MAX_ITEMS];      /* 0 = no table, else PSN_TN_INDEX_* bits */
    int a_vec[PSN_GEMM_TN_MAX_ITEMS], b_vec[PSN_GEMM_TN_MAX_ITEMS], c_vec[PSN_GEMM_TN_MAX_ITEMS];
    int reduce_vec[PSN_GEMM_TN_MAX_ITEMS];      /* the reduction of this item takes its float4 path */
} PsnGemmTnPlan;
int psn_gemm_tn_plan(int n_items, const PsnGemmTnItem* items, int64_t K, int split_k, int64_t workspace_addr,
                     PsnGemmTnPlan* plan);
/* Partial products per multiply of the psn_gemm_tn_grouped_x3 launches that follow: 6 (default; three bf16 pieces per operand,
 * fp32-class), 3 (two pieces: hi hi + hi mid + mid hi, ~16 significant bits) or 1 (plain bf16 operands, fp32 accumulation -- the
 * "bf16 MFMA path" of BASELINE configs[4] in its literal sense).  Process-wide; returns the previous value. */
int psn_gemm_tn_x3_set_products(int n_products);
/* psn_gemm_tn_grouped with the 256 x 256-tile products (128 < M, N <= 256: the hidden-layer weight gradients of
 * stage1/model/network.py:85-106 and of the stage-2 visibility net) evaluated on the bf16 matrix pipe with split operands --
 * every fp32 element as three bf16 pieces, six partial products per multiply, fp32 accumulation ("bf16x6"): fp32-class results,
 * HBM-bound instead of MFMA-bound.  EXPERIMENT for BASELINE configs[4]'s bf16 path; every other product of the group takes the
 * exact fp32 kernels of psn_gemm_tn_grouped.  Same arguments, same workspace size. */
int psn_gemm_tn_grouped_x3(int n_items, const PsnGemmTnItem* items, int64_t K, int split_k, float* workspace,
                        int64_t workspace_floats, void* stream);

/* column sums: out[j, n] (+)= sum_m w[m, j] X[m, n] for n_w <= 4 weight columns (row_weight [M, n_w], row stride ldw), or
 * plain column sums out[n] (+)= sum_m X[m, n] with row_weight = NULL, n_w = 0 -- bias gradients, and with weights the
 * n_w x N weight gradient g^T H of a layer with few outputs.  workspace >= 2048*N floats */
int psn_colsum(const float* X, const float* row_weight, int n_w, int64_t ldw, int64_t M, int N, int64_t ldx, float* out,
               int accumulate, float* workspace, void* stream);
/* What psn_colsum would launch (host-only, as psn_gemm_plan): x_addr and workspace_addr are addresses as integers. */
typedef struct {
    int vec;            /* 1: colsum_partial_vec_kernel (N <= 256, float4 loads), 0: colsum_partial_kernel */
    int nblocks;        /* row blocks of the partial kernel (at most 2048 / max(n_w, 1)) */
    int64_t rows_per_block;
} PsnColsumPlan;
int psn_colsum_plan(int64_t x_addr, int n_w, int64_t M, int N, int64_t ldx, int64_t workspace_addr, PsnColsumPlan* plan);

/* ------------------------------------------------------------------------
 * Points along rays.  Replaces the depth-profile arithmetic of stage1/model/rendering.py:110-176 (interval
 * sampling around the surface, outer samples after iteration 5000, free-space sampling of rays that miss,
 * stratified jitter) and :431-436 (the ray-march sweep), bit-identically for the same u tables and noise.
 *   origin, dir [N,3]; dist [N] (surface depth of hit rays, NULL otherwise); far [N] (sphere exit depth)
 *   idx [n] int64: the rays of this group = rows of out [N, c0+c1, 3] that are written (NULL: rays 0..n-1)
 *   hit = 0: d = near (1 - u0) + far u0.   hit = 1: [dnp, dfp] = [max(dist - delta, near), min(dist + delta, far)]
 *   sampled with u0 (c1 == 0), or [near, dnp] with u0 followed by [dnp, dfp] with u1.
 *   u*, omu* = linspace(0, 1, c) and 1 - linspace; noise [n, c0+c1] in [0,1) or NULL (no jitter).
 * ---------------------------------------------------------------------- */
int psn_sample_points(const float* origin, const float* dir, const float* dist, const float* far, const int64_t* idx,
                      int64_t n, int hit, float near, float delta, const float* u0, const float* omu0, int c0,
                      const float* u1, const float* omu1, int c1, const float* noise, float* out, void* stream);

/* Both ray groups of a stage-1 step in one launch: ray r uses the hit profile (as hit = 1 above, with dist / delta /
 * u0 / u1) if flags[r] != 0 and the free-space profile d = near * omum + far * um over all c0 + c1 samples otherwise
 * (flags [n] bytes: the renderer's hit mask).  No index lists, hence no nonzero() / host synchronisation. */
int psn_sample_points_flagged(const float* origin, const float* dir, const float* dist, const float* far,
                              const unsigned char* flags, int64_t n, float near, float delta, const float* u0, const float* omu0,
                              int c0, const float* u1, const float* omu1, int c1, const float* um, const float* omum,
                              const float* noise, float* out, void* stream);

/* ------------------------------------------------------------------------
 * Fully fused MLP inference (activations never leave registers).  Replaces the
 * no-grad network evaluations: stage2 visibility_net over L*Ns rows
 * (stage2/model/renderer.py:191-200, vis.detach()), stage1 occupancy queries
 * in ray_marching / secant / light_visibility (stage1/model/rendering.py:
 * 456-462, 537-540, 394-399).
 *
 * Hidden width is 256, 128 or 64 (8, 4 or 2 tiles of 32; one width per network).  A network is described by
 * PsnMlpDesc; weights are pre-packed into MFMA fragment order by
 * psn_mlp_pack_layer (one call per layer, into one contiguous buffer).
 * ---------------------------------------------------------------------- */
#define PSN_MLP_MAX_LAYERS 12
/* Per-layer activation "programs" of the fused kernel.  z = accumulator; a1 / a2 = optional row-major [n_rows,256]
 * operands (mask_ptrs / aux2_ptrs); the new activation (and for some codes a second value) can be dumped row-major
 * (save_ptrs / save2_ptrs).  Forward, backward and gradient-sweep chains of stage1/model/network.py:85-120 and
 * stage2/model/renderer.py:17-49 are all sequences of these. */
enum {
    PSN_ACT_NONE = 0,
    PSN_ACT_RELU = 1,
    PSN_ACT_SOFTPLUS100 = 2,   /* act = softplus_100(z);           second = sigmoid(100 z)                  */
    PSN_ACT_RELU_MASK = 3,     /* act = z * (a1 > 0)               (ReLU backward with the saved activation) */
    PSN_ACT_MUL_AUX = 4,       /* act = z * a1;                    second = z                               */
    PSN_ACT_MUL2 = 5,          /* act = z * a1;                    second = z * a2                          */
    PSN_ACT_SOFTPLUS_BWD = 6,  /* act = a1 z + 100 (1 - a1) a2     (softplus double-backward combine)        */
    PSN_ACT_HEAD = 7,          /* side output: z is dumped, the activations are left untouched              */
    PSN_ACT_RELU_BITS = 8,     /* act = z * bit: RELU_MASK with the mask as sign bits -- a1 = [n_rows, 4] uint64 words written
                                  by psn_mlp_launch save_bits_ptrs (bit 4 mt + r of word (row, g) = feature 16 mt + 4 g + r was > 0)    */
    /* single-dump forms of the softplus chains (stage1/model/network.py:85-120): a1 = the dumped softplus OUTPUT a of the forward
       layer; s = sigmoid(100 z) = 1 - exp(-100 a) is re-formed in the kernel (a < 0, impossible for a softplus, gives s = 0) */
    PSN_ACT_MUL_AUX_A = 9,     /* act = z * s(a1);                 second = z                               */
    PSN_ACT_MUL2_A = 10,       /* act = z * s(a1);                 second = z * a2                          */
    PSN_ACT_SOFTPLUS_BWD_A = 11 /* act = s(a1) z + 100 (1 - s(a1)) a2                                        */
};
enum { PSN_OUT_NONE = 0, PSN_OUT_SIGMOID = 1, PSN_OUT_OCC = 2 /* sigmoid(-10 x), network.py:125 */ };

/* Weight-stage formats.  PSN_W_F32: fp32 fragments of v_mfma_f32_16x16x4_f32 (exact; every parity-gated path).  PSN_W_BF16X2
 * (opt-in experiment, BASELINE configs[4] "bf16 MFMA path"): the same 32 KB stage geometry [k-tile][2][16-row tile][64 lanes][16 B],
 * the two halves being the bf16 heads and the bf16 remainders (x = hi + mid + O(2^-16 x)) of the lane's eight weights of the
 * k-tile; the chain engine multiplies hi hi + hi mid + mid hi on v_mfma_f32_16x16x32_bf16 with fp32 accumulation -- the matrix
 * work of stage1/model/network.py:85-120 (value pass, gradient sweep and their adjoints) and :98-106 on the bf16 pipe,
 * activation programs, dumps and epilogues unchanged (fp32). */
enum { PSN_W_F32 = 0, PSN_W_BF16X2 = 1 };

typedef struct {
    int n_kt_in;   /* 32-wide K tiles taken from the input-feature registers (0..4) */
    int n_kt_act;  /* 32-wide K tiles taken from the previous layer's activations: 0, the hidden n_mt, or n_mt - 1 when the
                      last 32 activation columns are padding (7 of 8 behind a 217-output layer) */
    int n_mt;      /* 32-wide output tiles: 8, 4 or 2 (hidden: 256- / 128- / 64-wide network) or 1 (final) */
    int act;       /* PSN_ACT_* applied to this layer's output */
    int64_t w_off; /* float offset of this layer's packed weights */
    int64_t b_off; /* float offset of this layer's bias (n_mt*32 floats, zero padded) */
    int64_t init_off; /* >= 0: the accumulator additionally starts from init_a[ia, init_off + f] + init_b[ib, init_off + f]
                         (per-row precomputed partial products of this layer's input-feature block); -1: unused */
} PsnMlpLayer;

typedef struct {
    int n_layers; /* hidden layers + the final layer (n_out > 0); a final layer alone (n_layers == 1, n_out > 0) is refused */
    int n_out;    /* real outputs of the final layer (<= 32; <= 64 in a 256-wide chain launch: final n_mt = 2, two weight stages) */
    int out_act;  /* PSN_OUT_* */
    int in_kt_a;  /* K tiles (of 32 floats) per row of feature table A (1..4) */
    int in_kt_b;  /* K tiles per row of table B (0 = unused); in_kt_a + in_kt_b <= 4 */
    int init_stride; /* floats per row of the init tables (multiple of the hidden width), 0 if no layer uses init_off */
    int w_format; /* PSN_W_F32, or PSN_W_BF16X2 (experiment; 256-wide networks through psn_mlp_launch / psn_mlp_infer_pe* /
                     psn_march_sweep, not psn_root_find): every block with n_mt >= 2 is packed as two bf16 planes and multiplied as
                     three bf16 partial products, see PsnPackItem.format */
    PsnMlpLayer layers[PSN_MLP_MAX_LAYERS];
} PsnMlpDesc;

/* Pack W[rows, cols] (row-major, ldw floats per row; with transpose != 0 the memory holds W^T, i.e. element (r, c) sits
 * at W[c * ldw + r]), zero-extended to [n_mt*32, k_tiles*32], into `dst` (n_mt*32 * k_tiles*32 floats) in stage order.
 * A layer whose K dimension consists of several blocks (activations | input features) is packed block by block into
 * consecutive k-tile ranges of its slot. */
int psn_mlp_pack_layer(const float* W, int64_t ldw, int rows, int cols, int transpose, int n_mt, int k_tiles, float* dst,
                       void* stream);

/* The same for up to PSN_PACK_MAX_ITEMS blocks in one launch (all layers of a network after an optimiser step).
 * HOST array of items holding device pointers. */
#define PSN_PACK_MAX_ITEMS 24
typedef struct {
    const float* W;
    float* dst;
    int64_t ldw;
    int rows, cols, transpose, n_mt, k_tiles;
    int format; /* PSN_W_F32 or PSN_W_BF16X2 (same size and geometry, see above) */
} PsnPackItem;
int psn_mlp_pack_layers(int n_items, const PsnPackItem* items, void* stream);

/* The operands of one launch of the fused engine (psn_mlp_launch); {0} = nothing optional (a_div and a_mod must still be >= 1).
 * Row q of the virtual input matrix is [ A[(q / a_div) % a_mod, :] | B[(q / b_div) % b_mod, :] ]; tables are row-major with
 * strides in_kt_a*32 / in_kt_b*32 floats, 16-byte aligned.  Because a layer that reads the input block is linear in it,
 * W_in [A_row | B_row] = W_a A_row + W_b B_row can be precomputed once per table row instead of once per (A,B) pair: init_a /
 * init_b ([rows, init_stride], indexed like tab_a / tab_b; init_b may be NULL) hold those partial products and the layers with
 * init_off >= 0 start their accumulators from them (tab_a may then be NULL if no layer has n_kt_in > 0).
 * save_ptrs (HOST array of n_layers-1 device pointers, entries or the array itself may be NULL): for rows >= save_row0 the
 * post-activation output of hidden layer l is also written row-major to save_ptrs[l] [n_rows - save_row0, 256] -- the training
 * rows of stage2/model/renderer.py:251-262 ride along with the gradient-free rows and leave exactly what their backward pass needs.
 * mask_ptrs / aux2_ptrs (HOST arrays of n_layers device pointers or NULL): row-major [n_rows, 256] operands a1 / a2 of the
 * layers' activation programs; save2_ptrs: second dumps (same indexing as save_ptrs).  With n_out == 0 there is no final layer
 * and `out` may be NULL: together with transposed weight packs, an init table holding d h of the last hidden layer, masks = the
 * dumped activations and save_ptrs = the d z outputs this runs the ReLU BACKWARD chain d h_{l-1} = W_l^T (d h_l * relu'(h_l)).
 * act_init (or NULL): row-major [act_init_rows, 256] initial activations, so that layer 0 may already read them; rows >=
 * act_init_rows (1 .. n_rows) start from zeros (a gradient that exists for a row prefix only: the colour network's d features
 * when the surface-normal points ride behind the render samples, stage1/model/rendering.py:196-212).
 * rk_coef [n_rows, rk_k], rk_basis [rk_k, init_stride] (or NULL, NULL, 0; rk_k <= 4): rank-k init -- the layers with
 * init_off >= 0 additionally start from sum_c rk_coef[row, c] * rk_basis[c, init_off + f].  This is the init table of a
 * backward chain whose network has 1..4 outputs, d h = g_out W_last (stage1/model/network.py:104-106 colour head,
 * :93-95 occupancy logit; stage2/model/renderer.py:47-49), formed in registers instead of a [n_rows, 256] tensor.
 * dump_tiles (HOST array of 2 * PSN_MLP_MAX_LAYERS words, or NULL = everything): bit mt of word l / word
 * PSN_MLP_MAX_LAYERS + l set = the 16-column tile mt of layer l's first / second dump is written; for dumps of which only
 * a column range is read afterwards (the raw sweep values that feed d logit / d pe, network.py:108-120).
 * out [n_rows, n_out].
 * live_count, live_period (NULL, 0: every row is real; one without the other is refused) -- a plain forward launch (no chain
 * operands) over a PADDED row set, the stage-2 visibility rows of stage2/model/renderer.py:191-200 when the surface-pixel list has
 * a fixed capacity (psn_surface_index: one captured HIP graph serves batches with different surface counts).  The rows
 * [0, save_row0) come in groups of live_period rows (one group per shading light; live_period a multiple of 64, save_row0 a
 * multiple of live_period), of which the first live_count[0] -- a float ON THE DEVICE, psn_surface_index's count -- are real.
 * 64-row blocks that hold padding only are not evaluated: their outputs are zeros.  Every other row is evaluated exactly as
 * without a count (bit-identical), the rows from save_row0 on (the supervision rows, whose dumps a backward pass reads) all of
 * them.  The grid enumerates the evaluated blocks first, so that the skipped ones do not unbalance the XCDs.
 * save_bits_ptrs (HOST array like save_ptrs, refused without it; NULL, or NULL per layer: none) -- a plain forward launch with
 * activation dumps (stage2/model/renderer.py:251-262: the supervision rows of the visibility network, :127-143 / :163-189 the
 * normal / BRDF networks) ALSO leaves the sign bits of every dumped activation behind: save_bits_ptrs[l] [n_rows - save_row0, 4]
 * uint64.  The ReLU-backward chain (PSN_ACT_RELU_BITS, the words passed as that layer's aux1 in mask_ptrs) reads 32 bytes per row
 * and layer instead of the 1 KB activation row -- the same d z = d h * (h > 0), bit for bit. */
typedef struct {
    const float* tab_a; int64_t a_div, a_mod; const float* tab_b; int64_t b_div, b_mod; const float* init_a; const float* init_b;
    float* const* save_ptrs; unsigned long long* const* save_bits_ptrs; int64_t save_row0;
    const float* const* mask_ptrs; const float* const* aux2_ptrs; float* const* save2_ptrs;
    const float* act_init; int64_t act_init_rows; const float* rk_coef; const float* rk_basis; int rk_k; const uint32_t* dump_tiles;
    int64_t n_rows; float* out; const float* live_count; int64_t live_period;
} PsnMlpLaunch;
/* What a launch ran: the kernel instantiation (chain or lean engine; width16 = hidden width / 16 = 16, 8 or 4; src = where the rows
 * come from: 0 tables, 1 / 4 the row- / feature-parallel root finder, 2 points, 3 the sweep) and its grid.  `path` (or NULL) is
 * filled when a launch happens and zeroed otherwise (n_rows <= 0, a refusal); psn_mlp_last_path gives the same for the calling
 * thread's last launch of the engine through ANY entry (psn_mlp_infer_pe*, psn_march_sweep and psn_root_find included). */
typedef struct { int chain, width16, src, trim, from_a, x3, tb_lds, pm_groups; int64_t blocks, pm_period; } PsnMlpPath;
int psn_mlp_launch(const PsnMlpDesc* desc, const float* packed_w, const float* packed_b, const PsnMlpLaunch* launch, PsnMlpPath* path,
                   void* stream);
int psn_mlp_last_path(PsnMlpPath* path);
/* Workgroup order of the psn_mlp_launch launches whose rows are (group, point) pairs, row = group * P + point with a_div = 1,
 * b_div = a_mod = P, n_rows = P * b_mod -- the light-major row set of stage2/model/renderer.py:163,183-193.  1 (default): the
 * 64-row blocks are visited point-tile-major with the group (light) running fastest and every XCD takes a contiguous eighth of
 * that order, so that the workgroups resident at one time share a few point tiles and the per-point init table is read from
 * the fabric once instead of once per light; 0: row order (the light-major sweep).  A row's result does not depend on the
 * order (bit-identical outputs and dumps).  Process-wide; returns the previous value. */
int psn_mlp_block_order(int point_major);

/* Dense per-pixel outputs of the stage-2 model, stage2/model/renderer.py:145-152,204-264: dense [B, N, C] = fill
 * everywhere except dense[b, idx[r], c] = rows[(b Ns + r) row_stride + c col_stride] (light-major surface rows;
 * col_stride 0 broadcasts one column, as the reference's .expand(-1, 3) does).  Up to PSN_SCATTER_MAX_ITEMS outputs in one
 * launch.  inv [N] int32: surface row of a pixel or -1.  psn_gather_rows is the adjoint: rows [B Ns, C] (contiguous,
 * written) = dense[b, idx[r], c] with idx [Ns] int64 (the `rows` pointer of an item is then the OUTPUT). */
#define PSN_SCATTER_MAX_ITEMS 16
typedef struct {
    const float* rows;
    float* dense;
    int64_t row_stride, col_stride;
    int B, C;
    float fill;
} PsnScatterItem;
int psn_scatter_rows(int n_items, const PsnScatterItem* items, const int* inv, int64_t N, int64_t Ns, void* stream);
int psn_gather_rows(int n_items, const PsnScatterItem* items, const int64_t* idx, int64_t N, int64_t Ns, void* stream);
/* psn_gather_rows for an index list that may be PADDED (psn_surface_index): rows r with inv[idx[r]] != r receive zeros. */
int psn_gather_rows_valid(int n_items, const PsnScatterItem* items, const int64_t* idx, const int* inv, int64_t N, int64_t Ns, void* stream);

/* One secant (regula falsi) iteration of the surface refinement, stage1/model/rendering.py:525-555, for n hit rays:
 * with occ [n] (occupancy at the current d_pred; NULL for the initial step) the bracket (d_low, d_high, f_low, f_high,
 * all [n], updated in place) moves -- f_mid = occ - tau replaces the end with its sign -- then
 * d_pred = -f_low (d_high - d_low) / (f_high - f_low) + d_low and, if p_mid != NULL, p_mid [n,3] = origin + d_pred dir. */
int psn_secant_step(const float* occ, float tau, float* d_pred, float* d_low, float* d_high, float* f_low, float* f_high,
                    const float* origin, const float* dir, float* p_mid, int64_t n, void* stream);

/* First free -> occupied crossing of the ray-march sweep, stage1/model/rendering.py:457-504: occ [n_rays, n_steps]
 * (occupancy of the sweep points), far [n_rays] (sphere exit depth), u / omu [n_steps] = linspace(0, 1) and 1 - it (the
 * sweep depths are near * omu + far * u).  bracket [4, n_rays] = d_low, d_high, f_low, f_high of the crossing (values are
 * occupancy - tau); flags [n_rays] int32: bit 0 = a free -> occupied crossing exists on a ray that starts in free space
 * (the reference's `mask`), bit 1 = the ray starts in free space (`mask_0_not_occupied`). */
int psn_first_crossing(const float* occ, const float* far, const float* u, const float* omu, float near, float tau,
                       int64_t n_rays, int n_steps, float* bracket, int* flags, void* stream);

/* Shadow-ray sample points that lie inside the object box, stage1/model/rendering.py:378-408: for the dense rows
 * q = (l n_surf + s) n_steps + m the point p = surf[s] + ldir[l] (lnear omu[m] + lfar u[m]) is generated and, if
 * |p|_inf <= box, appended (atomic counter, caller zeroes it) as pts[k] = p, rows[k] = q.  pts [>= in-box count, 3],
 * rows [>= in-box count] int64, counter [1] uint64.  The caller evaluates the occupancy on pts only; every other row has
 * occupancy 0 by the reference's own rule (alpha[~amask] = 0). */
int psn_shadow_points(const float* surf, const float* ldir, int64_t n_surf, int n_lights, int n_steps, float lnear, float lfar,
                      const float* u, const float* omu, float box, float* pts, int64_t* rows, unsigned long long* counter,
                      void* stream);

/* Positional encoding + network in one launch (stage1/model/network.py:141-150 feeding :85-101; the occupancy queries of
 * the march sweep, rendering.py:410-470, and of the shadow rays, :378-408): points [n_rows, 3]; the encoding
 * gamma(pe_scale * p) with pe_octaves bands is formed in the kernel prologue, in registers, with the expressions of
 * psn_pe_encode -- out equals psn_pe_encode (stride 64) followed by psn_mlp_launch bit for bit, and the [n_rows, 64] table
 * never exists.  desc / packed_w / packed_b as for psn_mlp_launch, restricted to: 256-wide hidden layers without init tables,
 * in_kt_a = 2 (one 64-column block), biases packed back to back, n_out <= 32.  out [n_rows, n_out]. */
int psn_mlp_infer_pe(const PsnMlpDesc* desc, const float* packed_w, const float* packed_b, const float* points, int64_t n_rows,
                     int pe_octaves, float pe_scale, float* out, void* stream);
/* psn_mlp_infer_pe over a compacted point list whose length lives on the device (the counter psn_shadow_points writes): the
 * grid covers `capacity` rows, workgroups behind *n_rows_dev leave at once; with out_rows, row r's outputs go to
 * out[out_rows[r] * n_out ...] (scatter).  The shadow-ray visibility of stage1/model/rendering.py:378-408 without a host
 * synchronisation between the +-1.1 box test (:400-401) and the occupancy network. */
int psn_mlp_infer_pe_indirect(const PsnMlpDesc* desc, const float* packed_w, const float* packed_b, const float* points,
                              int64_t capacity, const long long* n_rows_dev, const int64_t* out_rows, int pe_octaves,
                              float pe_scale, float* out, void* stream);

/* Ray-march sweep, stage1/model/rendering.py:447-462 (+ the early termination its consumer :472-504 allows): the occupancy
 * sigmoid(-10 logit) of n_steps proposal points per ray, p = origin + dir * (near (1 - u_m) + far u_m), generated and
 * encoded inside the kernel -- no [n_rays, n_steps, 3] point tensor, same bits as psn_sample_points + psn_mlp_infer_pe.
 * One workgroup = 64 consecutive steps of one ray (n_steps % 64 == 0), workgroups in block-major order.  skip: int32
 * [n_rays], ZEROED by the caller, or NULL: a block that contains a sign change of (occ - tau) between neighbouring steps
 * (or a ray whose first value is not free) records its block index in the ray's flag (INT_MAX - block, the lowest block
 * wins; 0 = none) and only blocks BEHIND the recorded one leave unevaluated, whatever order the workgroups ran in -- their
 * entries of occ stay untouched; every value up to and including the pair of the FIRST sign change is always written,
 * which is all psn_first_crossing reads.  n_blocks: NULL, or a device counter that receives the number of 64-step blocks
 * evaluated (measurement).  desc / packed_w / packed_b as for psn_root_find.  occ [n_rays, n_steps]. */
int psn_march_sweep(const PsnMlpDesc* desc, const float* packed_w, const float* packed_b, const float* origin, const float* dir,
                    const float* far, const float* u, const float* omu, float near, int64_t n_rays, int n_steps, float tau,
                    int pe_octaves, float pe_scale, int* skip, unsigned long long* n_blocks, float* occ, void* stream);

/* Fused secant refinement, stage1/model/rendering.py:525-555: n_iter regula-falsi iterations for every ray inside ONE
 * launch -- query point origin + d_pred * dir, its positional encoding (pe_octaves bands, input scaled by pe_scale), the
 * occupancy network (desc / packed_w / packed_b as for psn_mlp_launch: 256-wide, one output, PSN_OUT_OCC, input block =
 * one 64-column encoding) and the bracket update -- instead of one encoding + network + update launch per iteration.
 * bracket [4, n_rays] as written by psn_first_crossing (not modified); d_out [n_rays] = the final d_pred. */
int psn_root_find(const PsnMlpDesc* desc, const float* packed_w, const float* packed_b, const float* origin, const float* dir,
                  const float* bracket, int64_t n_rays, float tau, int n_iter, int pe_octaves, float pe_scale, float* d_out,
                  void* stream);

/* ------------------------------------------------------------------------
 * Stage-2 losses, stage2/model/loss.py:27-58,76-92 (MainLoss) and :123-141 (NormalLoss), over the dense outputs of the
 * model with mask = mask_a & mask_b (network_object_mask & object_mask, bool [N]):
 *   term 0  rgb        sum |rgb - rgb_gt| (l2 = 0) or squared (l2 = 1) over [L, N, 3]
 *   term 1  albedo     sum |alb - alb_j| over [N, 3]              term 2  SG weights  sum |wgt - wgt_j| over [N, nb]
 *   term 3  visibility sum |vis[v, n, 0] - vis_gt[v, n]| (or squared) over [V, N]   (vis is [V, N, 3])
 *   term 4  normal     sum (nrm - normalize(nrm_gt))^2 over [N, 3]   term 5  normal smoothness  sum |nrm - nrm_j|
 * A term whose first pointer is NULL is skipped (0).  out[i] = sum_i * inv_denom[i] (i < 6), out[6] = sum_i weight[i] out[i];
 * inv_denom, weight: HOST arrays [6] (passed by value).  count_dev (optional, device [1] float): the masked-pixel count;
 * when given, inv_denom holds only the per-pixel multiplicities (1 / (L 3), 1 / 3, 1 / nb, 1 / V, 1 / 3, 1 / 3) and
 * every term (and every gradient in _bwd) is divided by count_dev[0] on the device (0 for an empty mask), so the count --
 * possibly all-reduced over ranks -- never has to reach the host.  partial: device workspace of >= 2048 * 6 floats.
 * Deterministic summation order.
 * psn_stage2_loss_bwd writes d(out[6]) / d(input) * g_total[0] for every non-NULL d_* (k_i = weight_i * inv_denom_i on the
 * host); masked-out pixels get zeros; d_vis channels 1, 2 are zero. */
int psn_stage2_loss_fwd(const float* rgb, const float* rgb_gt, int L, const float* alb, const float* alb_j, const float* wgt,
                        const float* wgt_j, int nb, const float* vis, const float* vis_gt, int V, const float* nrm,
                        const float* nrm_gt, const float* nrm_j, const unsigned char* mask_a, const unsigned char* mask_b,
                        int64_t N, int l2, const float* inv_denom, const float* weight, const float* count_dev, float* partial,
                        float* out, void* stream);
int psn_stage2_loss_bwd(const float* g_total, const float* rgb, const float* rgb_gt, int L, float k_rgb, float* d_rgb,
                        const float* alb, const float* alb_j, float k_alb, float* d_alb, float* d_alb_j, const float* wgt,
                        const float* wgt_j, int nb, float k_wgt, float* d_wgt, float* d_wgt_j, const float* vis, const float* vis_gt,
                        int V, float k_vis, float* d_vis, const float* nrm, const float* nrm_gt, const float* nrm_j, float k_nrm,
                        float k_nrmj, float* d_nrm, float* d_nrm_j, const unsigned char* mask_a, const unsigned char* mask_b,
                        int64_t N, int l2, const float* count_dev, void* stream);

/* ------------------------------------------------------------------------
 * Stage-1 losses of the sync-free training forward, stage1/model/losses.py:24-70, over per-ray tensors ([N] / [N, 3]):
 *   sums[0] = sum |rgb - rgb_gt|                               sums[4] = #hit
 *   sums[1] = sum over hit rays of diff (smoothness)           sums[5] = #norm_mask
 *   sums[2] = sum over norm_mask of |normal - normal_gt|       sums[6] = #mask_valid
 *   sums[3] = sum over mask_valid of BCE(clamp(acc, 0, 1), mask_gt) with the log terms clamped at -100
 * terms[0..3] = sums[0] / n_rays, sums[1] / max(sums[4], 1), sums[2] / max(sums[5], 1), sums[3] / max(sums[6], 1);
 * terms[4] = weights[0] terms[0] + weights[1] terms[1] (+ weights[2] terms[2]) (+ weights[3] terms[3]), a term with NULL
 * inputs (or weight 0 for the first two) being skipped.  weights: HOST array [4] (full, grad, norm, mask).  n_rays: the
 * ray count of the whole batch (all ranks).  psn_stage1_loss_fwd with terms == NULL stops after the sums, so that the caller
 * can all-reduce sums[4..6] over ranks and finish with psn_stage1_loss_terms.  partial: device workspace of
 * psn_stage1_loss_partial_floats() floats.  Deterministic summation order.
 * psn_stage1_loss_bwd: d terms[4] / d input * g_loss[0] for every non-NULL d_* (counts read from sums on the device).
 * psn_surface_normals_{fwd,bwd}: stage1/model/rendering.py:200-212 for g [2 N, 3] (gradients of the geometry field at the N
 * surface points and at their N jittered neighbours): n = g / (|g| + eps); norm_pred [N, 3] = hit ? n[:N] : 0;
 * diff [N] = |n[:N] - n[N:]|; backward: dg [2 N, 3] from d_norm_pred / d_diff (either may be NULL). */
int psn_stage1_loss_partial_floats(void);
int psn_stage1_loss_fwd(const float* rgb, const float* rgb_gt, const float* diff, const unsigned char* hit, const float* normal,
                        const float* normal_gt, const unsigned char* norm_mask, const float* acc, const float* mask_gt,
                        const unsigned char* mask_valid, int64_t N, int64_t n_rays, const float* weights, float* partial,
                        float* sums, float* terms, void* stream);
int psn_stage1_loss_terms(const float* sums, int64_t n_rays, const float* weights, int has_grad, int has_norm, int has_mask,
                          float* terms, void* stream);
int psn_stage1_loss_bwd(const float* g_loss, const float* sums, const float* rgb, const float* rgb_gt, const unsigned char* hit,
                        const float* normal, const float* normal_gt, const unsigned char* norm_mask, const float* acc,
                        const float* mask_gt, const unsigned char* mask_valid, int64_t N, int64_t n_rays, const float* weights,
                        float* d_rgb, float* d_diff, float* d_normal, float* d_acc, void* stream);
int psn_surface_normals_fwd(const float* g, const unsigned char* hit, int64_t N, float eps, float* norm_pred, float* diff,
                            void* stream);
int psn_surface_normals_bwd(const float* g, const unsigned char* hit, int64_t N, float eps, const float* d_norm_pred,
                            const float* d_diff, float* dg, void* stream);

/* Sums of x [V, Ns, C] (C <= 256, V <= PSN_PAIR_SUMS_MAX_V) over V and over Ns in one pass: sx [Ns, C] = sum_v x and
 * sl_part [*n_chunks, V, C] = per-chunk partial sums over Ns (the caller adds the chunks; at most PSN_PAIR_SUMS_MAX_CHUNKS).
 * Used for the separable weight gradient of a layer whose input block is [table(x_n) | table(l_v)]. */
#define PSN_PAIR_SUMS_MAX_V 16
#define PSN_PAIR_SUMS_MAX_CHUNKS 2048
int psn_pair_sums(const float* x, int V, int64_t Ns, int C, float* sx, float* sl_part, int* n_chunks, void* stream);
/* The separable input-block weight gradients of the visibility network's backward (stage2/model/renderer.py:191-200, 251-262:
 * input row k = v Ns + n is [table(x_n) | table(l_v)]) for up to PSN_PAIR_GROUP_MAX input layers in two launches (three when the
 * per-chunk partial sums are many: their reduction is then sliced over 32 blocks per output tile).  Per item,
 * with x = d z [V, Ns, C]:  sx [Ns, C] = sum_v x (the K = Ns operand of d W_x);  dWl [C, ld_w] (columns < n_pe written) =
 * (sum_n x[v])^T pe_l[v] summed over v, pe_l [V, ld_pe];  bias [C] = sum over v and n of x (NULL: not wanted).
 * workspace: psn_pair_sums_group_workspace(...) floats, 16-byte aligned.  Fixed summation order (deterministic). */
#define PSN_PAIR_GROUP_MAX 4
typedef struct { const float* x; float* sx; float* dWl; float* bias; } PsnPairSumsItem;
int64_t psn_pair_sums_group_workspace(int n_items, int V, int64_t Ns, int C);
int psn_pair_sums_group(int n_items, const PsnPairSumsItem* items, int V, int64_t Ns, int C, const float* pe_l, int64_t ld_pe, int n_pe,
                        int64_t ld_w, float* workspace, void* stream);

/* torch.optim.SparseAdam on the touched rows of up to PSN_ROW_ADAM_MAX tables in one launch (the per-light direction
 * [n, 3] and intensity [n, 1] embeddings, stage2/trainer.py:126-168): rows listed in idx [n_idx] int64 (duplicates
 * allowed) advance their moments and move by -step_size m / (sqrt(v) + eps), step_size = lr sqrt(1 - b2^t) / (1 - b1^t)
 * computed by the caller; all other rows and their moments stay untouched.  grad is the DENSE gradient [rows, cols]. */
#define PSN_ROW_ADAM_MAX 4
typedef struct {
    float* param; const float* grad; float* exp_avg; float* exp_avg_sq;
    int64_t rows; int cols;
    float one_minus_beta1, one_minus_beta2, eps, step_size;  /* 1 - beta computed in double by the caller, like torch */
} PsnRowAdamItem;
int psn_row_adam(int n_items, const PsnRowAdamItem* items, const int64_t* idx, int n_idx, void* stream);
/* The same launch with the step sizes read from DEVICE memory (step_sizes_dev [n_items], item i uses element i; the host
 * values in items[] are ignored): identical from step to step, so it can be replayed from a HIP graph while the host
 * refreshes the scalars (psnerf_amd/stage2/graph.py; the lr schedule and the bias corrections of stage2/trainer.py:402-410,462-464). */
int psn_row_adam_dev(int n_items, const PsnRowAdamItem* items, const int64_t* idx, int n_idx, const float* step_sizes_dev, void* stream);

/* ------------------------------------------------------------------------
 * The launch-bound tail of a stage-2 train step as single kernels (csrc/small.hip).
 *
 * psn_normalize_rows_{fwd,bwd}: torch.nn.functional.normalize(x, p=2, dim=-1, eps) of [n, 3] rows, y = x / max(|x|, eps),
 *   and autograd's backward of it (div -> clamp_min -> norm); stage2/model/renderer.py:129,137 (the predicted normals).
 * psn_light_rows_{fwd,bwd}: the light-table lookups of a step, stage2/trainer.py:376-379: dir_out [n_idx, 3] =
 *   normalize(dir_table[idx]), int_out [n_idx] = int_table[idx] (int_table / int_out may both be NULL).  Backward writes
 *   the DENSE table gradients d_dir_table [n_rows, 3], d_int_table [n_rows] (every row: zeros where untouched, duplicate
 *   indices summed in list order -- what nn.Embedding(sparse=False) + F.normalize produce); a NULL gradient pair is skipped.
 * psn_camera_rays: stage2/utils/rend_util.py:90-147 for a 4 x 4 pose: out[i] = scale * normalize(R [(u - cx) / fx,
 *   (v - cy) / fy, 1]) for pixel idx[i] (idx NULL: pixel i) of uv [N, 2]; pose / intrinsics: 16 floats each, row-major, on
 *   the device.
 * psn_stage1_rays: the ray set-up of a stage-1 batch (batch size 1) in one launch: cam[i] = world_mat[:3, 3]
 *   (stage1/model/common.py:205-207), rays[i] = normalize(R [(px - cx) / fx, (py - cy) / fx, 1]) (common.py:210-226: BOTH
 *   axes over fx = K[0][0], the reference's quirk; rendering.py:64-65), far[i] = the sphere exit depth max(sqrt(b^2 - (|cam|^2 -
 *   radius2)) - b, 0), 0 for rays that miss the sphere (rendering.py:576-596).  camera_mat: k_ld x k_ld row-major (3 or 4),
 *   world_mat 4 x 4, both on the device.
 * psn_surface_points: rendering.py:516-522 + :84-108 -- d = flags & 1 ? d_pred : inf; d = flags & 2 ? d : 0 (d_i, optional
 *   output); obj_mask = finite(d) & d != 0; dists = obj_mask ? d : (d == 0 ? 0 : 1); points = cam + rays * dists.
 * psn_stage1_targets: the ground truth of the sampled pixels, stage1/model/common.py:172-202 (nearest-neighbour
 *   grid_sample, align_corners, at x = 2 px / w - 1, y = 2 py / h - 1) applied to the image [3, h, w], the masks [h, w] (a NULL
 *   mask / mask_valid image is all ones; outputs: mask_gt float 0/1, mask_valid_out / norm_mask_out bytes 0/1 = torch.bool
 *   storage) and the normal map [3, h, w] (training.py:176-191: norm_mask cleared where the UNROTATED n_z < cos_thresh when
 *   use_angle, then normal_gt = R diag(1, -1, -1) n with R = world_mat[:3, :3]).  Optional outputs may be NULL.
 * psn_adam_flat: torch.optim.Adam's update (torch/optim/adam.py::_multi_tensor_adam; amsgrad off, weight_decay 0;
 *   stage2/trainer.py:126-133) over ranges of one flat parameter / gradient / exp_avg / exp_avg_sq allocation:
 *   m += (1 - beta1)(g - m); v = v beta2 + (1 - beta2) g g; p += neg_step_size * m / (sqrt(v) / bias_correction2_sqrt + eps),
 *   neg_step_size = -lr / (1 - beta1^t) per range (parameters that joined the optimisation later have their own t).
 * ---------------------------------------------------------------------- */
int psn_normalize_rows_fwd(const float* x, int64_t n, float eps, float* y, void* stream);
int psn_normalize_rows_bwd(const float* x, const float* g, int64_t n, float eps, float* dx, void* stream);
int psn_light_rows_fwd(const float* dir_table, const float* int_table, const int64_t* idx, int n_idx, float eps, float* dir_out,
                       float* int_out, void* stream);
int psn_light_rows_bwd(const float* dir_table, const int64_t* idx, int n_idx, int64_t n_rows, float eps, const float* g_dir,
                       const float* g_int, float* d_dir_table, float* d_int_table, void* stream);
int psn_camera_rays(const float* uv, const float* pose, const float* intrinsics, const int64_t* idx, int64_t n, float scale,
                    float* out, void* stream);
int psn_stage1_rays(const float* pix, const float* camera_mat, int k_ld, const float* world_mat, float radius2, int64_t n,
                    float* cam, float* rays, float* far, void* stream);
int psn_surface_points(const float* d_pred, const int* flags, const float* cam, const float* rays, int64_t n, float* d_i,
                       float* dists, unsigned char* obj_mask, float* points, void* stream);
int psn_stage1_targets(const float* pix, int64_t n, int h, int w, const float* img, const float* mask, const float* mask_valid,
                       const float* normal, const float* norm_mask, const float* world_mat, int use_angle, float cos_thresh,
                       float* rgb_gt, float* mask_gt, unsigned char* mask_valid_out, float* normal_gt,
                       unsigned char* norm_mask_out, void* stream);
/* Front of a stage-2 step (stage2/trainer.py:355-392, stage2/model/renderer.py:110-152), one launch each:
 * psn_mask_count: out[0] = #{i : mask_a[i] && mask_b[i]} as a float (masks = torch.bool storage, mask_b may be NULL; n < 2^24) --
 *   the masked-pixel count that normalises the losses (stage2/model/loss.py:27-38);
 * psn_inverse_index: inv[p] = position of pixel p in the ascending surface-pixel list idx[0 .. ns), or -1 (the pixel -> row map
 *   of psn_scatter_rows). */
/* psn_copy2d_group: up to PSN_COPY2D_MAX row-major 2-D copies dst[r][c] = src[r][c] (r < rows, c < cols; row strides ld_*) in
 *   one launch -- the side tables of a weight pack (init-table column slices of the parameters, bias segments), which were
 *   a slice copy or a concatenation each.  HOST array of items holding device pointers. */
#define PSN_COPY2D_MAX 24
typedef struct {
    const float* src; int64_t ld_src;
    float* dst; int64_t ld_dst;
    int rows, cols;
} PsnCopy2dItem;
int psn_copy2d_group(int n_items, const PsnCopy2dItem* items, void* stream);
/* Up to PSN_COPY_BYTES_MAX contiguous copies of any element type in ONE launch: a training batch (stage2/trainer.py:364-392: ~17
 * tensors of floats, bools and indices) into the fixed input buffers of a captured HIP graph (one device-to-device copy each cost
 * ~5 us of dependent-launch latency).  `aligned` is filled in by the library (both pointers 16-byte aligned). */
#define PSN_COPY_BYTES_MAX 24
typedef struct { const void* src; void* dst; int64_t n_bytes; int aligned; } PsnCopyBytesItem;
int psn_copy_bytes_group(int n_items, const PsnCopyBytesItem* items, void* stream);
int psn_mask_count(const unsigned char* mask_a, const unsigned char* mask_b, int64_t n, float* out, void* stream);
/* psn_surface_index: idx[0 .. ns) = ascending positions of the set bytes of mask [n] (= surface_mask[0].nonzero(),
 *   stage2/model/renderer.py:125, without a host synchronisation), idx[ns .. cap) = idx[ns - 1]: a FIXED-size list whose
 *   dead tail repeats the last surface pixel (0 for an empty mask); count[0] (may be NULL) = ns as a float.  A list longer than
 *   cap is truncated.  Kernels that read such a list treat entries behind the first of equal neighbours as dead rows
 *   (psn_gather_rows_valid); psn_inverse_index maps a pixel to the FIRST of equal entries; count (device float [1], or NULL = ns):
 *   only the first count[0] entries of idx are real -- an EMPTY mask then gives no pixel a row. */
int psn_surface_index(const unsigned char* mask, int64_t n, int64_t cap, int64_t* idx, float* count, void* stream);
int psn_inverse_index(const int64_t* idx, int64_t ns, int64_t n_pix, int* inv, const float* count, void* stream);
/* psn_view_batch: ONE training batch of stage 2 gathered on the device from view tables that stay resident in HBM -- replaces the
 * host-side item construction of stage2/datasets/dataset.py:137-199 (light subset :149-151 -> rgb = imgs[view][lidx] * object_mask
 * :172; pixel subset :182-195 -> every per-pixel tensor indexed with sampling_idx), the un-batching of stage2/trainer.py:364-367 and
 * the vis_plus selection of stage2/trainer.py:384-392 (vis_train_gt = vis_plus_v[sidx][:, sampling_idx]) + the upload of the batch.
 * Only the drawn INDEX lists (lidx, pix, vidx: device int64) are per-step inputs; a data-parallel rank passes its slice of pix.
 *   images [n_view_lights, hw, 3] of image_type 0 = float32 | 1 = uint8 | 2 = uint16; integer images are decoded through lut
 *     ([256] / [65536] floats = value / 255 exactly as the reference's numpy division forms it, dataset.py:121);
 *   object_mask / surface_mask [hw] bytes, points / normal [hw, 3], visibility [n_view_lights, hw], vis_plus [n_rows, hw],
 *     light_direction [n_view_lights, 3] floats;
 *   pix [n] pixel indices, or NULL = the identity range pix0 .. pix0 + n (a test-split item, dataset.py:182 not taken); width = image
 *     width (uv = (pix % width, pix / width) as floats, dataset.py:138-140).
 * Outputs (any may be NULL = not produced; all contiguous): rgb [n_lights, n, 3]; object_mask_out / surface_mask_out [n] bytes;
 * uv [n, 2]; points_out / normal_out [n, 3]; visibility_out [n_lights, n]; vis_train_gt [n_vis, n]; sampling_idx_out [n] int64;
 * light_direction_out [n_lights, 3] = light_direction[lidx].
 * n = 0 (after the argument checks): PSN_OK without a launch, and NO output is written -- light_direction_out included, although
 * its rows do not depend on n: a batch without pixels has no consumer, and the caller's buffer keeps what it held. */
typedef struct {
    const void* images; int image_type; const float* lut;
    const unsigned char* object_mask; const unsigned char* surface_mask;
    const float* points; const float* normal; const float* visibility; const float* vis_plus; const float* light_direction;
    int64_t hw; int width;
    const int64_t* lidx; int n_lights;
    const int64_t* pix; int64_t pix0; int64_t n;
    const int64_t* vidx; int n_vis;
    float* rgb; unsigned char* object_mask_out; unsigned char* surface_mask_out; float* uv; float* points_out; float* normal_out;
    float* visibility_out; float* vis_train_gt; int64_t* sampling_idx_out; float* light_direction_out;
} PsnViewBatch;
int psn_view_batch(const PsnViewBatch* b, void* stream);
#define PSN_ADAM_MAX_SEGS 16
typedef struct {
    int64_t offset, grad_offset, n;    /* elements [offset, offset + n) of param / exp_avg / exp_avg_sq, [grad_offset, ..+n) of grad */
    float neg_step_size;               /* -lr / (1 - beta1^t) */
    float bias_correction2_sqrt;       /* sqrt(1 - beta2^t) */
} PsnAdamSeg;
int psn_adam_flat(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int n_segs, const PsnAdamSeg* segs,
                  float one_minus_beta1, float beta2, float one_minus_beta2, float eps, void* stream);
/* psn_adam_flat with (neg_step_size, bias_correction2_sqrt) of range i read from DEVICE memory, seg_scalars_dev[2 i],
 * seg_scalars_dev[2 i + 1] (the host values in segs[] are ignored): a launch that is identical from step to step (HIP-graph
 * replay; the host refreshes the scalars before each replay). */
int psn_adam_flat_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int n_segs, const PsnAdamSeg* segs,
                      float one_minus_beta1, float beta2, float one_minus_beta2, float eps, const float* seg_scalars_dev, void* stream);

/* ------------------------------------------------------------------------
 * Weight normalisation of up to PSN_WN_MAX_ITEMS layers in one launch: nn.utils.weight_norm(nn.Linear) as used by every
 * layer of stage1/model/network.py:37-66 (state_dict keys weight_g [rows,1], weight_v [rows,cols]).
 *   fwd: w = v * (g / |v|_row) [* scale]       (scale = 1/sqrt(2) folds the cat[x, pe]/sqrt(2) of network.py:90-91)
 *   bwd: given dw (gradient of the scaled w):  dv, dg
 * All matrices row-major and dense (row stride = cols).  HOST array of items holding device pointers.
 * ---------------------------------------------------------------------- */
#define PSN_WN_MAX_ITEMS 16
typedef struct {
    const float* v;   /* [rows, cols] */
    const float* g;   /* [rows] */
    float* w;         /* fwd: [rows, cols] output */
    const float* dw;  /* bwd: [rows, cols] */
    float* dv;        /* bwd: [rows, cols] output */
    float* dg;        /* bwd: [rows] output */
    int rows, cols;
    float scale;
} PsnWnItem;
int psn_weight_norm_fwd(int n_items, const PsnWnItem* items, void* stream);
int psn_weight_norm_bwd(int n_items, const PsnWnItem* items, void* stream);

/* ------------------------------------------------------------------------
 * bf16 inference engine (evaluation / relighting only; BASELINE config 5 "bf16 MFMA path ... envmap relight eval"):
 * the 256-wide ReLU networks of stage2/model/renderer.py:34-49 on v_mfma_f32_32x32x16_bf16 -- weights, input
 * features and post-ReLU activations rounded to bf16 (RNE), fp32 accumulation, fp32 output.  Replaces the no-grad
 * evaluation of visibility_net in stage2/eval.py:199-218 (via renderer.py:191-200) when the caller opts in; training
 * and every parity-gated path use psn_mlp_launch (exact fp32).
 *
 * Network: n_hidden hidden layers of width 256 with ReLU; layer 0 reads the input block only, layer l >= 1 reads the
 * previous activations and, if has_in[l], the input block again (skip connection cat[y, x]); a final layer with
 * n_out <= 32 outputs followed by out_act.  The input block of row q is
 * [ A[(q / a_div) % a_mod, 0:64] | B[(q / b_div) % b_mod, 0:64] ] with bf16 tables of 64 columns (128-byte rows).
 *
 * Weight stream (bf16, one contiguous buffer, in execution order), each piece written by psn_lowp_pack with one plane:
 *   layer 0:      input block k-steps 0..7 [W_a | W_b] natural order, 1 bias k-step            (72 KB)
 *   layer l >= 1: activation k-steps 0..7 (permuted), 1 bias k-step (72 KB); if has_in[l]: input block k-steps 0..7
 *                 (64 KB); activation k-steps 8..15 (64 KB)
 *   final:        activation k-steps 0..15 with n_ot = 1 (16 KB); its bias is added in fp32 from final_bias[32].
 *                 The kernel always requests whole 72 KB stages: the buffer must extend (any content) 56 KB past
 *                 the final block.
 * A k-step covers 16 K indices; a bias k-step is the [256, 2] matrix (bf16(b), b - bf16(b)) packed in natural order.
 * ---------------------------------------------------------------------- */
typedef struct {
    int32_t n_hidden;
    int32_t n_out;
    int32_t out_act; /* PSN_OUT_* */
    int32_t reserved;
    uint8_t has_in[PSN_MLP_MAX_LAYERS + 4];
} PsnBf16Desc;

/* The packers of this engine (n_planes = 1, n_pieces = 2) and of the split-bf16 engine below (3, 3; anything else is refused).
 * Piece p of an fp32 value = the round-to-nearest-even bf16 of what pieces 0 .. p - 1 left: three add up to the value exactly.
 * psn_lowp_pack: k-steps [ks0, ks0 + n_ks) of W[rows, cols] (row-major fp32, ldw floats per row, zero-extended) for n_ot output
 * tiles of 32 (8 = hidden layer, 1 = final layer) -> dst[n_ks][n_ot][n_planes][64 lanes][8] bf16, plane p = piece p, element j
 * of lane (m, h) = W[32 ot + m][k].  permuted != 0: K follows the register layout of the previous layer's activations,
 * k = 32 (ks / 2) + 16 (ks % 2) + 8 (j / 4) + 4 h + (j % 4); 0: natural order (input block, bias columns), k = 16 ks + 8 h + j.
 * psn_lowp_pack_bias: V [n, 256] fp32 -> dst[n][8 tiles][64 lanes][8] bf16: n bias k-steps, K slots 0 .. n_pieces - 1 = the pieces. */
int psn_lowp_pack(const float* W, int64_t ldw, int rows, int cols, int permuted, int n_ot, int ks0, int n_ks, int n_planes,
                  uint16_t* dst, void* stream);
int psn_lowp_pack_bias(const float* V, int64_t n, int n_pieces, uint16_t* dst, void* stream);

/* out [n_rows, n_out] fp32.  tab_b may be NULL (input block = table A only).  All device buffers 16-byte aligned. */
int psn_mlp_infer_bf16(const PsnBf16Desc* desc, const uint16_t* packed_w, const float* final_bias, const uint16_t* tab_a,
                       int64_t a_div, int64_t a_mod, const uint16_t* tab_b, int64_t b_div, int64_t b_mod, int64_t n_rows,
                       float* out, void* stream);

/* Grouped form for the light-major rows (g, n) -> g * rows_per_group + n of stage2/model/renderer.py:163,193 (g = light,
 * n = surface point; the 512-light evaluation of stage2/eval.py:199-218): the input block of a row is table A row n
 * ([rows_per_group, 64] bf16) and the group's part of every input layer, W_b * B[g] + b, arrives as that group's bias:
 * group_bias [n_groups][n_in][8 KB] = one bias k-step per (group, input layer in network order), written by
 * psn_lowp_pack_bias (two pieces) from fp32 rows.  The light's encoding and its weight columns therefore stay in fp32 (one
 * small product per light and input layer on the host side) and cost no k-steps per row.
 * Weight stream: as above with 4 input k-steps (table A columns only) instead of 8 and WITHOUT the bias k-step of the
 * layers that read the input block:
 *   layer 0: input k-steps 0..3 (32 KB);  layer l >= 1: activation k-steps 0..7, bias k-step unless has_in[l];
 *   if has_in[l]: input k-steps 0..3 (32 KB); activation k-steps 8..15;  final: 16 KB, then >= 56 KB of padding.
 * out [n_groups * rows_per_group, n_out] fp32. */
int psn_mlp_infer_bf16_grouped(const PsnBf16Desc* desc, const uint16_t* packed_w, const float* final_bias,
                               const uint16_t* tab_a, int64_t rows_per_group, const uint16_t* group_bias, int64_t n_groups,
                               float* out, void* stream);

/* ------------------------------------------------------------------------
 * Split-bf16 ("bf16x6") inference engine, csrc/mlp_infer_x3.hip -- EXPERIMENT, opt-in, gradient-free rows only.  The network of
 * psn_mlp_infer_bf16_grouped with every fp32 operand carried as three bf16 planes (hi / mid / lo, exact sum) and every product as the
 * six partial products of weight >= 2^-16: fp32-class results from the bf16 matrix pipe.  Weights and bias k-steps: psn_lowp_pack and
 * psn_lowp_pack_bias with three planes / pieces.  Every entry (psn_march_sweep_x3 since version 102) refuses a packed_w or bias_steps
 * (grouped form: also U, V) off a 16-byte boundary.
 *   psn_mlp_infer_x3_grouped: rows (g, n) -> g * rows_per_group + n; packed_w = the weight stream in execution order (48 KB
 *     stages of 2 k-steps: every hidden layer >= 1 = its 16 activation k-steps; final layer = one stage [16 k-steps][3 planes],
 *     + 56 KB of padding); bias_steps [n_hidden][8 KB] (used for the layers without an input block).  The layers that read
 *     the input block start from U[n] + V[g] (both fp32, [., n_input_layers * 256]): U = W_a x_n per row, V = W_b x_g + b per
 *     group, as the init tables of psn_mlp_launch; layer 0 is that sum alone.  out [n_groups * rows_per_group, n_out] fp32.
 * ---------------------------------------------------------------------- */
int psn_mlp_infer_x3_grouped(const PsnBf16Desc* desc, const uint16_t* packed_w, const uint16_t* bias_steps, const float* final_bias,
                             const float* U, int64_t rows_per_group, const float* V, int64_t n_groups, float* out, void* stream);
/* The stage-1 occupancy network (stage1/model/network.py:85-101: softplus(beta = 100) stack on the positional encoding of the point,
 * cat[h, pe] / sqrt(2) in front of the skip layer, output row 0) on the split-bf16 engine, for GRADIENT-FREE queries (shadow rays
 * rendering.py:378-408, ray march :447-462, shape_extract :297-376): out[r] = sigmoid(-10 logit(points[r])). desc: n_hidden, n_out = 1,
 * out_act; packed_w: layer 0 as 4 natural-order k-steps of its encoding columns, every further hidden layer 16 permuted k-steps (the
 * skip layer as ONE 256-input matrix, scaled by 1 / sqrt(2)), the final row as one stage; bias_steps [n_hidden][4096]; final_bias [32].
 * The kernel forms the encoding (pe_octaves, pe_scale: the expressions of psn_pe_encode) and writes it into input features pe_first ..
 * of layer skip_layer (-1: none).  n_rows_dev / out_rows: as psn_mlp_infer_pe_indirect (row count on the device, outputs scattered). */
int psn_mlp_infer_x3_occ(const PsnBf16Desc* desc, const uint16_t* packed_w, const uint16_t* bias_steps, const float* final_bias,
                         const float* points, int64_t n_rows, const long long* n_rows_dev, const int64_t* out_rows, int pe_octaves,
                         float pe_scale, int skip_layer, int pe_first, float* out, void* stream);
/* The ray-march sweep of stage1/model/rendering.py:447-462 on the split-bf16 engine (opt-in experiment; psn_march_sweep is the exact
 * form): occ [n_rays, n_steps] = sigmoid(-10 logit) at the points origin + dir (near (1 - u_m) + far u_m), formed and encoded in the
 * kernel; a workgroup = 128 consecutive steps of one ray, block-major.  skip [n_rays] int32, zeroed by the caller (or NULL = every
 * block is evaluated): the blocks behind a ray's first sign change are left out -- their entries stay unwritten, and nothing
 * reads them (psn_first_crossing stops at the first crossing).  n_steps a multiple of 128; desc / packed_w / bias_steps /
 * final_bias / skip_layer / pe_first as for psn_mlp_infer_x3_occ.  n_blocks (or NULL): counts the evaluated blocks. */
int psn_march_sweep_x3(const PsnBf16Desc* desc, const uint16_t* packed_w, const uint16_t* bias_steps, const float* final_bias,
                       const float* origin, const float* dir, const float* far, const float* u, const float* omu, float near,
                       int64_t n_rays, int n_steps, float tau, int pe_octaves, float pe_scale, int skip_layer, int pe_first,
                       int* skip, float* occ, unsigned long long* n_blocks, void* stream);


/* ------------------------------------------------------------------------
 * Spherical-Gaussian shading over the light-major rows (l, n) -> l*Ns + n:
 * stage2/model/sgbasis.py:16-32 + stage2/model/renderer.py:174-204
 *   h = normalize(l + v); D_k = exp(max(lobe_k,0) (h.n - 1)); spec_c = max(sum_k w_{c,k} D_k, 0)
 *   rgb = clamp((albedo + spec) * I_l * (l.n) * clamp(vis,0,1), 0, 1)
 * light_dir [L,3]; view/normal/albedo [Ns,3]; weights [Ns, 3*nb] (specular_rgb, channel-major as
 * sgbasis.py:27 view(-1,3,nb)) or [Ns, nb]; lobe [nb<=9]; light_int [L, int_ch] or NULL (then light_int_scalar),
 * int_ch = 1, or 3 for RGB environment-map lights (stage2/eval.py:200; forward only);
 * vis [L*Ns] or NULL.  rgb [L*Ns,3]; spec [L*Ns,3] (specular_rgb) or [L*Ns].
 * Backward: g_rgb [L*Ns,3], g_spec like spec or NULL -> d_albedo [Ns,3], d_weights like weights,
 * d_normal [Ns,3], d_vis [L*Ns] or NULL, d_light_dir [L,3], d_light_int [L] or NULL;
 * workspace >= ceil(Ns/64)*L*4 floats.
 * ---------------------------------------------------------------------- */
int psn_sg_shade_fwd(const float* light_dir, const float* view, const float* normal, const float* albedo,
                     const float* weights, const float* lobe, const float* light_int, int int_ch, float light_int_scalar,
                     const float* vis, int L, int64_t Ns, int nb, int specular_rgb, float* rgb, float* spec,
                     void* stream);
int psn_sg_shade_bwd(const float* light_dir, const float* view, const float* normal, const float* albedo,
                     const float* weights, const float* lobe, const float* light_int, float light_int_scalar,
                     const float* vis, int L, int64_t Ns, int nb, int specular_rgb, const float* g_rgb,
                     const float* g_spec, float* d_albedo, float* d_weights, float* d_normal, float* d_vis,
                     float* d_light_dir, float* d_light_int, float* workspace, void* stream);

/* ------------------------------------------------------------------------
 * GGX microfacet shading (train.render_model = microfacet): stage2/model/microfacet.py:35-114 followed by
 * stage2/model/renderer.py:187-204, same row layout as psn_sg_shade_*.  rough [Ns] (sigmoid output of rough_net),
 * f0 = brdf.fresnel_f0.  rgb [L*Ns,3].  Backward: d_albedo [Ns,3], d_rough [Ns], d_normal [Ns,3], d_vis [L*Ns] or
 * NULL, d_light_dir [L,3], d_light_int [L] or NULL; workspace >= ceil(Ns/64)*L*4 floats.
 * ---------------------------------------------------------------------- */
int psn_mf_shade_fwd(const float* light_dir, const float* view, const float* normal, const float* albedo,
                     const float* rough, const float* light_int, float light_int_scalar, float f0, const float* vis,
                     int L, int64_t Ns, float* rgb, void* stream);
int psn_mf_shade_bwd(const float* light_dir, const float* view, const float* normal, const float* albedo,
                     const float* rough, const float* light_int, float light_int_scalar, float f0, const float* vis,
                     int L, int64_t Ns, const float* g_rgb, float* d_albedo, float* d_rough, float* d_normal,
                     float* d_vis, float* d_light_dir, float* d_light_int, float* workspace, void* stream);

/* ------------------------------------------------------------------------
 * Stage-1 mesh extraction: stage1/model/extracting.py:75-206 with utils/libmise/mise.pyx (multi-resolution iso-surface
 * refinement) and utils/libmcubes/marchingcubes.h:23-193 (marching cubes, first variant), state resident on the device.
 *   grid   float32 [n, n, n], n = resolution + 1 points per axis, x-major; NaN = hole (no value yet)
 *   flags  one byte per grid point (0 = no grid point yet, 1 = pending, 2 = known), 4-byte aligned, padded with zero
 *          bytes to a multiple of 4
 *   vox    voxel states of the octree levels 0 .. depth - 1 back to back, level l = (resolution0 << l)^3 bytes x-major
 *          (0 = absent, 1 = leaf, 2 = split); level 0 starts as all leaves
 * Sizes beyond PSN_MESH_MAX_RESOLUTION return PSN_E_UNSUPPORTED.
 *
 * psn_mise_collect (mise.pyx:107-129 + extracting.py:105-108): the pending points as a compact list -- rows[r] = linear grid
 *   index, points[r] = box_size * ((float)i / (float)resolution - 0.5f) per axis, float32 in that order -- and their
 *   transition to known.  count[0] = number of pending points found (entries behind `capacity` are dropped).  The order of
 *   the list is not defined.  The list feeds psn_mlp_infer_pe_indirect (points, n_rows_dev = count, out_rows = rows, out = grid).
 * psn_mise_refine (mise.pyx:185-282): one round over every leaf of every level < depth, finest level first.  A leaf is active iff
 *   the known grid points of its closed cube hold a value >= threshold and a value <= threshold (double, both non-strict); it
 *   is split, its children become leaves, the points of its half-edge lattice that are no grid points yet become pending.
 *   pending[0] = number of points that became pending in this round; 0 ends the refinement.
 * psn_grid_ffill (mise.pyx:143-164, to_dense): in place, every hole takes its predecessor's value along x, then along y,
 *   then along z (three passes in that order; pure copies).
 * psn_mc_count (marchingcubes.h:59-72 on the grid padded by one layer of -1e6, extracting.py:170-171; the padding is
 *   virtual): cells (n + 1)^3, x-major; cube index bit m set iff value(v_m) <= threshold.  code[c] = bit a set iff the
 *   lattice edge from the cell's lower corner along axis a carries a vertex, | number of triangles << 3;
 *   block_v / block_t [psn_mc_blocks(n)] = vertices / triangles per run of 256 consecutive cells.
 * psn_mc_emit (marchingcubes.h:74-187, extracting.py:175-181): v_base / t_base = exclusive scans of those block sums,
 *   n_vertices / n_faces their totals.  vertices [n_vertices, 3] float64: x1 + (x2 - x1) (threshold - f1) / (f2 - f1) in
 *   double on the lattice edge, then box_size * ((v - 1) / (n - 1) - 0.5) (box_size <= 0: units of the padded lattice),
 *   ascending by (owning grid point x-major, axis); faces [n_faces, 3] int64 ascending by (cell x-major, order of the case
 *   table csrc/mc_table.h, which tools/gen_mc_table.py derives).  v_off: scratch, int32 [(n + 1)^3], uninitialised.
 * ---------------------------------------------------------------------- */
#define PSN_MESH_MAX_RESOLUTION 1024
int psn_mise_collect(unsigned char* flags, int resolution, float box_size, int64_t capacity, int64_t* rows, float* points,
                     long long* count, void* stream);
int psn_mise_refine(const float* grid, unsigned char* flags, unsigned char* vox, int resolution0, int depth, double threshold,
                    long long* pending, void* stream);
int psn_grid_ffill(float* grid, int n, void* stream);
int64_t psn_mc_blocks(int n);
int psn_mc_count(const float* grid, int n, double threshold, unsigned char* code, int* block_v, int* block_t, void* stream);
int psn_mc_emit(const float* grid, int n, double threshold, const unsigned char* code, const int64_t* v_base, const int64_t* t_base,
                int64_t n_vertices, int64_t n_faces, double box_size, int* v_off, double* vertices, int64_t* faces, void* stream);

/* ------------------------------------------------------------------------
 * Mesh evaluation: the point-to-mesh query behind the reference's Chamfer distance (chamfer_dist.py:19-35,
 * stage2/utils/metrics.py:79-113), i.e. what it asks of trimesh.proximity.closest_point (an r-tree on the host).  Here: a
 * uniform grid of triangle lists over the mesh's bounding box, built and queried on the device, float64 throughout.
 *   vertices  float64 [V, 3];  faces  int64 [F, 3], every index in 0 .. V - 1 (NOT checked here: the caller's duty),
 *             1 <= F <= PSN_TRI_GRID_MAX_FACES.  Zero-area and duplicated triangles are allowed and take part with their true
 *             distance (segment / point); no NaN arises from them.
 *   PsnTriGrid (host memory): lo / hi = the exact minimum / maximum of the vertices per axis (mesh units); cell = edge of the
 *             cubic cells (> 0, mesh units); n[a] = cells per axis, 1 .. PSN_TRI_GRID_MAX_CELLS_PER_AXIS, as a rule with
 *             lo[a] + n[a] cell >= hi[a].  A grid may stop short of hi (a small cell with n at its limit): a coordinate beyond
 *             lo[a] + n[a] cell belongs to the last cell n[a] - 1, for the builder and for every query alike, so the results
 *             are the same and only the last cell's lists grow (tests/test_trigrid_gpu.py builds such a grid).  Cell (i, j, k)
 *             has the linear index (i n[1] + j) n[2] + k.  max_span >= 1: a triangle
 *             whose bounding box overlaps more cells than this is kept in the oversize list instead of the cell lists.
 *   lists     int32 triangle ids.  The order within a cell's list and within the oversize list is not defined (atomics); the
 *             query's result does not depend on it.
 *   PsnMeshIndex (host memory, device pointers): the mesh and its built grid in one value, what every query takes.  cell_start
 *             [cells + 1] int32 = the exclusive scan of psn_tri_grid_count's counts with the total appended; list [n_entries] as
 *             psn_tri_grid_fill wrote it (may be null when n_over = F: no cell has an entry); over_list: its first n_over entries
 *             are the oversize triangles, 0 <= n_over <= F (may be null when n_over = 0).  A query refuses with PSN_E_ARG a null
 *             index, null vertices, faces or cell_start, F out of range, n_over or a null list against these rules, a bad grid.
 *
 * psn_tri_grid_count: cell_count [cells] int32 (zeroed here) = per cell, the triangles whose bounding box overlaps it;
 *   over_list [F] receives the oversize triangles, n_over[0] (set here) their number.
 * psn_tri_grid_fill: cursor [cells] int32 = the exclusive scan of those counts (advanced here to the inclusive scan);
 *   list [n_entries], n_entries = their total (< 2^31).
 * psn_closest_point: points float64 [Q, 3]; order = null or a permutation of 0 .. Q - 1 in which the points are worked on (sorted
 *   by home cell keeps a wave's lanes in neighbouring cells; outputs are written at the point's own row either way).  closest
 *   float64 [Q, 3], dist float64 [Q] (Euclidean, mesh units), tri int64 [Q]: the minimum over ALL triangles of the distance to
 *   the triangle as the closed convex hull of its corners, ties to the lowest triangle index -- bitwise reproducible.  The search
 *   walks shells of cells around the point's (clamped) home cell and stops by an exact bound (csrc/meshdist.hip), also for points
 *   outside the bounding box.  A point with a NaN coordinate gets NaN, NaN, -1.  n_tests: null, or an int64 counter to which the
 *   number of point-triangle tests is added.  Q = 0 is a no-op.
 * Errors: PSN_E_ARG for null pointers, Q out of range, a bad PsnTriGrid or PsnMeshIndex, n_entries >= 2^31; PSN_E_LAUNCH.
 * ---------------------------------------------------------------------- */
#define PSN_TRI_GRID_MAX_CELLS_PER_AXIS 256
#define PSN_TRI_GRID_MAX_FACES 2147483646LL
typedef struct {
    double lo[3];
    double hi[3];
    double cell;
    int n[3];
    int max_span;
} PsnTriGrid;
typedef struct {
    PsnTriGrid grid;
    const double* vertices; const int64_t* faces; int64_t n_faces;
    const int* cell_start; const int* list; const int* over_list; int64_t n_over;
} PsnMeshIndex;
int psn_tri_grid_count(const PsnTriGrid* grid, const double* vertices, const int64_t* faces, int64_t n_faces, int* cell_count,
                       int* over_list, long long* n_over, void* stream);
int psn_tri_grid_fill(const PsnTriGrid* grid, const double* vertices, const int64_t* faces, int64_t n_faces, int* cursor,
                      int64_t n_entries, int* list, void* stream);
int psn_closest_point(const PsnMeshIndex* index, const double* points, const int64_t* order, int64_t n_points, double* closest,
                      double* dist, int64_t* tri, long long* n_tests, void* stream);

/* ------------------------------------------------------------------------
 * Ray casting against the mesh, over the same index (csrc/meshray.hip; the float64 numpy definition is
 * psnerf_amd/meshdist.py:host_ray_cast).  The reference has no such query: its depth, normal and shadow maps all come from marching
 * the occupancy network.  index: the PsnMeshIndex (above).
 *
 * psn_ray_cast: origins / directions float64 [Q, 3] (directions need not be unit vectors: t is the parameter of o + t d); order =
 *   null or a permutation of 0 .. Q - 1 in which the rays are worked on (outputs are written at the ray's own row either way).
 *   The intersection test is the watertight one of Woop, Benthin and Wald (JCGT 2013), without back-face culling; a hit counts
 *   when t_min <= t <= t_max (either may be infinite; t_min <= t_max).  mode = PSN_RAY_FIRST_HIT: t float64 [Q], tri int64 [Q],
 *   bary float64 [Q, 3] or null, hit bytes [Q] = the minimum of (t, triangle index) in lexicographic order over ALL triangles the
 *   test accepts -- bitwise reproducible; a miss gives inf, -1, NaN, 0.  mode = PSN_RAY_ANY_HIT: hit only, the walk ends at the
 *   first accepted triangle; t, tri and bary receive the values of a miss.  A triangle of zero area or seen edge-on is never hit; a
 *   ray with a non-finite component or a zero direction misses.  n_tests: null, or an int64 counter to which the number of
 *   ray-triangle tests is added.  Q = 0 is a no-op.
 * Errors: PSN_E_ARG for null pointers, a bad PsnMeshIndex, Q out of range, an unknown mode, t_min > t_max; PSN_E_LAUNCH.
 * ---------------------------------------------------------------------- */
#define PSN_RAY_FIRST_HIT 0
#define PSN_RAY_ANY_HIT 1
int psn_ray_cast(const PsnMeshIndex* index, const double* origins, const double* directions, const int64_t* order, int64_t n_rays,
                 double t_min, double t_max, int mode, double* t, int64_t* tri, double* bary, unsigned char* hit, long long* n_tests,
                 void* stream);

/* ------------------------------------------------------------------------
 * Occlusion of surface rows by the mesh, over the same index (csrc/meshocclude.hip; the float64 numpy definition is
 * psnerf_amd/meshocclude.py:host_occlusion_rows): per row (a point and a normal) the K rays of a direction table are formed in
 * registers and walked through the grid by psn_ray_cast's own any-hit walk (csrc/meshray.h), so no ray is ever written to memory.
 * The reference has no such query.  index: the PsnMeshIndex (above).
 *
 * psn_occlusion_rows: points / normals float64 [R, 3], table float64 [K, 3], 1 <= K <= PSN_OCC_MAX_DIRS.  A row whose point or normal
 *   has a non-finite component, or whose normal is zero, casts nothing: hits = -1, visible = 0, ao = NaN, bent = 0, words = 0.
 *   Otherwise the origin is o = p + bias n (the products, then the sums) and direction k, (x, y, z) = table[k], is
 *     PSN_OCC_LOCAL  d = (x t + y b) + z n per component, (t, b) the branchless basis of Duff et al. about n:  s = n_z >= 0 ? 1 : -1,
 *                    a = -1 / (s + n_z), q = (n_x n_y) a, t = (1 + (s (n_x n_x)) a, s q, (-s) n_x), b = (q, s + (n_y n_y) a, -n_y);
 *                    every direction is cast;
 *     PSN_OCC_WORLD  d = table[k]; cast only when it faces the normal, (n0 d0 + n1 d1) + n2 d2 > 0.
 *   A cast direction is blocked when psn_ray_cast in mode PSN_RAY_ANY_HIT with t_min = 0 and this t_max reports a hit for (o, d).
 *   hits int32 [R] = the cast directions that are blocked; visible int32 [R] = those that are not; ao float64 [R] = 1 - hits / K'
 *   with K' = hits + visible (1 when K' = 0); bent float64 [R, 3] = the sum of the unblocked cast d in index order, divided by its
 *   length sqrt((m0 m0 + m1 m1) + m2 m2), zero where that is not > 0; words int32 [R, (K + 31) / 32] or null: bit k % 32 of word
 *   k / 32 is set iff direction k was cast and not blocked.  All arithmetic is float64 without contraction in the order written,
 *   so every output is bitwise reproducible and equal to the definition's.  n_tests: null, or an int64 counter to which the
 *   number of ray-triangle tests is added.  R = 0 is a no-op.
 * Errors: PSN_E_ARG for null pointers, a bad PsnMeshIndex, R or K out of range, an unknown mode, a bias that is not finite,
 *   t_max < 0 or NaN; PSN_E_LAUNCH.
 * ---------------------------------------------------------------------- */
#define PSN_OCC_LOCAL 0
#define PSN_OCC_WORLD 1
#define PSN_OCC_MAX_DIRS 1024
int psn_occlusion_rows(const PsnMeshIndex* index, const double* points, const double* normals, int64_t n_rows, const double* table,
                       int n_dirs, int mode, double bias, double t_max, int* hits, int* visible, double* ao, double* bent, int* words,
                       long long* n_tests, void* stream);

/* ------------------------------------------------------------------------
 * The views projected onto surface rows, over the same index (csrc/meshproject.hip; the float64 numpy definition is
 * psnerf_amd/meshproject.py:host_project_rows): per row (a point and a normal) which of V cameras see it, and the weighted sums of
 * what their images show there.  The segment to a camera is formed in registers and walked by psn_ray_cast's own any-hit walk
 * (csrc/meshray.h), so no ray and no per-(row, view) value is ever written to memory.  The reference has no such query.
 * index: the PsnMeshIndex (above).
 *
 * psn_project_rows: points / normals float64 [R, 3]; views float64 [V, 16], 1 <= V <= PSN_PROJECT_MAX_VIEWS, one row per view:
 *   R row-major (9, camera to world), o (3), K00, K02, K12, 0 (the table of psn_hull_points); images [V, H, W, C], PSN_IMG_U8 (a byte
 *   u is the double u / 255.0) or PSN_IMG_F32 (widened exactly), 1 <= H, W <= PSN_PROJECT_MAX_EXTENT, 1 <= C <=
 *   PSN_PROJECT_MAX_CHANNELS -- or images null and C = 0: visibility only, sum / sum_sq / best_value are not touched and may be
 *   null; masks uint8 [V, H, W] (non-zero = set) or null.
 *   A row whose point or normal has a non-finite component, or whose normal is zero, sees nothing: n_seen = 0, best_view = -1, every
 *   sum, weight and word 0.  Otherwise the views are taken in ascending order, and view v SEES the row iff
 *     1. d = p - o, x_c = (d0 R[0, c] + d1 R[1, c]) + d2 R[2, c], x_2 > 0, u = K02 + K00 (x_0 / x_2), v = K12 + K00 (x_1 / x_2);
 *     2. 0 <= u <= W - 1 and 0 <= v <= H - 1 (a NaN is outside); x0 = floor u, x1 = min(x0 + 1, W - 1), fx = u - x0, likewise y;
 *     3. e = o - p, c = ((n0 e0 + n1 e1) + n2 e2) / sqrt((e0 e0 + e1 e1) + e2 e2) > cos_min;
 *     4. with masks, the four pixels (y0 | y1, x0 | x1) of view v are all non-zero;
 *     5. psn_ray_cast in mode PSN_RAY_ANY_HIT with t in [0, 1] reports no hit for (q, o - q), q = p + bias n (the products, then
 *        the sums).
 *   Its sample per channel is val = (1 - fy)((1 - fx) t00 + fx t10) + fy ((1 - fx) t01 + fx t11); with
 *   PSN_PROJECT_FRAME_CAMERA_NORMAL (C = 3) val becomes w_i = (R[i, 0] val0 + R[i, 1] (-val1)) + R[i, 2] (-val2).  Its weight is
 *   w = c (PSN_PROJECT_WEIGHT_COSINE) or 1 (PSN_PROJECT_WEIGHT_UNIFORM).  In view order: sum[ch] += w val[ch];
 *   sum_sq[ch] += w (val[ch] val[ch]); weight += w; n_seen += 1; best_view = the seeing view of the largest w (a tie: the lowest),
 *   best_value = its val; bit v % 32 of word v / 32 is set.
 *   Outputs: sum, sum_sq, best_value float64 [R, C]; weight float64 [R]; n_seen, best_view int32 [R]; words int32 [R, (V + 31) / 32]
 *   or null.  All arithmetic is float64 without contraction in the order written and a row's views accumulate in one thread, so
 *   every output is bitwise reproducible and equal to the definition's.  n_tests: null, or an int64 counter to which the number of
 *   ray-triangle tests is added.  R = 0 is a no-op.
 * Errors: PSN_E_ARG for null pointers, a bad PsnMeshIndex, R, V, H, W or C out of range, C = 0 with images or C > 0 without, an
 *   unknown image type, weight mode or frame mode, PSN_PROJECT_FRAME_CAMERA_NORMAL with C != 3, a bias or cos_min that is not
 *   finite; PSN_E_LAUNCH.
 * ---------------------------------------------------------------------- */
#define PSN_PROJECT_MAX_VIEWS 256
#define PSN_PROJECT_MAX_EXTENT 32768
#define PSN_PROJECT_MAX_CHANNELS 4
#define PSN_PROJECT_WEIGHT_COSINE 0
#define PSN_PROJECT_WEIGHT_UNIFORM 1
#define PSN_PROJECT_FRAME_RAW 0
#define PSN_PROJECT_FRAME_CAMERA_NORMAL 1
int psn_project_rows(const PsnMeshIndex* index, const double* points, const double* normals, int64_t n_rows, const double* views,
                     int n_views, const void* images, int image_type, int H, int W, int C, const unsigned char* masks, double bias,
                     double cos_min, int weight_mode, int frame_mode, double* sum, double* sum_sq, double* weight, int* n_seen,
                     int* best_view, double* best_value, int* words, long long* n_tests, void* stream);

/* ------------------------------------------------------------------------
 * Crossing counts of an axis-parallel line with the mesh, over the same index (csrc/meshinside.hip; the float64 numpy definition is
 * psnerf_amd/meshdist.py:host_crossings): the inside test behind volume IoU.  The reference has no such query.  index: the
 * PsnMeshIndex (above).
 *
 * psn_mesh_crossings: points float64 [Q, 3]; order = null or a permutation of 0 .. Q - 1 in which the points are worked on (sorted
 *   by column, then by cell along the axis; outputs are written at the point's own row either way).  axis = 0, 1 or 2: the line
 *   through a point runs along it.  With kz = axis, kx = (axis + 1) % 3, ky = (axis + 2) % 3 the corners are translated by -p and
 *   U, V, W are the watertight test's edge functions without its shear; an edge function that is exactly 0 is decided by simulation
 *   of simplicity (p moved by (+d, +d^2) in (kx, ky)): sign(e), else sign(Qy - Py), else sign(Px - Qx).  The rule is antisymmetric
 *   in the edge's two ends, so of two triangles on opposite sides of a shared edge exactly one owns a point on it.  A triangle is
 *   accepted when p lies in the closed bounding box of its projection (exact; it keeps slivers whose U, V, W are rounding noise
 *   from counting far from where they are), the three sides are equal and non-zero and det = U + V + W != 0;
 *   z = (U Az + V Bz + W Cz) / det.
 *   above int32 [Q] = accepted triangles of the WHOLE mesh with z > 0; below int32 [Q] or null: z < 0; on int32 [Q] or null:
 *   z == 0 -- each triangle once, bitwise reproducible, independent of the order of the lists.  inside = above & 1;
 *   (above + below + on) & 1 = the line does not see a closed surface.  Without below the walk starts at the point's own cell;
 *   above and on do not change.  Zero-area and edge-on triangles are never counted; a point with a non-finite coordinate, or
 *   outside the bounding box in kx or ky, gets zeros.  n_tests: null, or an int64 counter to which the number of line-triangle
 *   tests is added (at most Q F).  Q = 0 is a no-op.
 * Errors: PSN_E_ARG for null pointers, an axis outside 0 .. 2, a bad PsnMeshIndex, Q out of range; PSN_E_LAUNCH.
 * ---------------------------------------------------------------------- */
#define PSN_CROSSINGS_MAX_POINTS 137438953408LL
int psn_mesh_crossings(const PsnMeshIndex* index, const double* points, const int64_t* order, int64_t n_points, int axis,
                       int* above, int* below, int* on, long long* n_tests, void* stream);

/* ------------------------------------------------------------------------
 * Mesh clean-up: connected components of a triangle mesh, per-component statistics and compaction (csrc/meshclean.hip; the numpy
 * definition is psnerf_amd/meshclean.py:host_*).  The reference has no such step (its only answer to floaters is --clip,
 * stage1/model/extracting.py:130-132); users of the pipeline take trimesh's split() on the host.
 *   vertices float64 [V, 3];  faces int64 [F, 3];  0 <= V <= PSN_CC_MAX_VERTICES, 0 <= F <= PSN_CC_MAX_FACES.  Duplicated faces and
 *   faces with a repeated index are legal.  A face with an index outside 0 .. V - 1 is SKIPPED and PSN_CC_E_INDEX is set in status.
 *   status  int32 [1] on the device, bits PSN_CC_E_*; the caller reads it with the table and raises.
 *
 * psn_cc_label: labels int32 [V], labels[v] = the smallest vertex index reachable from v (two vertices are adjacent when one face
 *   names both; an unreferenced vertex keeps its own index).  parent int32 [V]: scratch.  status is zeroed here.  One pass of a
 *   lock-free union-find and a flatten launch; no host read, no rounds; bitwise reproducible.  PSN_CC_E_BOUND: a loop ran into its
 *   static bound (labels are then not valid).
 * psn_cc_stats: per component, indexed by its label (all three arrays [V], zeroed here): vertex_count, face_count (a face belongs
 *   to the component of its first index) and area = the sum of 0.5 |(b - a) x (c - a)| in float64.  Counts are exact; the order of
 *   the area sum is not defined (within n 2^-53 relative of the exact sum of n faces).  status: bits are added.
 * psn_cc_flag: face_keep [F] bytes = keep_label[labels[first index]] != 0 (keep_label [V] bytes); vertex_keep [V] bytes (zeroed
 *   here) = 1 for every vertex a kept face names.
 * psn_cc_compact: face_pos [F] / vertex_pos [V] int64 = exclusive scans of those flags, n_out_* their totals.  out_vertices
 *   [n_out_vertices, 3] = the kept vertices in their original order, bits untouched; out_normals likewise from normals [V, 3] of
 *   normal_bytes = 4 (float) or 8 (double) per component, or null with normal_bytes = 0; out_faces [n_out_faces, 3] = the kept faces in
 *   their original order with vertex_pos applied.
 * Errors: PSN_E_ARG for null pointers and sizes out of range; PSN_E_LAUNCH.
 * ---------------------------------------------------------------------- */
#define PSN_CC_MAX_VERTICES 2147483646LL
#define PSN_CC_MAX_FACES 274877906944LL
#define PSN_CC_E_INDEX 1
#define PSN_CC_E_BOUND 2
int psn_cc_label(const int64_t* faces, int64_t n_faces, int64_t n_vertices, int* parent, int* labels, int* status, void* stream);
int psn_cc_stats(const double* vertices, const int64_t* faces, int64_t n_faces, int64_t n_vertices, const int* labels,
                 long long* vertex_count, long long* face_count, double* area, int* status, void* stream);
int psn_cc_flag(const int64_t* faces, int64_t n_faces, int64_t n_vertices, const int* labels, const unsigned char* keep_label,
                unsigned char* face_keep, unsigned char* vertex_keep, void* stream);
int psn_cc_compact(const double* vertices, const void* normals, int normal_bytes, const int64_t* faces, int64_t n_faces,
                   int64_t n_vertices, const unsigned char* face_keep, const unsigned char* vertex_keep, const int64_t* face_pos,
                   const int64_t* vertex_pos, int64_t n_out_faces, int64_t n_out_vertices, double* out_vertices, void* out_normals,
                   int64_t* out_faces, void* stream);

/* ------------------------------------------------------------------------
 * Mesh simplification: quadric vertex clustering on a uniform grid (csrc/meshsimplify.hip; the numpy definition, which these
 * kernels repeat operation for operation in float64, is psnerf_amd/meshsimplify.py:host_*).  The reference has no such step;
 * the extractor's lineage had one behind a native library (Occupancy Networks' simplify_nfaces).  The sorts and scans between
 * the kernels are the caller's (torch); compaction is psn_cc_compact on (positions, g).
 *   vertices float64 [V, 3], finite;  faces int64 [F, 3];  0 <= V <= PSN_CC_MAX_VERTICES, 0 <= F <= PSN_VC_MAX_FACES.
 *   grid     origin (ox, oy, oz) = the per-axis minimum of the vertices, cell edge h > 0, dims (dx, dy, dz) =
 *            floor(extent / h) + 1 per axis, each 1 .. PSN_VC_MAX_RESOLUTION + 1; computed by the caller on the host.
 *   status   int32 [1] on the device, bits PSN_VC_E_*, zeroed by the caller; the caller reads it with its counts and raises.
 *
 * psn_vc_cell_keys: keys int64 [V] = (c_z dy + c_y) dx + c_x with c_a = min(max(floor((v_a - origin_a) / h), 0), dims_a - 1).
 *   The caller's stable sort of the keys gives the clusters (the occupied cells ascending by key; cluster[v] = the rank of v's
 *   cell) and each cluster's vertex run in ascending vertex index.
 * psn_vc_face_keys: cluster int64 [V] -> g int64 [F, 3] = the faces re-indexed; face_keys int64 [F] = -1 for a face that names a
 *   cluster twice, else (g0' 2^21 + g1') 2^21 + g2' of the face rotated so that its smallest id comes first, orientation kept
 *   (equal keys are duplicates; the same three clusters in opposite orientation are not); corner_keys int64 [3 F] (or null:
 *   not written) = cluster * 3 F + 3 f + k per corner k, which sorted give every cluster its run of (face, corner) pairs in
 *   ascending order.  A face with an index outside 0 .. V - 1 is SKIPPED (key -1, g = 0, corner keys behind every run) and
 *   PSN_VC_E_INDEX is set; a cluster id outside 0 .. PSN_VC_MAX_CLUSTERS - 1 likewise with PSN_VC_E_CLUSTER (three ids
 *   share one 63-bit key: more clusters are refused by the caller).
 * psn_vc_solve: per cluster c (a wave each) -> positions float64 [C, 3], clamped bytes [C].  vertex_order int64 [V] = the
 *   stable sort's permutation, cell_key_sorted int64 [V] its keys, vertex_start int64 [C + 1] the run bounds in them;
 *   corner_sorted int64 [3 F] = the sorted corner keys, corner_start int64 [C + 1] their run bounds.
 *     x0 = (the sum of the run's vertices, one after the other) / count
 *     per (face, corner) of the run, in order, n = (b - a) x (c - a) unnormalised:  A += n n^T (six entries),
 *       r += n ((n_x (a_x - x0_x) + n_y (a_y - x0_y)) + n_z (a_z - x0_z)),  a = the face's first vertex
 *     t = (A00 + A11) + A22;  t == 0: x = x0;  else (A + regularisation t I) delta = r by the LDL^T sequence written out in
 *       meshsimplify.py, x = x0 + delta;  x clamped per axis into its cell [origin + c h, origin + (c + 1) h]; clamped[c] = 1
 *       where that moved a coordinate.
 *   Additions happen in exactly that order (lanes share the loads and the products, one lane owns each accumulator); no
 *   floating-point atomics; two runs give the same bits, and they are numpy's.
 * psn_vc_face_flags: face_keep bytes [F] (not degenerate, first of its key in face order) -> vertex_keep bytes [C] (zeroed
 *   here) = 1 for every cluster a kept face names; flipped bytes [F] = 1 for a kept face whose new normal
 *   (x[g1] - x[g0]) x (x[g2] - x[g0]) has a strictly negative dot product with its old one.
 * Errors: PSN_E_ARG for null pointers and bad arguments; PSN_E_UNSUPPORTED for sizes beyond the limits; PSN_E_LAUNCH.
 * ---------------------------------------------------------------------- */
#define PSN_VC_MAX_RESOLUTION 4096
#define PSN_VC_MAX_CLUSTERS 2097151
#define PSN_VC_MAX_FACES 274877906944LL
#define PSN_VC_E_INDEX 1
#define PSN_VC_E_CLUSTER 2
int psn_vc_cell_keys(const double* vertices, int64_t n_vertices, double ox, double oy, double oz, double h, int dx, int dy, int dz,
                     int64_t* keys, void* stream);
int psn_vc_face_keys(const int64_t* faces, int64_t n_faces, int64_t n_vertices, const int64_t* cluster, int64_t* corner_keys,
                     int64_t* face_keys, int64_t* g, int* status, void* stream);
int psn_vc_solve(const double* vertices, const int64_t* faces, int64_t n_faces, int64_t n_vertices, const int64_t* vertex_order,
                 const int64_t* vertex_start, const int64_t* cell_key_sorted, const int64_t* corner_sorted,
                 const int64_t* corner_start, int64_t n_clusters, double ox, double oy, double oz, double h, int dx, int dy, int dz,
                 double regularisation, double* positions, unsigned char* clamped, void* stream);
int psn_vc_face_flags(const double* vertices, const int64_t* faces, int64_t n_faces, int64_t n_vertices, const int64_t* g,
                      const double* positions, int64_t n_clusters, const unsigned char* face_keep, unsigned char* vertex_keep,
                      unsigned char* flipped, void* stream);

/* ------------------------------------------------------------------------
 * Mesh connectivity and smoothing: the edge table of a triangle mesh, vertex rings, per-vertex corner runs, vertex normals over
 * them, the lambda | mu (Taubin) smoothing step and the area / volume sums (csrc/meshtopo.hip; the numpy definitions, which these
 * kernels repeat operation for operation in float64, are psnerf_amd/meshtopo.py:host_* and psnerf_amd/meshsmooth.py:host_smooth).
 * The reference has none of it.  The stable sorts and the head-flag scan between the kernels are the caller's (torch).
 *   vertices float64 [V, 3];  faces int64 [F, 3];  0 <= V <= PSN_CC_MAX_VERTICES, 0 <= F <= PSN_CC_MAX_FACES.  A face with an index
 *   outside 0 .. V - 1 is SKIPPED and PSN_TOPO_E_INDEX is set in status (int32 [1] on the device, zeroed by the caller, who reads it
 *   with the counters and raises).  A face with a repeated index is degenerate: legal, and it contributes no half-edge.
 *
 * psn_topo_edge_keys: keys int64 [3 F]; half-edge h = 3 f + k of a non-degenerate face runs from a = f[k] to b = f[(k + 1) % 3] and
 *   has the key min(a, b) V + max(a, b); the three keys of a degenerate or skipped face are INT64_MAX, which sorts last.
 * psn_topo_edges: sorted_keys / order int64 [3 F] = the caller's STABLE sort of those keys and its permutation; rank_incl int64
 *   [3 F] = the inclusive scan of the head flags (a position is a head when its key is not INT64_MAX and differs from its
 *   predecessor's), n_edges = E its total.  -> edges int64 [E, 2] = (lo, hi) ascending by key; count int32 [E] = the half-edges of
 *   the run; forward int32 [E] = those with a < b; halfedge_edge int64 [3 F] = the rank of each half-edge's edge, -1 for INT64_MAX;
 *   vertex_used bytes [V] = 1 for every vertex of an edge, vertex_open bytes [V] = 1 for every vertex of an edge with count != 2
 *   (both zeroed here); counters int64 [4] (zeroed here) = edges with count == 1, with count > 2, with count == 2 and
 *   forward != 1, and degenerate (or skipped) faces.  Integer counters only: ballot + popcount per wave, one atomic per workgroup.
 * psn_topo_ring_keys: edges int64 [E, 2] -> keys int64 [2 E]: lo V + hi and hi V + lo.  Sorted, key / V owns the run and key % V is
 *   the neighbour: every neighbour once, ascending.
 * psn_topo_corner_keys: keys int64 [3 F], corner-major: keys[k F + f] = f[k] (V for a skipped face: behind every run).  The caller's
 *   stable sort gives every vertex its (corner, face) pairs in ascending (k, f); degenerate faces stay in the runs.
 * psn_topo_runs: sorted_keys int64 [n] ascending -> start int64 [V + 1], start[x] = the first position whose key / div is >= x (n where
 *   there is none; a key / div above V counts as V); rem int64 [n] (or null) = key % div, -1 for such a key.
 * psn_topo_vertex_normals: corner_start int64 [V + 1] and corner int64 [3 F] (values k F + f) from the two calls above -> normals
 *   float64 [V, 3]: from +0.0, per corner of the run in order, += (b - a) x (c - a) of its face (PSN_TOPO_WEIGHT_AREA) or that
 *   divided by its length sqrt((nx nx + ny ny) + nz nz), nothing for a face without length (PSN_TOPO_WEIGHT_UNIFORM); then divided by
 *   the sum's length formed the same way, zero where that is not > 0.
 * psn_topo_smooth_step: ring_start int64 [V + 1], ring int64 [n_ring] -> out [V, 3] (must not be x): per vertex with a non-empty
 *   ring of n neighbours and pinned[v] == 0 (pinned bytes [V], or null: none), per axis acc = +0.0, acc += x[w] in ring order,
 *   m = acc / n, out = x + s (m - x); every other vertex keeps its bits.
 * psn_topo_measures: out float64 [2] = the sum of 0.5 |(b - a) x (c - a)| and of (a . (b x c)) / 6 over the faces.  partial float64
 *   [2 PSN_TOPO_MEASURE_BLOCKS]: workspace; a fixed grid of per-workgroup sums and a fixed-order second step, so two calls give the
 *   same bits; the order of the sums is not numpy's (within F 2^-53 relative of the sum of the terms' absolute values).
 * Errors: PSN_E_ARG for null pointers and bad arguments; PSN_E_UNSUPPORTED for sizes beyond the limits; PSN_E_LAUNCH.
 * ---------------------------------------------------------------------- */
#define PSN_TOPO_E_INDEX 1
#define PSN_TOPO_WEIGHT_AREA 0
#define PSN_TOPO_WEIGHT_UNIFORM 1
#define PSN_TOPO_MEASURE_BLOCKS 1024
int psn_topo_edge_keys(const int64_t* faces, int64_t n_faces, int64_t n_vertices, int64_t* keys, int* status, void* stream);
int psn_topo_edges(const int64_t* sorted_keys, const int64_t* order, const int64_t* rank_incl, const int64_t* faces, int64_t n_faces,
                   int64_t n_vertices, int64_t n_edges, int64_t* edges, int* count, int* forward, int64_t* halfedge_edge,
                   unsigned char* vertex_used, unsigned char* vertex_open, long long* counters, void* stream);
int psn_topo_ring_keys(const int64_t* edges, int64_t n_edges, int64_t n_vertices, int64_t* keys, void* stream);
int psn_topo_corner_keys(const int64_t* faces, int64_t n_faces, int64_t n_vertices, int64_t* keys, int* status, void* stream);
int psn_topo_runs(const int64_t* sorted_keys, int64_t n_keys, int64_t div, int64_t n_vertices, int64_t* start, int64_t* rem,
                  void* stream);
int psn_topo_vertex_normals(const double* vertices, const int64_t* faces, int64_t n_faces, int64_t n_vertices,
                            const int64_t* corner_start, const int64_t* corner, int weight, double* normals, void* stream);
int psn_topo_smooth_step(const double* x, int64_t n_vertices, const int64_t* ring_start, const int64_t* ring, int64_t n_ring,
                         const unsigned char* pinned, double s, double* out, void* stream);
int psn_topo_measures(const double* vertices, const int64_t* faces, int64_t n_faces, int64_t n_vertices, double* partial, double* out,
                      void* stream);

/* ------------------------------------------------------------------------
 * Image evaluation: what the reference's evaluation.py computes per image pair and per view (csrc/imgmetrics.hip; the float64
 * numpy definition is psnerf_amd/imgmetrics.py:host_*).  float64 arithmetic, no floating-point atomics: each call writes one row
 * of partial sums per tile / chunk into ``partial`` (psn_img_workspace doubles; every row written on every call) and a second,
 * fixed-order step adds them, so two calls on the same input give the same bits everywhere.
 *   images   pred / gt [B, H, W, 3], both PSN_IMG_F32 (float) or both PSN_IMG_U8 (a byte u is the float32 value (float)u / 255.0f);
 *            PSN_IMG_MIN_EXTENT <= H, W <= PSN_IMG_MAX_EXTENT (the 11-tap window must fit), 1 <= B <= 65535.
 *   mask     bytes (0 / non-0) [mask_batch, H, W] with mask_batch = B or 1 (one mask for every image), or null = every pixel.
 *
 * psn_img_scale_sums: sums [B, 7] = per image the masked sums of pred * gt per channel (3), of pred * pred per channel (3) and the
 *   number of masked pixels (1): the terms of evaluation.py:15-24 (scale = mean over the channels of the quotients).
 * psn_img_metrics: the fused pass.  scale: null, or double [B]: pred becomes clip(pred * scale [b], 0, 1).  Then both images are
 *   composited onto white outside the mask.  ssim [B]: skimage's structural_similarity(data_range=1, channel_axis=2,
 *   gaussian_weights=True, sigma=1.5, use_sample_covariance=False) of the composited pair -- 11 taps, scipy's 'reflect' border,
 *   axis 0 filtered before axis 1, the mean over the map with a 5-pixel border cropped, per channel, then over the channels.
 *   psnr [B]: -10 log10 of the mean squared difference over the masked pixels and the three channels; 100 if that is 0.
 *   sums [B, 7]: cropped sum of the SSIM map per channel (3), masked squared error per channel (3), masked pixels (1).
 *   ssim_map: null, or double [B, H, W, 3], the uncropped map.
 * psn_normal_mae: pred / gt float [B, n_pixels, 3] normal maps; stage2/utils/metrics.py:17-37: v / (|v| + 1e-5) if normalize
 *   (a zero vector stays zero and gives 90 degrees), the dot product clipped to [-1, 1], acos in degrees.  sums [B, 2] = the
 *   masked sum of the errors and the number of masked pixels; err_map: null, or double [B, n_pixels], every pixel's error.
 * psn_img_workspace: the doubles ``partial`` must hold for (which, B, H, W) (normal MAE: H * W = n_pixels); -1 on a bad argument.
 * Errors: PSN_E_ARG for null pointers, an unknown image_type, sizes out of range, a mask batch that is neither 1 nor B; PSN_E_LAUNCH.
 * ---------------------------------------------------------------------- */
#define PSN_IMG_F32 0
#define PSN_IMG_U8 1
#define PSN_IMG_MIN_EXTENT 11
#define PSN_IMG_MAX_EXTENT 16384
#define PSN_IMG_WS_SCALE_SUMS 0
#define PSN_IMG_WS_METRICS 1
#define PSN_IMG_WS_NORMAL_MAE 2
int64_t psn_img_workspace(int which, int B, int H, int W);
int psn_img_scale_sums(const void* pred, const void* gt, int image_type, const unsigned char* mask, int mask_batch, int B, int H, int W,
                       double* partial, double* sums, void* stream);
int psn_img_metrics(const void* pred, const void* gt, int image_type, const unsigned char* mask, int mask_batch, const double* scale, int B,
                    int H, int W, double* partial, double* sums, double* ssim, double* psnr, double* ssim_map, void* stream);
int psn_normal_mae(const float* pred, const float* gt, const unsigned char* mask, int mask_batch, int normalize, int B, int64_t n_pixels,
                   double* partial, double* sums, double* err_map, void* stream);

/* ------------------------------------------------------------------------
 * Calibrated photometric stereo: one view's images under L known directional lights -> the normal map of the stage-1 normal loss, the
 * per-light intensities and light_avg.py's light-averaged image (csrc/photostereo.hip; the float64 numpy definition, with every step
 * and operation order, is psnerf_amd/photostereo.py:host_*).  float64 arithmetic in the definition's order; no floating-point atomics.
 *   images     [L, n_pixels, 3], PSN_IMG_U8 (a byte u is the double u / 255.0) or PSN_IMG_F32 (converted exactly);
 *              PSN_PS_MIN_LIGHTS <= L <= PSN_PS_MAX_LIGHTS, 1 <= n_pixels <= PSN_PS_MAX_PIXELS.
 *   mask       bytes (0 / non-0) [n_pixels], or null = every pixel.
 *   light_dir  double [L, 3], used as given (not normalised).
 *
 * psn_ps_normals: light_int null, or double [L, 3], the divisor per light and channel.  Per masked pixel: g[l] = (v0 + v1) + v2 with
 *   v = I / light_int; a light is lit if g > dark; the lit lights are ranked by g ascending, ties by light index, and light i is kept
 *   if floor(low n_lit) <= rank[i] < n_lit - floor(high n_lit); A = sum l l^T and b = sum l g over the kept lights in index order;
 *   m = adj(A) b; valid if kept >= min_lights, det A > cond t^3 (t = trace A / 3) and |m| > 0; normal = m / |m|; albedo [c] =
 *   sum v[l, c] s[l] / sum s[l]^2, s = max(n . l, 0) over the kept lights.  Outputs, written for every pixel: normal / albedo double
 *   [n_pixels, 3], valid bytes [n_pixels], kept int32 [n_pixels] (the kept count of a masked pixel); an invalid or unmasked pixel gets
 *   zeros.  They equal the definition bit for bit on either path: PSN_PS_PATH_TILE keeps the wave's g tile in LDS
 *   (L <= PSN_PS_TILE_LIGHTS), PSN_PS_PATH_REFORM re-forms g from the images (any L), PSN_PS_PATH_AUTO picks TILE where it fits.
 * psn_ps_light_intensity: intensity [L, 3] = sum_p I m / sum_p m^2 with m = albedo [p, c] max(n_p . l, 0) over the pixels with a
 *   non-0 valid byte whose I [l, p, c] lies in the open interval (dark, bright); 0 where the denominator is 0.  sums [L, 6] = the three
 *   numerators and the three denominators.  Each workgroup writes one row of six partial sums into ``partial`` (psn_ps_workspace
 *   doubles; every row on every call) and a second, fixed-order step adds them: two calls on the same input give the same bits.
 * psn_ps_light_average: light_avg.py:58-67.  limg [l] = I * mask, divided by relat_int [l, c] (double [L, 3]) unless that is null;
 *   mean double [n_pixels, 3] = the sequential sum over l divided by L; mean_u8 = round-half-even(clip(mean, 0, 1) * 255); norm_u8
 *   null, or bytes [L, n_pixels, 3] = the same rounding of every limg [l].
 * psn_ps_workspace: the doubles ``partial`` must hold for (L, n_pixels); -1 on a bad argument.
 * Errors: PSN_E_ARG for null pointers, L or n_pixels out of range, an unknown image_type or path, PSN_PS_PATH_TILE with
 *   L > PSN_PS_TILE_LIGHTS, low or high outside [0, 1) or low + high >= 1, min_lights < PSN_PS_MIN_LIGHTS; PSN_E_LAUNCH.
 * ---------------------------------------------------------------------- */
#define PSN_PS_MAX_LIGHTS 256
#define PSN_PS_MIN_LIGHTS 3
#define PSN_PS_TILE_LIGHTS 96
#define PSN_PS_MAX_PIXELS 1073741824
#define PSN_PS_PATH_AUTO 0
#define PSN_PS_PATH_TILE 1
#define PSN_PS_PATH_REFORM 2
int64_t psn_ps_workspace(int L, int64_t n_pixels);
int psn_ps_normals(const void* images, int image_type, const unsigned char* mask, const double* light_dir, const double* light_int, int L,
                   int64_t n_pixels, double low, double high, double dark, int min_lights, double cond, int path, double* normal,
                   double* albedo, unsigned char* valid, int32_t* kept, void* stream);
int psn_ps_light_intensity(const void* images, int image_type, const double* normal, const double* albedo, const unsigned char* valid,
                           const double* light_dir, int L, int64_t n_pixels, double dark, double bright, double* partial, double* sums,
                           double* intensity, void* stream);
int psn_ps_light_average(const void* images, int image_type, const unsigned char* mask, const double* relat_int, int L, int64_t n_pixels,
                         double* mean, unsigned char* mean_u8, unsigned char* norm_u8, void* stream);

/* ------------------------------------------------------------------------
 * Baking a per-point field onto a mesh: the texel <-> surface maps of the two-faces-per-cell atlas (csrc/meshbake.hip; the numpy
 * definition, which is THE definition, is psnerf_amd/meshbake.py: Atlas, host_atlas_points, host_atlas_scatter, host_atlas_sample).
 * The atlas (T, cell, n_faces): a T x T texture of G = T / cell cells per side, PSN_ATLAS_MIN_CELL <= cell <= T <= PSN_ATLAS_MAX_SIZE,
 * G * G >= ceil(n_faces / 2); n = cell - 3, K = (n + 2)(n + 3) / 2 rows per face.  Face f: cell q = f / 2 with origin ((q % G) cell,
 * (q / G) cell), half f % 2; local texel (i, j), i + j <= n + 1, is texel (X0 + i, Y0 + j) in half 0 and (X0 + cell - 1 - i,
 * Y0 + cell - 1 - j) in half 1 (x = column, y = row of the array); its row is f K + j (n + 2) - j (j - 1) / 2 + i.  Corners: (0, 0),
 * (n, 0), (0, n).  All float64 arithmetic is the definition's, in its order: every output equals the definition bit for bit.
 *
 * psn_atlas_points: vertices double [V, 3], faces int64 [F, 3], vertex_normals null or double [V, 3]; for the rows of the faces
 *   f0 <= f < f1: points double [(f1 - f0) K, 3] = (v0 + (i / n) e1) + (j / n) e2 (gutter rows continue the plane beyond the
 *   hypotenuse, unclamped), points_f32 = the same rounded once to float, normals double = normalise((b0 n0 + b1 n1) + b2 n2) with
 *   b = (1 - (i + j) / n, i / n, j / n), or normalise(e1 x e2) without vertex normals; a zero vector stays zero.  A face with a
 *   vertex index outside 0 .. V - 1 gives NaN rows.
 * psn_atlas_scatter: rows float [(f1 - f0) K, C] -> the texels of the faces f0 <= f < f1 of texture [T, T, C], PSN_IMG_F32 (copied) or
 *   PSN_IMG_U8 (in float: clip to [0, 1], x 255, round half to even; NaN -> 0).  No other texel is written.
 * psn_atlas_fill: every texel that NO face owns (cell diagonals, the free half of a last cell, free cells, the margin beyond G cell)
 *   := fill (through the same rule for PSN_IMG_U8); owned texels are left alone.
 * psn_atlas_sample: face int64 [Q], bary double [Q, 3] in the corner order of psn_ray_cast, texture float [T, T, C] -> out double
 *   [Q, C]: (x, y) = (b0 (x0, y0) + b1 (x1, y1)) + b2 (x2, y2) over the corner texels; x0 = clamp(floor x, 0, T - 1), x1 = min(x0 + 1,
 *   T - 1), fx = x - floor x, likewise y; out = (1 - fy)((1 - fx) t00 + fx t10) + fy ((1 - fx) t01 + fx t11) in double.  A face
 *   outside 0 .. n_faces - 1 (a miss is -1) or a position that is not finite gives a NaN row.
 * Errors: PSN_E_ARG for null pointers, sizes, channel counts or face ranges out of range, an unknown texture_type; PSN_E_LAUNCH.
 * ---------------------------------------------------------------------- */
#define PSN_ATLAS_MIN_CELL 4
#define PSN_ATLAS_MAX_SIZE 32768
#define PSN_ATLAS_MAX_CHANNELS 32
int psn_atlas_points(const double* vertices, int64_t n_vertices, const int64_t* faces, int64_t n_faces, const double* vertex_normals, int T,
                     int cell, int64_t f0, int64_t f1, double* points, float* points_f32, double* normals, void* stream);
int psn_atlas_scatter(const float* rows, int C, int T, int cell, int64_t n_faces, int64_t f0, int64_t f1, void* texture, int texture_type,
                      void* stream);
int psn_atlas_fill(float fill, int C, int T, int cell, int64_t n_faces, void* texture, int texture_type, void* stream);
int psn_atlas_sample(const int64_t* face, const double* bary, int64_t n_queries, const float* texture, int C, int T, int cell,
                     int64_t n_faces, double* out, void* stream);

/* ------------------------------------------------------------------------
 * Silhouette carving: dilated object masks, the visual-hull test of points and of the lattice of a value grid (csrc/hull.hip; the
 * numpy definition, which is THE definition, is psnerf_amd/hull.py: host_dilate, host_project, host_carve_points, host_carve_grid).
 *   masks      bytes [V, H, W], non-0 = set; V, H, W >= 1.
 *   views      double [V, 16] on the device: world_mat[:3, :3] row-major (9), world_mat[:3, 3] (3), K[0, 0], K[0, 2], K[1, 2], 0
 *              (world_mat = camera to world, K in pixel units; hull._views builds the table).
 *
 * psn_mask_dilate: half_widths = a HOST table of 2 r + 1 half-widths w[dy], dy = -r .. r, 0 <= w <= r <= PSN_HULL_MAX_RADIUS;
 *   out[v, y, x] = OR over dy, |dx| <= w[dy] of the mask at (y + dy, x + dx), bytes 0 / 1, where a pixel outside the image has the
 *   value ``border``.  invert = 1: the input is negated before and the output after (with border = 1: the erosion).  workspace:
 *   psn_mask_dilate_workspace(V, H, W) 8-byte words on the device (-1 on a bad argument), the bit-packed rows.  Exact for every size.
 * psn_hull_points: points [n_points, 3], PSN_HULL_F32 (widened exactly) or PSN_HULL_F64.  Per point and view, in float64, each
 *   product and sum one operation: d = p - o; x_c = (d0 R[0, c] + d1 R[1, c]) + d2 R[2, c]; u = K[0, 2] + K[0, 0] (x_0 / x_2),
 *   v = K[1, 2] + K[0, 0] (x_1 / x_2); the image contains the point if x_2 > 0, 0 <= floor(u + 0.5) < W and 0 <= floor(v + 0.5) < H.
 *   carved_by int32 [n_points] = the lowest view whose image contains the point and whose mask is 0 at (floor(v + 0.5), floor(u + 0.5)),
 *   -2 if no image contains it, else -1; keep bytes [n_points] = (carved_by == -1).  The views are taken PSN_HULL_VIEW_CHUNK at a
 *   time, chained inside the launch: V has no upper bound.
 * psn_hull_grid: the same for the lattice point (axis[x], axis[y], axis[z]) of every element of grid float [n, n, n] (x-major; axis
 *   double [n]): ``value`` is stored where the point is not kept, no other element is written; the number stored is ADDED to *count
 *   (the caller zeroes it).  2 <= n <= PSN_MESH_MAX_RESOLUTION + 1.
 * Errors: PSN_E_ARG for null pointers, V < 1, H or W < 1, n out of range, r out of range, border or invert not 0 / 1, a negative
 *   half-width or one above r, an unknown point_type; PSN_E_LAUNCH.
 * ---------------------------------------------------------------------- */
#define PSN_HULL_MAX_RADIUS 64
#define PSN_HULL_VIEW_CHUNK 32
#define PSN_HULL_F32 0
#define PSN_HULL_F64 1
int64_t psn_mask_dilate_workspace(int V, int H, int W);
int psn_mask_dilate(const unsigned char* masks, int V, int H, int W, const int32_t* half_widths, int r, int border, int invert,
                    unsigned long long* workspace, unsigned char* out, void* stream);
int psn_hull_points(const void* points, int point_type, int64_t n_points, const double* views, int V, const unsigned char* masks, int H,
                    int W, unsigned char* keep, int32_t* carved_by, void* stream);
int psn_hull_grid(float* grid, int n, const double* axis, const double* views, int V, const unsigned char* masks, int H, int W, float value,
                  unsigned long long* count, void* stream);

/* ------------------------------------------------------------------------
 * Mesh registration, trimmed point-to-plane ICP: the device steps of one iteration that are not a mesh query (csrc/meshalign.hip; the
 * numpy definition, which is THE definition and states every operation order, is psnerf_amd/meshalign.py: host_transform, host_dist,
 * host_sums).  float64 arithmetic in the definition's order; no floating-point atomics.  0 <= n <= PSN_ALIGN_MAX_ROWS.
 *
 * psn_align_transform: points double [n, 3] -> out [n, 3] = s (R x) + t, row i of R x = (R[i,0] x0 + R[i,1] x1) + R[i,2] x2, then the
 *   product with s, then the sum with t[i]: bit for bit the definition.  rotation (9, row-major) and translation (3) are HOST tables.
 * psn_align_dist: dist [n] = sqrt((dx dx + dy dy) + dz dz) with (dx, dy, dz) = Y - P, bit for bit: the distances whose order statistic
 *   is the trim's max_dist.
 * psn_align_sums: rows P, Y double [n, 3], tri int64 [n] and the mesh (vertices double [V, 3], faces int64 [F, 3]) whose triangle
 *   normals are meant; rotation = null, or a HOST table of 9 doubles applied to the unit normal.  Per row: N = normalise(e1 x e2) of
 *   triangle tri (rotated); the row is skipped as (1) no triangle / not finite when tri is outside 0 .. F - 1, a coordinate of P or Y
 *   is not finite or the face names a vertex outside 0 .. V - 1, else as (2) zero normal when |e1 x e2| is not > 0, else as (3) beyond
 *   max_dist unless |Y - P| <= max_dist (closed: a tie is kept).  For the used rows, with J = [P x N (3), N (3), P . N] and
 *   r = N . (Y - P): sums [PSN_ALIGN_SUMS] = the upper triangle of sum J J^T row by row (28), sum J r (7), sum r r, sum |Y - P|^2;
 *   counts int64 [PSN_ALIGN_COUNTS] = used, then the three skip counts in the order above; the counts are exact.  Each workgroup
 *   writes one partial row per PSN_ALIGN_CHUNK rows into ``partial`` (psn_align_workspace 8-byte words; every row on every call) and
 *   a second, fixed-order step adds them: two calls on the same input give the same bits.
 * psn_align_workspace: the 8-byte words ``partial`` must hold for n rows; -1 on a bad argument.
 * Errors: PSN_E_ARG for null pointers, n out of range, V or F < 1, a max_dist that is negative or NaN; PSN_E_LAUNCH.
 * ---------------------------------------------------------------------- */
#define PSN_ALIGN_MAX_ROWS 1073741824
#define PSN_ALIGN_CHUNK 1024
#define PSN_ALIGN_SUMS 37
#define PSN_ALIGN_COUNTS 4
int64_t psn_align_workspace(int64_t n);
int psn_align_transform(const double* points, int64_t n, double scale, const double* rotation, const double* translation, double* out,
                        void* stream);
int psn_align_dist(const double* P, const double* Y, int64_t n, double* dist, void* stream);
int psn_align_sums(const double* P, const double* Y, const int64_t* tri, int64_t n, const double* vertices, int64_t n_vertices,
                   const int64_t* faces, int64_t n_faces, const double* rotation, double max_dist, double* partial, double* sums,
                   int64_t* counts, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PSNERF_HIP_H */
