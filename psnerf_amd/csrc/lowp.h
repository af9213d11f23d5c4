// Host helpers and vector types shared by the two reduced-precision engines (mlp_infer_bf16.hip, mlp_infer_x3.hip): what their
// five entry points check of a PsnBf16Desc, the input-layer count, and the launch of a kernel that needs more dynamic LDS than
// the default limit.
#pragma once
#include "common.h"

namespace psn {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float floatx2 __attribute__((ext_vector_type(2)));
typedef int intx4 __attribute__((ext_vector_type(4)));

// The rules every engine form has: min_hidden..PSN_MLP_MAX_LAYERS hidden layers, 1..32 outputs, a known output activation and
// -- layer0_in -- a first layer that reads the input block.
inline int lowp_check_desc(const PsnBf16Desc& d, const char* what, int min_hidden, bool layer0_in) {
    PSN_CHECK_ARG(d.n_hidden >= min_hidden && d.n_hidden <= PSN_MLP_MAX_LAYERS, "%s: n_hidden=%d", what, d.n_hidden);
    PSN_CHECK_ARG(d.n_out >= 1 && d.n_out <= 32, "%s: n_out=%d", what, d.n_out);
    PSN_CHECK_ARG(d.out_act >= PSN_OUT_NONE && d.out_act <= PSN_OUT_OCC, "%s: out_act=%d", what, d.out_act);
    PSN_CHECK_ARG(!layer0_in || d.has_in[0] != 0, "%s: layer 0 must read the input block", what);
    return PSN_OK;
}

// hidden layers that read the input block
inline unsigned lowp_n_in(const PsnBf16Desc& d) {
    unsigned n = 0;
    for (int l = 0; l < d.n_hidden; ++l) n += d.has_in[l] != 0;
    return n;
}

// > 64 KB of dynamic LDS need the opt-in attribute; set per call (per-device state, cheap, no static flag to race on)
template <typename Args>
int lowp_launch(void (*kernel)(Args), const Args& a, int64_t blocks, int threads, size_t lds_bytes, void* stream, const char* what) {
    PSN_CHECK_ARG(blocks < (1ll << 31), "%s: too many rows", what);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e != hipSuccess) {
        set_error("%s: cannot reserve %zu bytes of LDS: %s", what, lds_bytes, hipGetErrorString(e));
        return PSN_E_LAUNCH;
    }
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(threads), lds_bytes, (hipStream_t)stream, a);
    PSN_CHECK_LAUNCH(what);
    return PSN_OK;
}

}  // namespace psn
