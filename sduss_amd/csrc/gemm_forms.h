// Every kernel instantiation the GEMM / conv launchers can start, as X-macro lists.  An entry is T(id, kernel, (template arguments)) or
// P(id, kernel) for a kernel without template arguments.  The route in gemm_dispatch.cpp (form_of) names an id; each family's launcher
// starts it through one switch over its list, and mx_gemm_kernel_name / mx_gemm_kernel_names report the same entries by name
// ("gemm_v2_kernel<160, 2, true, EPI_F_ALL, false>": the kernel and its template arguments as written here).
#pragma once

#define MX_GEMM_GENERIC_FORMS(T)                          \
  T(GK_GEN64, gemm_kernel, (64, false))                   \
  T(GK_GEN64_CONV, gemm_kernel, (64, true))               \
  T(GK_GEN128, gemm_kernel, (128, false))                 \
  T(GK_GEN128_CONV, gemm_kernel, (128, true))

// gemm_bf16_v2.hip: 128-row tiles <BN, MI = 2, CONV, FEAT, GEGLU>
#define MX_GEMM_V2_FORMS(T)                                                    \
  T(GK_V2_128_GEGLU_ACT, gemm_v2_kernel, (128, 2, false, EPI_F_ACT, true))     \
  T(GK_V2_128_GEGLU, gemm_v2_kernel, (128, 2, false, 0, true))                 \
  T(GK_V2_160_CONV, gemm_v2_kernel, (160, 2, true, 0, false))                  \
  T(GK_V2_160_CONV_ALL, gemm_v2_kernel, (160, 2, true, EPI_F_ALL, false))      \
  T(GK_V2_128_CONV, gemm_v2_kernel, (128, 2, true, 0, false))                  \
  T(GK_V2_128_CONV_ALL, gemm_v2_kernel, (128, 2, true, EPI_F_ALL, false))      \
  T(GK_V2_160, gemm_v2_kernel, (160, 2, false, 0, false))                      \
  T(GK_V2_160_QKV, gemm_v2_kernel, (160, 2, false, EPI_F_QKV, false))          \
  T(GK_V2_160_ALL, gemm_v2_kernel, (160, 2, false, EPI_F_ALL, false))          \
  T(GK_V2_128, gemm_v2_kernel, (128, 2, false, 0, false))                      \
  T(GK_V2_128_QKV, gemm_v2_kernel, (128, 2, false, EPI_F_QKV, false))          \
  T(GK_V2_128_ALL, gemm_v2_kernel, (128, 2, false, EPI_F_ALL, false))

// gemm_bf16_v5.hip: 256-row tiles <BN, MI = 4, CONV, FEAT, GEGLU, VEC>
#define MX_GEMM_V5_FORMS(T)                                                           \
  T(GK_V5_128_GEGLU_ACT, gemm_v5_kernel, (128, 4, false, EPI_F_ACT, true, false))     \
  T(GK_V5_128_GEGLU, gemm_v5_kernel, (128, 4, false, 0, true, false))                 \
  T(GK_V5_160_CONV, gemm_v5_kernel, (160, 4, true, 0, false, false))                  \
  T(GK_V5_160_CONV_VEC, gemm_v5_kernel, (160, 4, true, 0, false, true))               \
  T(GK_V5_160_CONV_ALL, gemm_v5_kernel, (160, 4, true, EPI_F_ALL, false, true))       \
  T(GK_V5_128_CONV, gemm_v5_kernel, (128, 4, true, 0, false, false))                  \
  T(GK_V5_128_CONV_VEC, gemm_v5_kernel, (128, 4, true, 0, false, true))               \
  T(GK_V5_128_CONV_ALL, gemm_v5_kernel, (128, 4, true, EPI_F_ALL, false, true))       \
  T(GK_V5_160, gemm_v5_kernel, (160, 4, false, 0, false, false))                      \
  T(GK_V5_160_QKV, gemm_v5_kernel, (160, 4, false, EPI_F_QKV, false, false))          \
  T(GK_V5_160_ALL, gemm_v5_kernel, (160, 4, false, EPI_F_ALL, false, true))           \
  T(GK_V5_128, gemm_v5_kernel, (128, 4, false, 0, false, false))                      \
  T(GK_V5_128_QKV, gemm_v5_kernel, (128, 4, false, EPI_F_QKV, false, false))          \
  T(GK_V5_128_ALL, gemm_v5_kernel, (128, 4, false, EPI_F_ALL, false, true))

// gemm_bf16_v4.hip: the persistent 256 x 256 kernel <VEC, FEAT, GEGLU[, LN]>; LN = true: the folded LayerNorm's finalised statistics (ln_final)
#define MX_GEMM_V4_FORMS(T)                                                 \
  T(GK_V4_GEGLU_LN, gemm_v4_kernel, (false, 0, true, true))                 \
  T(GK_V4_QKV_LN, gemm_v4_kernel, (false, EPI_F_QKV, false, true))          \
  T(GK_V4_LN, gemm_v4_kernel, (false, 0, false, true))                      \
  T(GK_V4_GEGLU_ACT, gemm_v4_kernel, (false, EPI_F_ACT, true))              \
  T(GK_V4_GEGLU, gemm_v4_kernel, (false, 0, true))                          \
  T(GK_V4, gemm_v4_kernel, (false, 0, false))                               \
  T(GK_V4_QKV, gemm_v4_kernel, (false, EPI_F_QKV, false))                   \
  T(GK_V4_TANH, gemm_v4_kernel, (false, EPI_F_TANH, false))                 \
  T(GK_V4_VEC_ALL, gemm_v4_kernel, (true, EPI_F_ALL, false))                \
  T(GK_V4_VEC, gemm_v4_kernel, (true, 0, false))

// gemm_small_m.hip: M <= 16 as a weight stream <F32OUT[, WAVES]>
#define MX_GEMM_SMALL_M_FORMS(T)                                            \
  T(GK_SM_STREAM_F32, gemm_small_m_stream_kernel, (true))                   \
  T(GK_SM_STREAM, gemm_small_m_stream_kernel, (false))                      \
  T(GK_SM16_F32, gemm_small_m_kernel, (true, 16))                           \
  T(GK_SM16, gemm_small_m_kernel, (false, 16))                              \
  T(GK_SM4_F32, gemm_small_m_kernel, (true, 4))                             \
  T(GK_SM4, gemm_small_m_kernel, (false, 4))

// conv_small_n.hip
#define MX_GEMM_CONV_SMALL_FORMS(P)                                         \
  P(GK_CONV_SMALL_N, conv3x3_small_n_kernel)                                \
  P(GK_CONV_SMALL_CIN, conv3x3_small_cin_kernel)

#define MX_FORM_UNPAREN(...) __VA_ARGS__
#define MX_FORM_FIRST(x, ...) x        /* MX_FORM_FIRST targs: the first template argument (the tile's features BN of the tile kernels) */
#define MX_FORM_TARGS(...) "<" #__VA_ARGS__ ">"
#define MX_FORM_NAME_T(id, k, targs) #k MX_FORM_TARGS targs,
#define MX_FORM_NAME_P(id, k) #k,

namespace mx {
enum GemmKernelId {
#define MX_FORM_ID_T(id, k, targs) id,
#define MX_FORM_ID_P(id, k) id,
  MX_GEMM_GENERIC_FORMS(MX_FORM_ID_T) MX_GEMM_V2_FORMS(MX_FORM_ID_T) MX_GEMM_V5_FORMS(MX_FORM_ID_T) MX_GEMM_V4_FORMS(MX_FORM_ID_T)
  MX_GEMM_SMALL_M_FORMS(MX_FORM_ID_T) MX_GEMM_CONV_SMALL_FORMS(MX_FORM_ID_P)
#undef MX_FORM_ID_T
#undef MX_FORM_ID_P
  GK_COUNT
};
}  // namespace mx
