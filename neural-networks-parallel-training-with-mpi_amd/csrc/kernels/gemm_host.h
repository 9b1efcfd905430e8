// Host side of the bf16 GEMM family that gemm_bf16.hip shares with csrc/experiments: the weak
// references to the experiment entry points, the gemm_host helpers and two small launch helpers.
// (gemm_tiles.h is the device side.)
#pragma once
#include "gemm_tiles.h"

namespace nnmpi {

// ---- experiment kernels (csrc/experiments/gemm_experiments.hip) ------------------------------
// Built into the library only with NNMPI_BUILD_EXPERIMENTS=1 (_build.py); weak references here,
// so a production build links without them and every entry point below is a null pointer.
// variant 19..24: the deep-ring twin of the 256x256 kernel (docs/PERF.md §4)
__attribute__((weak)) hipError_t exp_pp256_ring(int variant, int la, int lb, int epi, int act,
                                                int bg, GemmParams p, dim3 grid, hipStream_t s);
// gemm_bf16_pp256_pair_kernel (off by default even when built: NNMPI_PAIR=1)
__attribute__((weak)) void exp_set_wide_pair(int on);
__attribute__((weak)) bool exp_wide_pair_wgrad_ok(int rows, int out_f, int in_f);
__attribute__((weak)) bool exp_wide_pair_dgrad_ok(int rows, int out_f, int in_f);
__attribute__((weak)) hipError_t exp_wide_pair(const WgradArgs& w1, const DgradArgs* dg,
                                               const WgradArgs* w2, hipStream_t s);
__attribute__((weak)) hipError_t exp_fwd_stamped(const bf16* X, int ldx, const bf16* W, int ldw,
                                                 const float* bias, bf16* Y, int ldy, int M, int N,
                                                 int K, unsigned long long* stamps, hipStream_t s);

// ---- host helpers shared with csrc/experiments (defined in gemm_bf16.hip) ----
namespace gemm_host {
// the weight-gradient GEMM of a WgradArgs and its pending split-K combine (returns the splits)
int make_wgrad(const WgradArgs& a, GemmParams& p, SlabReduce& pending);
int pick_tile(int M, int N);
int wgrad_tile(int M, int N);
// the production kernel selection is in effect (LDS-DMA path, no forced tile or variant)
bool default_path();
}  // namespace gemm_host

template <int LA, int LB>
static inline void set_extents(GemmParams& p) {
  // storage extents (bytes) of the operands, for the buffer-resource range checks
  const long long a = (LA == KMAJ) ? ((long long)(p.M - 1) * p.lda + p.K) : ((long long)(p.K - 1) * p.lda + p.M);
  const long long b = (LB == KMAJ) ? ((long long)(p.N - 1) * p.ldb + p.K) : ((long long)(p.K - 1) * p.ldb + p.N);
  p.a_bytes = (unsigned)std::min<long long>(a * 2, DMA_OOB - 16);
  p.b_bytes = (unsigned)std::min<long long>(b * 2, DMA_OOB - 16);
}

// hipFuncAttributeMaxDynamicSharedMemorySize of a kernel picked at run time from a table: set
// the first time each kernel pointer is seen
inline void dyn_lds_once(const void* f, int bytes) {
  static const void* done[64] = {};
  for (const void*& a : done) {
    if (a == f) return;
    if (!a) { a = f; break; }
  }
  (void)hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
}

}  // namespace nnmpi
