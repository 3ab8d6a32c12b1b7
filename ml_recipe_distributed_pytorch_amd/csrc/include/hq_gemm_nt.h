// The bf16 NT GEMM's kernel families, as gemm_nt.hip (the dispatch behind hq_gemm_nt) sees them: one host entry
// per family, defined beside its kernels.  Private to csrc/kernels; the public API is hq_kernels.h.
#pragma once
#include <type_traits>
#include <utility>

#include "hq_common.h"
#include "hq_kernels.h"

// hq_gemm_nt's operands on the host.  The kernels keep plain parameter lists (launch() spells them out), so
// this never becomes a kernel argument.
struct HqNtArgs {
  const uint16_t *A, *B;
  uint16_t* C;
  const float* bias;
  uint16_t* P;
  const uint16_t* R;
  float* part;
  int M, N, K, lda, ldb, ldc;
  HqDropArg dr;

  // kern<<<grid, block, lds, s>>>(A, B, C, bias, P, R, part, M, N, K, lda, ldb, ldc, extra..., dr)
  template <class Kern, class... Extra>
  void launch(Kern kern, int grid, int block, size_t lds, hipStream_t s, Extra... extra) const {
    hipLaunchKernelGGL(kern, dim3(grid), dim3(block), lds, s, A, B, C, bias, P, R, part, M, N, K, lda, ldb, ldc, extra...,
                       dr);
  }
};

// f(std::integral_constant<int, EPI>) for the runtime epilogue code `epi`
template <class F, int... E>
void hq_with_epi(int epi, F&& f, std::integer_sequence<int, E...>) {
  ((epi == E ? f(std::integral_constant<int, E>{}) : (void)0), ...);
}
template <class F>
void hq_with_epi(int epi, F&& f) {
  hq_with_epi(epi, f, std::make_integer_sequence<int, HQ_EPI_BDR + 1>{});
}

// dynamic LDS of the per-tile 256-row kernels (v1, v2) at block width bn: two operand stages or the epilogue staging
constexpr size_t hq_nt_tile_lds(int bn) {
  const size_t stage = 2 * (size_t)(256 * 128 + bn * 128);
  const size_t epi = 8 * 128 * (size_t)(bn / 4 * 2 + 16);
  return stage > epi ? stage : epi;
}

// Each entry picks the EPI instantiation, raises its LDS limit once and launches on s.
void hq_nt_v1_launch(int epi, const HqNtArgs& a, int bn, hipStream_t s);   // gemm_nt_v1.hip; bn = 256 or 128
// gemm_nt_vs.hip: 128² tiles, any M; split-K into ws when hq_nt_vs_ksplit(...) > 1 and ws is given
void hq_nt_vs_launch(int epi, const HqNtArgs& a, float* ws, hipStream_t s);
int hq_nt_vs_ksplit(int epi, int tiles, int nk);
// gemm_nt_v2.hip; tail: the last, at most half-full wave of tiles runs as 128-row half tiles
void hq_nt_v2_launch(int epi, const HqNtArgs& a, bool tail, hipStream_t s);
// gemm_nt_v3.hip (persistent).  Its flag word (hq_gemm_set_stagger) carries the half-tile-tail switch that the
// dispatch reads for v2 as well.
void hq_nt_v3_launch(int epi, const HqNtArgs& a, hipStream_t s);
constexpr int kHqNtHalfTail = 1 << 16;
int hq_nt_v3_flags();
