// bf16 "NT" GEMM for gfx950 with fused epilogues:  C[M,N] = A[M,K] · B[N,K]ᵀ  (+ epilogue)
//
// Both operands are K-contiguous row-major — the layout of every BERT projection in the forward
// (x · Wᵀ) and, with the transposed bf16 weight copy kept by the ParamStore, of every dgrad
// (dy · W = dy · (Wᵀ)ᵀ).  Epilogues fuse what used to be separate HBM passes (the math: hq_gemm_epi.h):
//   EPI_NONE   C = acc
//   EPI_BIAS   C = acc + bias[n]
//   EPI_GELU   P = acc + bias[n] (stored, needed by backward),  C = gelu_erf(P)
//   EPI_DGELU  C = acc · gelu'(P[m,n])  and per-block column sums of C (the bias gradient of the
//              producing Linear) into part[M/BM][N]  — replaces the separate gelu_bwd pass
//   EPI_RESID  C = acc + R[m,n]  (residual-gradient add of dgrad)
//   EPI_GELUD  as EPI_GELU but P receives gelu'(pre) instead of pre: the forward already evaluates
//              Φ and φ, so the derivative costs one FMA here and saves the backward ~15 VALU/element
//   EPI_DMUL   C = acc · P[m,n] (P = stored gelu') + column partials — the backward of EPI_GELUD
//
// This file is the dispatch only.  The kernels, one family per file, each behind one host entry of hq_gemm_nt.h:
//   gemm_nt_v1.hip  256×BN tiles, whole-tile double buffer        gemm_nt_vs.hip  128² tiles, M tails, split-K
//   gemm_nt_v2.hip  256² tiles, four halves in flight per K-tile   gemm_nt_v3.hip  v2's pipeline, persistent
// and the tile core they share in hq_gemm_tile.h.
#include "hq_gemm_nt.h"
#include "hq_gemm_tile.h"

namespace {

using hq_tile::BK;
using hq_tile::BM;

// 0 = auto (v3 for K <= 2304, else v2), 1 = force v1, 2 = force v2, 3 = force v3, 4 = force vS; set only by
// the tests / lab tools through hq_gemm_set_variant (no environment knob)
int g_gemm_variant = 0;

// Half-tile tail of v3 and v2: the last wave of `grid` 256² tiles is at most half full (and not the only wave), so
// its tiles run as 128-row halves.  Column partials are per 256-row block: those epilogues never split.
bool half_tile_tail(int epi, int grid) {
  const int ncu = hq_num_cus(), rt = grid % ncu;
  return (hq_nt_v3_flags() & kHqNtHalfTail) && !hq_epi_col_partials(epi) && rt > 0 && 2 * rt <= ncu && grid > ncu;
}

// the kernel family for block width bn (hq_gemm_nt_supported's answer: 1 = vS, 256 / 128 = the 256-row kernels)
void launch(int epi, const HqNtArgs& a, int bn, float* ws, hipStream_t s) {
  if (bn == 1) return hq_nt_vs_launch(epi, a, ws, s);
  const int K = a.K, grid = (a.M / BM) * (a.N / bn);
  const bool srd_ok = (size_t)BM * a.lda * 2 < (1ull << 31) && (size_t)256 * a.ldb * 2 < (1ull << 31);
  const bool pipelined = bn == 256 && K >= 2 * BK && srd_ok;   // v2 / v3: 256² tiles, a two-K-tile prologue
  // v3 (persistent, pipelined across tiles) where the per-tile fixed cost matters: K <= 2304 (+2-6 % at
  // K = 768 / 2304 on the b256 shapes, -1-3 % at K = 3072: tools/gemm_nt3_check.py, profiles/s3_gemm_v3)
  // (and at any K when the half-tile tail applies: at K = 3072 v3 + tail beat v2 + tail by 0.2-2.8 % on two
  // boxes, profiles/r3_halftail)
  const bool tail = half_tile_tail(epi, grid);
  const bool v3_auto = g_gemm_variant == 0 && (K <= 2304 || tail);
  if (pipelined && (g_gemm_variant == 3 || v3_auto)) hq_nt_v3_launch(epi, a, s);
  else if (pipelined && (g_gemm_variant == 0 || g_gemm_variant == 2 || g_gemm_variant == 3)) hq_nt_v2_launch(epi, a, tail, s);
  else hq_nt_v1_launch(epi, a, bn, s);   // N % 256 != 0 (128-wide blocks), K = 64, or forced
}

}  // namespace

void hq_gemm_set_variant(int v) { g_gemm_variant = v; }

// Kernel family for a shape: 256 / 128 = the 256-row kernels with that block width, 1 = vS (128² tiles),
// 0 = unsupported.  Variants 1-3 force the 256-row kernels where they apply, 4 forces vS; auto takes the
// 256-row kernels when M % 256 == 0 and their grid fills >= 80 % of the CUs' last wave, else vS.
int hq_gemm_nt_supported(int M, int N, int K) {
  if (M <= 0 || K % BK || K < BK || N % 128) return 0;
  const int big = (M % BM == 0) ? (N % 256 == 0 ? 256 : 128) : 0;
  if (g_gemm_variant == 4 || !big) return 1;
  if (g_gemm_variant != 0) return big;
  const int ncu = hq_num_cus();
  const long tiles = (long)(M / BM) * (N / big);
  const long waves = (tiles + ncu - 1) / ncu;
  return tiles * 5 >= waves * ncu * 4 ? big : 1;
}

int hq_gemm_nt_part_rows(int M, int N, int K) {
  const int k = hq_gemm_nt_supported(M, N, K);
  return k == 1 ? (M + 127) / 128 : M / BM;
}

size_t hq_gemm_nt_ws_floats(int M, int N, int K, int epi) {
  if (hq_gemm_nt_supported(M, N, K) != 1) return 0;   // split-K exists on the 128² (vS) kernel only
  const int grid_s = ((M + 127) / 128) * (N / 128);
  const int ks = hq_nt_vs_ksplit(epi, grid_s, K / BK);
  return ks > 1 ? (size_t)ks * M * N : 0;
}

void hq_gemm_nt(const uint16_t* A, const uint16_t* B, uint16_t* C, const float* bias, uint16_t* P, const uint16_t* R,
                float* part, int M, int N, int K, int lda, int ldb, int ldc, int epi, int bn, hipStream_t s, float drop_p,
                uint32_t drop_seed, uint32_t drop_opid, float* ws) {
  HqDropArg dr{hq_drop_key(drop_seed, drop_opid), 0u, 1.f};
  if (epi == HQ_EPI_BDR && drop_p > 0.f) {
    dr.thr = hq_threshold(drop_p);
    dr.ks = hq_keep_scale(dr.thr);
  }
  launch(epi, HqNtArgs{A, B, C, bias, P, R, part, M, N, K, lda, ldb, ldc, dr}, bn, ws, s);
}
