// The epilogue of the NT GEMMs, once: every kernel of gemm_nt_v1 / _vs / _v2 / _v3.hip turns a staged piece into its C
// piece, P piece and column sums with hq_epi_piece below, so "every variant computes the same C and P" is a
// property of the code.  Device code only; what differs per kernel stays with the kernel: where the staged piece
// and the operand piece come from, and how the stores are issued (v3: buffer stores with a cache policy and held
// data registers, the others plain pointers).  gemm_fp8.hip's epi_piece adds the fp8-only forms (the 8-bit gelu'
// code, the e4m3 / e5m2 copies, DMUL without fma contraction) and takes the rest from here.
#pragma once
#include "hq_common.h"
#include "hq_kernels.h"

// ---- the piece math: one 8-column bf16 piece of the staged tile -> the C piece, in place
// piece: the staged acc (+bias) piece in, the C piece out; the C store is the caller's.
// load_aux() -> the operand piece at the same place (DGELU: the stored pre-activation, DMUL: the stored gelu',
//   RESID / BDR: the residual).  Only these four call it, at the point where the kernels read the operand before,
//   so an instantiation without an operand never touches its (unfilled) operand registers.
// goff: the piece's element offset in C (the BDR dropout index); dr, key: the BDR dropout stream.
// csum: the lane's column sums (DGELU / DMUL).  Whether d·gd contracts into the sum is left to hipcc, per kernel,
//   as it always was (the partials are compared with a tolerance); gemm_fp8.hip's DMUL forbids it.
// store_p(const uint4&): GELU / GELUD hand it the P piece (pre-activation / gelu') before the C piece's math.
// kSkipMath: v3's HQ_EPI_DIAG bit 1 (timing lab only, results WRONG): GELUD without the GELU math.
// The form (piece by reference, the operand through a callable) is the one hipcc compiles to the code the kernels
// had with the block written out in each: tools/isa_diff.py is the check when this changes.
template <int EPI, bool kSkipMath = false, class LoadAux, class StoreP>
__device__ __forceinline__ void hq_epi_piece(uint4& piece, LoadAux&& load_aux, size_t goff, const HqDropArg& dr,
                                              uint32_t key, float (&csum)[8], StoreP&& store_p) {
  if constexpr (EPI == HQ_EPI_GELU) {
    const uint4 pre = piece;   // pre-activation (bf16), kept for backward
    store_p(pre);
    float x[8];
    hq_unpack8(piece, x);
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] = hq_gelu(x[e]);
    piece = hq_pack8(x);
  } else if constexpr (EPI == HQ_EPI_GELUD) {
    float x[8], g[8];
    hq_unpack8(piece, x);
    if constexpr (kSkipMath) {
      for (int e = 0; e < 8; ++e) g[e] = x[e];
    } else {
      hq_gelu_grad8(x, g);   // g = gelu'(x), x = gelu(x)
    }
    store_p(hq_pack8(g));
    piece = hq_pack8(x);
  } else if constexpr (EPI == HQ_EPI_DMUL) {
    float d[8], gd[8];
    hq_unpack8(piece, d);
    hq_unpack8(load_aux(), gd);
#pragma unroll
    for (int e = 0; e < 8; ++e) { d[e] *= gd[e]; csum[e] += d[e]; }
    piece = hq_pack8(d);
  } else if constexpr (EPI == HQ_EPI_DGELU) {
    float d[8], pr[8];
    hq_unpack8(piece, d);
    hq_unpack8(load_aux(), pr);
#pragma unroll
    for (int e = 0; e < 8; ++e) { d[e] *= hq_gelu_grad(pr[e]); csum[e] += d[e]; }
    piece = hq_pack8(d);
  } else if constexpr (EPI == HQ_EPI_RESID) {
    float d[8], rr[8];
    hq_unpack8(piece, d);
    hq_unpack8(load_aux(), rr);
#pragma unroll
    for (int e = 0; e < 8; ++e) d[e] += rr[e];
    piece = hq_pack8(d);
  } else if constexpr (EPI == HQ_EPI_BDR) {
    piece = hq_epi_bdr8(piece, load_aux(), (uint32_t)goff, dr, key);
  }
}

// ---- column partials (DGELU / DMUL; the bias gradient of the producing Linear): a lane's csum[e] is the sum of one
// tile column over its rows, and the 64 / SEGS lanes with equal lane % SEGS hold the same columns: the xor-reduction
// over them.  The block's two wave rows then add through LDS in the kernels, behind the barrier and at the offset
// of each one's LDS plan.
template <int SEGS>
__device__ __forceinline__ void hq_epi_csum_reduce(float (&csum)[8]) {
#pragma unroll
  for (int e = 0; e < 8; ++e)
    for (int o = SEGS; o < 64; o <<= 1) csum[e] += __shfl_xor(csum[e], o, 64);
}
