// Private helpers of the fp32 kernel files of ``--precision fp32`` (f32_embed.hip, f32_norm.hip, f32_rowops.hip,
// f32_attention.hip): the one-wave-per-row layout — 256-thread blocks of kW waves, lane l holds columns c·64 + l
// (coalesced 256-B rows), NC = ceil(H / 64) <= 16 — the dropout multiplier and the column-partial fold.
//
// These files run everything the fp32 encoder does per element or per row instead of ATen ops — fp32 in, fp32 out,
// fp32 statistics, dropout masks from the same counter hash as every other kernel (hq_keep, bit-identical to
// ops/rng.py), so the GPU fp32 model reproduces the CPU oracle (ops/reference.py) op for op; the step's GEMMs run on
// gemm_f32.hip (exact-f32 MFMA).
#pragma once
#include <cstdio>
#include <cstdlib>
#include <type_traits>

#include "hq_common.h"
#include "hq_kernels.h"

constexpr int kW = 4;              // waves per block in the row kernels (one row per wave at a time)
constexpr int kRowsPerBlock = 64;  // column-partial kernels: rows summed per partial (hq_f32_row_partials(T) partials)

static __device__ __forceinline__ float keep_mul(uint32_t idx, uint32_t key, uint32_t thr, float ks) {
  return thr ? (hq_keep(idx, key, thr) ? ks : 0.f) : 1.f;
}

// f(std::integral_constant<int, NC>) for the hidden size's column count per lane
template <typename F>
static void dispatch_nc(int H, F&& f) {
  if (H <= 256) f(std::integral_constant<int, 4>{});
  else if (H <= 512) f(std::integral_constant<int, 8>{});
  else if (H <= 768) f(std::integral_constant<int, 12>{});
  else if (H <= 1024) f(std::integral_constant<int, 16>{});
  else { fprintf(stderr, "f32 row kernels: hidden size %d > 1024 unsupported\n", H); abort(); }
}

// f32_rowops.hip: the deterministic two-level fold of column partials part[nb][width·nout] into outs (nb =
// hq_f32_row_partials(T)).  part must have room for hq_f32_part_rows(T) rows: the level-1 result lives past the nb
// partial rows.
void hq_f32_fold(float* part, int nb, int width, int nout, HqOuts outs, bool accumulate, hipStream_t s);
