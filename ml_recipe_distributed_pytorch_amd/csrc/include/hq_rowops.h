// Private helpers of the row-wise bf16 kernel files (norm.hip, embed.hip, heads.hip): the one-wave-per-row layout —
// 256-thread blocks of kWaves waves, lane owns 4 consecutive columns per 256-column chunk, NCH = ceil(H/256) chunks.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <type_traits>

#include <hip/hip_runtime.h>

constexpr int kRowsPerWave = 8;   // rows a wave walks in the backward kernels
constexpr int kWaves = 4;         // 256-thread blocks

// Reduce NQ per-lane column accumulators over the 4 waves of the block into part[block][q][H].
template <int NCH, int NQ>
static __device__ __forceinline__ void block_partials(float (&acc)[NQ][NCH][4], float* lds, float* part, int H) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int col = c * 256 + lane * 4;
      if (col < H) *reinterpret_cast<float4*>(lds + wave * H + col) = make_float4(acc[q][c][0], acc[q][c][1], acc[q][c][2], acc[q][c][3]);
    }
    __syncthreads();
    for (int col = threadIdx.x; col < H; col += 256) {
      float s = lds[col] + lds[H + col] + lds[2 * H + col] + lds[3 * H + col];
      part[(((size_t)blockIdx.y * gridDim.x + blockIdx.x) * NQ + q) * H + col] = s;  // linear block id (2-D grids)
    }
    __syncthreads();
  }
}

// f(std::integral_constant<int, NCH>) for the hidden size's chunk count
template <typename F>
static void dispatch_nch(int H, F&& f) {
  const int nch = (H + 255) / 256;
  switch (nch) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 5: f(std::integral_constant<int, 5>{}); break;
    case 6: f(std::integral_constant<int, 6>{}); break;
    case 8: f(std::integral_constant<int, 8>{}); break;
    default: fprintf(stderr, "hq: unsupported hidden size %d\n", H); abort();
  }
}
