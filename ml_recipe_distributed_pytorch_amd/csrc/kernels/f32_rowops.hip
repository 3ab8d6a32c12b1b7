// fp32 element-wise and column-sum ops of ``--precision fp32`` (helpers: hq_f32_rowops.h).
//
//   f32_gelu_fwd / _bwd : erf GELU; backward with the producing Linear's bias-gradient column partials
//   f32_colsum          : column partials of a [T, N] matrix (the Linear bias gradients), then a fixed-order fold
//   hq_f32_fold         : the fold every fp32 column-partial kernel ends with (also f32_embed.hip, f32_norm.hip)
#include "hq_f32_rowops.h"

namespace {

constexpr float kInvSqrt2 = 0.70710678118654752f;
constexpr float kInvSqrt2Pi = 0.39894228040143268f;

__global__ __launch_bounds__(256) void f32_gelu_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, size_t n) {
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    const float v = x[i];
    y[i] = 0.5f * v * (1.f + erff(v * kInvSqrt2));
  }
}

// d = dout·gelu'(x); column partials of d per kRowsPerBlock rows (thread = column: coalesced rows)
__global__ __launch_bounds__(256) void f32_gelu_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ x,
                                                           float* __restrict__ d, float* __restrict__ part, int T, int N) {
  const int col = blockIdx.x * 256 + threadIdx.x;
  if (col >= N) return;
  const int r0 = blockIdx.y * kRowsPerBlock, r1 = min(T, r0 + kRowsPerBlock);
  float s = 0.f;
  for (int r = r0; r < r1; ++r) {
    const size_t o = (size_t)r * N + col;
    const float v = x[o];
    const float g = dout[o] * (0.5f * (1.f + erff(v * kInvSqrt2)) + v * expf(-0.5f * v * v) * kInvSqrt2Pi);
    d[o] = g;
    s += g;
  }
  if (part) part[(size_t)blockIdx.y * N + col] = s;
}

// column partials of x [T, N] per kRowsPerBlock rows
__global__ __launch_bounds__(256) void f32_colpart_kernel(const float* __restrict__ x, float* __restrict__ part, int T, int N) {
  const int col = blockIdx.x * 256 + threadIdx.x;
  if (col >= N) return;
  const int r0 = blockIdx.y * kRowsPerBlock, r1 = min(T, r0 + kRowsPerBlock);
  float s = 0.f;
  for (int r = r0; r < r1; ++r) s += x[(size_t)r * N + col];
  part[(size_t)blockIdx.y * N + col] = s;
}

// Deterministic two-level fold of column partials part[nb][W] (nb ~ T / 64 rows, W up to 3·H): a single
// column-per-thread pass had W / 256 blocks (9 at W = 2304) each walking ~400 rows serially — 97 µs per fold.
// Level 1: blocks of (64 columns × one of kFoldS row slices), 4 waves each summing every 4th row of the slice,
// combined in LDS in a fixed order -> p2[kFoldS][W]; level 2: out[c] (+)= Σ_s p2[s][c] in slice order.
constexpr int kFoldS = 16;
__global__ __launch_bounds__(256) void f32_fold1_kernel(const float* __restrict__ part, int nb, int W,
                                                        float* __restrict__ p2) {
  __shared__ float red[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lane, sl = blockIdx.y;
  const int b0 = nb * sl / kFoldS, b1 = nb * (sl + 1) / kFoldS;
  float s = 0.f;
  if (c < W)
    for (int b = b0 + wave; b < b1; b += 4) s += part[(size_t)b * W + c];
  red[wave][lane] = s;
  __syncthreads();
  if (wave == 0 && c < W) p2[(size_t)sl * W + c] = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
}
__global__ __launch_bounds__(256) void f32_fold2_kernel(const float* __restrict__ p2, int W, int width, HqOuts outs,
                                                        int accumulate) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= W) return;
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < kFoldS; ++k) s += p2[(size_t)k * W + i];
  float* dst = outs.p[i / width];
  if (dst == nullptr) return;
  const int c = i % width;
  dst[c] = accumulate ? dst[c] + s : s;
}

}  // namespace

int hq_f32_row_partials(int T) { return (T + kRowsPerBlock - 1) / kRowsPerBlock; }
int hq_f32_part_rows(int T) { return hq_f32_row_partials(T) + kFoldS; }

// part must have room for kFoldS more rows past its nb partial rows (the level-1 result lives there)
void hq_f32_fold(float* part, int nb, int width, int nout, HqOuts outs, bool accumulate, hipStream_t s) {
  const int W = width * nout;
  float* p2 = part + (size_t)nb * W;
  hipLaunchKernelGGL(f32_fold1_kernel, dim3((W + 63) / 64, kFoldS), dim3(256), 0, s, part, nb, W, p2);
  hipLaunchKernelGGL(f32_fold2_kernel, dim3((W + 255) / 256), dim3(256), 0, s, p2, W, width, outs, accumulate ? 1 : 0);
}

void hq_f32_gelu_fwd(const float* x, float* y, size_t n, hipStream_t s) {
  const int grid = (int)std::max<size_t>(1, std::min<size_t>((n + 255) / 256, 8192));
  hipLaunchKernelGGL(f32_gelu_fwd_kernel, dim3(grid), dim3(256), 0, s, x, y, n);
}

void hq_f32_gelu_bwd(const float* dout, const float* x, float* d, float* part, float* g_bias, int T, int N, bool accumulate,
                     hipStream_t s) {
  const int nb = hq_f32_row_partials(T);
  hipLaunchKernelGGL(f32_gelu_bwd_kernel, dim3((N + 255) / 256, nb), dim3(256), 0, s, dout, x, d, g_bias ? part : nullptr, T,
                     N);
  if (g_bias) hq_f32_fold(part, nb, N, 1, HqOuts{{g_bias, nullptr, nullptr, nullptr}}, accumulate, s);
}

void hq_f32_colsum(const float* x, float* part, float* out, int T, int N, bool accumulate, hipStream_t s) {
  const int nb = hq_f32_row_partials(T);
  hipLaunchKernelGGL(f32_colpart_kernel, dim3((N + 255) / 256, nb), dim3(256), 0, s, x, part, T, N);
  hq_f32_fold(part, nb, N, 1, HqOuts{{out, nullptr, nullptr, nullptr}}, accumulate, s);
}
