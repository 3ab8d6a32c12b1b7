// Small element-wise and column-reduction kernels shared by the whole step (gfx950, wave64), and the process-wide
// state every kernel file's launchers read.
//
//   gelu_fwd / gelu_bwd (+ bias-grad column partials), bias_grad partials (colpart)
//   colsum: the deterministic finish of every [P][N] column-partial buffer (hq_colsum, hq_colsum_outs)
//   zero_f32, key_bias
//   the dropout seed pointer behind hq_drop_key, and hq_num_cus
#include "hq_common.h"
#include "hq_kernels.h"

namespace {

__global__ __launch_bounds__(256) void gelu_fwd_kernel(const uint16_t* __restrict__ pre, uint16_t* __restrict__ out, size_t n8) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += stride) {
    float x[8], o[8];
    hq_unpack8(reinterpret_cast<const uint4*>(pre)[i], x);
#pragma unroll
    for (int k = 0; k < 8; ++k) o[k] = hq_gelu(x[k]);
    reinterpret_cast<uint4*>(out)[i] = hq_pack8(o);
  }
}

// dpre = dout * gelu'(pre); per-block column partials of dpre.  Block: 256 threads × 8 columns =
// 2048-column tile, kRowsBlock rows.  grid = (ceil(N/2048), ceil(T/kRowsBlock)).
constexpr int kRowsBlock = 32;
__global__ __launch_bounds__(256) void gelu_bwd_kernel(const uint16_t* __restrict__ dout, const uint16_t* __restrict__ pre,
                                                       uint16_t* __restrict__ dpre, float* __restrict__ part, int T, int N) {
  const int col = (blockIdx.x * 256 + threadIdx.x) * 8;
  const int r0 = blockIdx.y * kRowsBlock;
  float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (col < N) {
    for (int r = r0; r < min(T, r0 + kRowsBlock); ++r) {
      const size_t off = (size_t)r * N + col;
      float d[8], x[8], o[8];
      hq_unpack8(*reinterpret_cast<const uint4*>(dout + off), d);
      hq_unpack8(*reinterpret_cast<const uint4*>(pre + off), x);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        float cdf, pdf;
        hq_normal_cdf_pdf(x[k], cdf, pdf);
        o[k] = d[k] * (cdf + x[k] * pdf);
        acc[k] += o[k];
      }
      *reinterpret_cast<uint4*>(dpre + off) = hq_pack8(o);
    }
    float* dst = part + (size_t)blockIdx.y * N + col;
    *reinterpret_cast<float4*>(dst) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    *reinterpret_cast<float4*>(dst + 4) = make_float4(acc[4], acc[5], acc[6], acc[7]);
  }
}

__global__ __launch_bounds__(256) void colpart_kernel(const uint16_t* __restrict__ x, float* __restrict__ part, int T, int N) {
  const int col = (blockIdx.x * 256 + threadIdx.x) * 8;
  const int r0 = blockIdx.y * kRowsBlock;
  if (col >= N) return;
  float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int r = r0; r < min(T, r0 + kRowsBlock); ++r) {
    float d[8];
    hq_unpack8(*reinterpret_cast<const uint4*>(x + (size_t)r * N + col), d);
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] += d[k];
  }
  float* dst = part + (size_t)blockIdx.y * N + col;
  *reinterpret_cast<float4*>(dst) = make_float4(acc[0], acc[1], acc[2], acc[3]);
  *reinterpret_cast<float4*>(dst + 4) = make_float4(acc[4], acc[5], acc[6], acc[7]);
}

// out[q*H + c] (+)= Σ_p part[p][q][c]   for the columns named by (Q, H): part is [P][Q*H].
// One 1024-thread block per 64 columns; 16 waves stride over the logical rows p < P, which live at
// physical rows p·Pphys/P (Pphys == P: all rows; otherwise the chunk heads of colsum_chunk_kernel).
// LDS combine.  Deterministic.
__global__ __launch_bounds__(1024) void colsum_kernel(const float* __restrict__ part, int P, int N, HqOuts outs, int Hq,
                                                      int accumulate, int Pphys) {
  __shared__ float red[16][64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int col = blockIdx.x * 64 + lane;
  float s = 0.f;
  if (col < N) {
    if (Pphys == P) {
      int p = wave;
      for (; p + 48 < P; p += 64) {
        s += part[(size_t)p * N + col] + part[(size_t)(p + 16) * N + col] + part[(size_t)(p + 32) * N + col] +
             part[(size_t)(p + 48) * N + col];
      }
      for (; p < P; p += 16) s += part[(size_t)p * N + col];
    } else {
      for (int p = wave; p < P; p += 16) s += part[(size_t)((long)p * Pphys / P) * N + col];
    }
  }
  red[wave][lane] = s;
  __syncthreads();
  if (wave == 0 && col < N) {
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < 16; ++w) t += red[w][lane];
    float* out = outs.p[col / Hq];
    if (out) {
      const int c = col % Hq;
      out[c] = accumulate ? out[c] + t : t;
    }
  }
}

// First pass for tall partial matrices: block (x, c) sums rows [c·P/C, (c+1)·P/C) of its 64 columns
// and writes the sum over the chunk's FIRST row (a row only this block reads), so the pass needs no
// scratch and stays deterministic; colsum_kernel then folds the C chunk heads.  The single-pass
// kernel ran only N/64 blocks (36 for a 2304-column LayerNorm partial of 3072 rows: ~20 µs).
__global__ __launch_bounds__(1024) void colsum_chunk_kernel(float* __restrict__ part, int P, int N, int C) {
  __shared__ float red[16][64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int col = blockIdx.x * 64 + lane;
  const int r0 = (int)((long)blockIdx.y * P / C), r1 = (int)((long)(blockIdx.y + 1) * P / C);
  float s = 0.f;
  if (col < N)
    for (int p = r0 + wave; p < r1; p += 16) s += part[(size_t)p * N + col];
  red[wave][lane] = s;
  __syncthreads();
  if (wave == 0 && col < N) {
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < 16; ++w) t += red[w][lane];
    part[(size_t)r0 * N + col] = t;
  }
}

// The same first pass with 16-B loads: block (x, c) = 4 waves over 256 columns (a float4 per lane) and rows
// [c·P/C, (c+1)·P/C); each wave walks every 4th row with 4 loads in flight, the block folds its 4 waves in LDS in
// wave order.  The 64-column form issued 4-B loads (256 B per wave instruction, one row at a time): 9.7 µs for a
// 28 MB LayerNorm partial (2.9 TB/s).  Needs N % 4 == 0 and 16-B-aligned rows.
__global__ __launch_bounds__(256) void colsum_chunk4_kernel(float* __restrict__ part, int P, int N, int C) {
  __shared__ float4 red[4][64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int c4 = blockIdx.x * 64 + lane;                       // float4 column index
  const int n4 = N >> 2;
  const int r0 = (int)((long)blockIdx.y * P / C), r1 = (int)((long)(blockIdx.y + 1) * P / C);
  const float4* p4 = reinterpret_cast<const float4*>(part);
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
  if (c4 < n4) {
    int p = r0 + wave;
    for (; p + 12 < r1; p += 16) {   // 4 rows in flight, two accumulators (fixed association per wave)
      const float4 v0 = p4[(size_t)p * n4 + c4], v1 = p4[(size_t)(p + 4) * n4 + c4];
      const float4 v2 = p4[(size_t)(p + 8) * n4 + c4], v3 = p4[(size_t)(p + 12) * n4 + c4];
      a.x += v0.x; a.y += v0.y; a.z += v0.z; a.w += v0.w;
      b.x += v1.x; b.y += v1.y; b.z += v1.z; b.w += v1.w;
      a.x += v2.x; a.y += v2.y; a.z += v2.z; a.w += v2.w;
      b.x += v3.x; b.y += v3.y; b.z += v3.z; b.w += v3.w;
    }
    for (; p < r1; p += 4) {
      const float4 v = p4[(size_t)p * n4 + c4];
      a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
    }
  }
  red[wave][lane] = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
  __syncthreads();
  if (wave == 0 && c4 < n4) {
    float4 t = red[0][lane];
#pragma unroll
    for (int w = 1; w < 4; ++w) { const float4 v = red[w][lane]; t.x += v.x; t.y += v.y; t.z += v.z; t.w += v.w; }
    reinterpret_cast<float4*>(part)[(size_t)r0 * n4 + c4] = t;
  }
}

void colsum(const float* part, int P, int N, HqOuts outs, int Hq, bool accumulate, hipStream_t s) {
  const int C = P >= 128 ? std::min(32, P / 32) : P;
  if (C < P) {
    if (N % 4 == 0 && reinterpret_cast<uintptr_t>(part) % 16 == 0)
      hipLaunchKernelGGL(colsum_chunk4_kernel, dim3((N / 4 + 63) / 64, C), dim3(256), 0, s, const_cast<float*>(part), P, N,
                         C);
    else
      hipLaunchKernelGGL(colsum_chunk_kernel, dim3((N + 63) / 64, C), dim3(1024), 0, s, const_cast<float*>(part), P, N, C);
  }
  hipLaunchKernelGGL(colsum_kernel, dim3((N + 63) / 64), dim3(1024), 0, s, part, C, N, outs, Hq, accumulate ? 1 : 0, P);
}

}  // namespace

// Zero-fill of a gradient buffer (the embedding backward's fresh g_word / g_pos): an own grid-stride kernel with
// 16-B stores instead of hipMemsetAsync, so the step's graph holds kernel nodes only (a runtime memset node
// is the one kind of node the rest of the step never uses) and the step trace names every kernel.
// p[0, head) and the last `tail` (< 4 each) are the unaligned ends, [head, head + 4·n4) the 16-B-aligned body
__global__ __launch_bounds__(256) void zero_f32_kernel(float* __restrict__ p, int head, size_t n4, int tail) {
  float4* body = reinterpret_cast<float4*>(p + head);
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) body[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  if (blockIdx.x == 0) {
    if ((int)threadIdx.x < head) p[threadIdx.x] = 0.f;
    if ((int)threadIdx.x < tail) p[head + 4 * n4 + threadIdx.x] = 0.f;
  }
}

// ================================================================================== launchers
namespace {
const uint32_t* g_seed_ptr = nullptr;
}
void hq_set_dropout_seed_ptr(const uint32_t* p) { g_seed_ptr = p; }
void hq_zero_f32(float* p, size_t n, hipStream_t s) {
  if (n == 0) return;
  const size_t mis = (reinterpret_cast<uintptr_t>(p) / sizeof(float)) % 4;   // p is 4-B aligned (f32 tensor)
  const int head = (int)std::min<size_t>(n, mis ? 4 - mis : 0);
  const size_t n4 = (n - head) / 4;
  const int tail = (int)(n - head - 4 * n4);
  const size_t blocks = (n4 + 255) / 256;
  const int grid = (int)(blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks));
  hipLaunchKernelGGL(zero_f32_kernel, dim3(grid), dim3(256), 0, s, p, head, n4, tail);
}
HqDropKey hq_drop_key(uint32_t seed, uint32_t opid) { return HqDropKey{hq_op_key(seed, opid), opid, g_seed_ptr}; }

int hq_num_cus() {
  static int ncu = [] {
    int dev = 0, n = 0;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
    return n > 0 ? n : 256;
  }();
  return ncu;
}

// Additive attention key bias from the collated bool mask (HF: (1 - mask)·-10000): 0 for a real key, -10000 for
// padding.  Replaces a cast / rsub / mul chain of ATen kernels at the start of every forward.
__global__ __launch_bounds__(256) void key_bias_kernel(const uint8_t* __restrict__ mask, float* __restrict__ kb, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) kb[i] = mask[i] ? 0.f : -10000.f;
}

void hq_key_bias(const uint8_t* mask, float* kb, int n, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(key_bias_kernel, dim3((n + 255) / 256), dim3(256), 0, s, mask, kb, n);
}

void hq_gelu_fwd(const uint16_t* pre, uint16_t* out, size_t n, hipStream_t s) {
  const size_t n8 = n / 8;
  const int grid = (int)std::min<size_t>((n8 + 255) / 256, 256 * 16);
  hipLaunchKernelGGL(gelu_fwd_kernel, dim3(grid), dim3(256), 0, s, pre, out, n8);
}

int hq_rowblock_partials(int T) { return (T + kRowsBlock - 1) / kRowsBlock; }

void hq_gelu_bwd(const uint16_t* dout, const uint16_t* pre, uint16_t* dpre, float* part, HqOuts outs, int T, int N,
                 bool accumulate, hipStream_t s) {
  const int nb = hq_rowblock_partials(T);
  hipLaunchKernelGGL(gelu_bwd_kernel, dim3((N + 2047) / 2048, nb), dim3(256), 0, s, dout, pre, dpre, part, T, N);
  if (outs.p[0]) colsum(part, nb, N, outs, N, accumulate, s);
}

void hq_bias_grad(const uint16_t* dy, float* part, HqOuts outs, int T, int N, bool accumulate, hipStream_t s) {
  const int nb = hq_rowblock_partials(T);
  hipLaunchKernelGGL(colpart_kernel, dim3((N + 2047) / 2048, nb), dim3(256), 0, s, dy, part, T, N);
  colsum(part, nb, N, outs, N, accumulate, s);
}

void hq_colsum(const float* part, int P, int N, float* out, bool accumulate, hipStream_t s) {
  colsum(part, P, N, HqOuts{{out, nullptr, nullptr, nullptr}}, N, accumulate, s);
}

void hq_colsum_outs(const float* part, int P, int N, HqOuts outs, int Hq, bool accumulate, hipStream_t s) {
  colsum(part, P, N, outs, Hq, accumulate, s);
}
