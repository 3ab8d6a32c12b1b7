// fp32 residual + dropout + LayerNorm of ``--precision fp32`` (the row layout of hq_f32_rowops.h).
//
//   f32_ln_fwd / _bwd : z = dropout(a) + resid, y = LN(z); backward dz, da and γ / β / bias column partials
#include "hq_f32_rowops.h"

namespace {

template <int NC>
__global__ __launch_bounds__(256) void f32_ln_fwd_kernel(const float* __restrict__ a, const float* __restrict__ resid,
                                                         const float* __restrict__ gamma, const float* __restrict__ beta,
                                                         float* __restrict__ y, float* __restrict__ z, float* __restrict__ mean,
                                                         float* __restrict__ rstd, int T, int H, float eps, HqDropKey kd,
                                                         uint32_t thr, float ks) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * kW + (threadIdx.x >> 6);
  if (row >= T) return;
  const uint32_t key = kd.get();
  float x[NC];
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int col = c * 64 + lane;
    const size_t o = (size_t)row * H + col;
    x[c] = col < H ? a[o] * keep_mul((uint32_t)o, key, thr, ks) + resid[o] : 0.f;
    s += x[c];
  }
  const float mu = hq_wave_sum(s) / H;
  float v = 0.f;
#pragma unroll
  for (int c = 0; c < NC; ++c)
    if (c * 64 + lane < H) v += (x[c] - mu) * (x[c] - mu);
  const float rs = rsqrtf(hq_wave_sum(v) / H + eps);
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int col = c * 64 + lane;
    if (col < H) {
      const size_t o = (size_t)row * H + col;
      z[o] = x[c];
      y[o] = (x[c] - mu) * rs * gamma[col] + beta[col];
    }
  }
  if (lane == 0) { mean[row] = mu; rstd[row] = rs; }
}

// dz = LN backward of g = dy (+ dy2), da = dz·keep; partials [block][3H] = Σ g·x̂ | Σ g | Σ da.  beta != null: `z` is
// the forward output y and x̂ = (y − β)/γ (0 where γ = 0), ops/reference.py ln_bwd's FROMY form.
template <int NC>
__global__ __launch_bounds__(256) void f32_ln_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ dy2,
                                                         const float* __restrict__ z, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, const float* __restrict__ mean,
                                                         const float* __restrict__ rstd, float* __restrict__ dz,
                                                         float* __restrict__ da, float* __restrict__ part, int T, int H,
                                                         HqDropKey kd, uint32_t thr, float ks) {
  __shared__ float red[kW][3][NC * 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t key = kd.get();
  float acc[3][NC], gam[NC], ig[NC], bb[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    acc[0][c] = acc[1][c] = acc[2][c] = 0.f;
    const int col = c * 64 + lane;
    gam[c] = col < H ? gamma[col] : 0.f;
    ig[c] = gam[c] != 0.f ? 1.f / gam[c] : 0.f;
    bb[c] = (beta != nullptr && col < H) ? beta[col] : 0.f;
  }
  const int r0 = blockIdx.x * kRowsPerBlock, r1 = min(T, r0 + kRowsPerBlock);
  for (int row = r0 + wave; row < r1; row += kW) {
    const float mu = mean[row], rs = rstd[row];
    float xh[NC], g[NC], s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int col = c * 64 + lane;
      const size_t o = (size_t)row * H + col;
      if (col < H) {
        g[c] = dy[o] + (dy2 ? dy2[o] : 0.f);
        xh[c] = beta != nullptr ? z[o] * ig[c] - bb[c] * ig[c] : (z[o] - mu) * rs;
      } else {
        g[c] = xh[c] = 0.f;
      }
      acc[0][c] += g[c] * xh[c];
      acc[1][c] += g[c];
      const float d = g[c] * gam[c];
      s1 += d;
      s2 += d * xh[c];
    }
    s1 = hq_wave_sum(s1) / H;
    s2 = hq_wave_sum(s2) / H;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int col = c * 64 + lane;
      if (col < H) {
        const size_t o = (size_t)row * H + col;
        const float d = rs * (g[c] * gam[c] - s1 - xh[c] * s2);
        const float dd = d * keep_mul((uint32_t)o, key, thr, ks);
        dz[o] = d;
        da[o] = dd;
        acc[2][c] += dd;
      }
    }
  }
#pragma unroll
  for (int c = 0; c < NC; ++c)
#pragma unroll
    for (int k = 0; k < 3; ++k) red[wave][k][c * 64 + lane] = acc[k][c];
  __syncthreads();
  for (int i = threadIdx.x; i < 3 * H; i += 256) {
    const int k = i / H, col = i - k * H;
    part[(size_t)blockIdx.x * 3 * H + i] = (red[0][k][col] + red[1][k][col]) + (red[2][k][col] + red[3][k][col]);
  }
}

}  // namespace

void hq_f32_ln_fwd(const float* a, const float* resid, const float* gamma, const float* beta, float* y, float* z, float* mean,
                   float* rstd, int T, int H, float eps, float p, uint32_t seed, uint32_t opid, hipStream_t s) {
  const uint32_t thr = p > 0.f ? hq_threshold(p) : 0u;
  const HqDropKey kd = hq_drop_key(seed, opid);
  dispatch_nc(H, [&](auto nc) {
    hipLaunchKernelGGL(f32_ln_fwd_kernel<decltype(nc)::value>, dim3((T + kW - 1) / kW), dim3(256), 0, s, a, resid, gamma,
                       beta, y, z, mean, rstd, T, H, eps, kd, thr, hq_keep_scale(thr));
  });
}

void hq_f32_ln_bwd(const float* dy, const float* dy2, const float* z, const float* gamma, const float* beta, const float* mean,
                   const float* rstd, float* dz, float* da, float* part, HqOuts outs, int T, int H, float p, uint32_t seed,
                   uint32_t opid, bool accumulate, hipStream_t s) {
  const uint32_t thr = p > 0.f ? hq_threshold(p) : 0u;
  const HqDropKey kd = hq_drop_key(seed, opid);
  const int nb = hq_f32_row_partials(T);
  dispatch_nc(H, [&](auto nc) {
    hipLaunchKernelGGL(f32_ln_bwd_kernel<decltype(nc)::value>, dim3(nb), dim3(256), 0, s, dy, dy2, z, gamma, beta, mean, rstd,
                       dz, da, part, T, H, kd, thr, hq_keep_scale(thr));
  });
  hq_f32_fold(part, nb, H, 3, outs, accumulate, s);
}
