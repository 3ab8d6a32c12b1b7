// fp32 flash attention of ``--precision fp32`` (head_dim 64; helpers: hq_f32_rowops.h).
//
//   f32_attn_fwd / _bwd : never holds a [B, nh, L, L] tensor: scores are recomputed per 32-key tile in registers
//                         (online softmax forward, LSE backward).
// Layout: a quad of lanes owns one query (forward / dQ) or one key (dK / dV), lane q & 3 holding head dims
// [16·(q & 3), +16); a dot product over the 64 dims is 16 FMAs per lane + a 2-step DPP quad sum, so every lane of the
// quad ends with the same score (no LDS exchange).
// qkv [T, 3H] (q | k | v, head h at columns h·64 of each third), key_bias [B, L], z = b·nh + h.
#include "hq_f32_rowops.h"

namespace {

constexpr int AD = 64;      // head dim
constexpr int AQ = 64;      // queries (forward / dQ) or keys (dK / dV) per block: 16 quads per wave × 4 waves
constexpr int AT = 32;      // keys (or queries) per LDS tile

__device__ __forceinline__ float quad_sum(float v) {
  v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xB1, 0xF, 0xF, false));   // lane ^ 1
  v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x4E, 0xF, 0xF, false));   // lane ^ 2
  return v;
}

__device__ __forceinline__ void load16(const float* __restrict__ p, float (&v)[16]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float4 t = reinterpret_cast<const float4*>(p)[i];
    v[4 * i] = t.x; v[4 * i + 1] = t.y; v[4 * i + 2] = t.z; v[4 * i + 3] = t.w;
  }
}
__device__ __forceinline__ float dot16(const float (&a)[16], const float* __restrict__ b) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float4 t = reinterpret_cast<const float4*>(b)[i];
    s = fmaf(a[4 * i], t.x, s); s = fmaf(a[4 * i + 1], t.y, s); s = fmaf(a[4 * i + 2], t.z, s); s = fmaf(a[4 * i + 3], t.w, s);
  }
  return s;
}
__device__ __forceinline__ void axpy16(float (&y)[16], float a, const float* __restrict__ x) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float4 t = reinterpret_cast<const float4*>(x)[i];
    y[4 * i] = fmaf(a, t.x, y[4 * i]); y[4 * i + 1] = fmaf(a, t.y, y[4 * i + 1]);
    y[4 * i + 2] = fmaf(a, t.z, y[4 * i + 2]); y[4 * i + 3] = fmaf(a, t.w, y[4 * i + 3]);
  }
}

// stage rows [r0, r0 + AT) (clamped to L) of one head matrix (column offset `col`) into an [AT][AD] LDS tile;
// rows past L are zero
__device__ __forceinline__ void stage_rows(float* __restrict__ dst, const float* __restrict__ src, int ld, int col, int b,
                                           int L, int r0) {
  for (int i = threadIdx.x; i < AT * AD / 4; i += 256) {
    const int r = i / (AD / 4), c4 = i % (AD / 4);
    const int row = r0 + r;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row < L) v = *reinterpret_cast<const float4*>(src + (size_t)(b * L + row) * ld + col + 4 * c4);
    reinterpret_cast<float4*>(dst)[i] = v;
  }
}

__global__ __launch_bounds__(256) void f32_attn_fwd_kernel(const float* __restrict__ qkv, const float* __restrict__ key_bias,
                                                           float* __restrict__ ctx, float* __restrict__ lse, int B, int L,
                                                           int nh, float scale, HqDropKey kd, uint32_t thr, float ks) {
  __shared__ __attribute__((aligned(16))) float Ks[AT * AD], Vs[AT * AD], Bs[AT];
  const int z = blockIdx.y, b = z / nh, h = z - b * nh;
  const int H = nh * AD, H3 = 3 * H;
  const int lane = threadIdx.x & 63, sub = lane & 3;
  const int q = blockIdx.x * AQ + (threadIdx.x >> 2);
  const bool qv = q < L;
  const uint32_t key = kd.get();
  float qr[16], o[16];
  if (qv) load16(qkv + (size_t)(b * L + q) * H3 + h * AD + 16 * sub, qr);
  else
#pragma unroll
    for (int i = 0; i < 16; ++i) qr[i] = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) o[i] = 0.f;
  float m = -INFINITY, l = 0.f;
  const uint32_t rowidx = (uint32_t)(((size_t)z * L + (qv ? q : 0)) * L);
  for (int k0 = 0; k0 < L; k0 += AT) {
    __syncthreads();
    stage_rows(Ks, qkv, H3, H + h * AD, b, L, k0);
    stage_rows(Vs, qkv, H3, 2 * H + h * AD, b, L, k0);
    if (threadIdx.x < AT) Bs[threadIdx.x] = k0 + (int)threadIdx.x < L ? key_bias[b * L + k0 + threadIdx.x] : 0.f;
    __syncthreads();
    const int nk = min(AT, L - k0);
    float s[AT];
    float tmax = -INFINITY;
#pragma unroll
    for (int j = 0; j < AT; ++j) {
      s[j] = j < nk ? quad_sum(dot16(qr, Ks + j * AD + 16 * sub)) * scale + Bs[j] : -INFINITY;
      tmax = fmaxf(tmax, s[j]);
    }
    const float mn = fmaxf(m, tmax);
    const float alpha = m == -INFINITY ? 0.f : expf(m - mn);
    l *= alpha;
#pragma unroll
    for (int i = 0; i < 16; ++i) o[i] *= alpha;
#pragma unroll
    for (int j = 0; j < AT; ++j) {
      if (j < nk) {
        const float p = expf(s[j] - mn);
        l += p;
        axpy16(o, p * keep_mul(rowidx + (uint32_t)(k0 + j), key, thr, ks), Vs + j * AD + 16 * sub);
      }
    }
    m = mn;
  }
  if (!qv) return;
  const float inv = 1.f / l;
  float* out = ctx + (size_t)(b * L + q) * H + h * AD + 16 * sub;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    reinterpret_cast<float4*>(out)[i] = make_float4(o[4 * i] * inv, o[4 * i + 1] * inv, o[4 * i + 2] * inv, o[4 * i + 3] * inv);
  if (sub == 0) lse[(size_t)z * L + q] = m + logf(l);
}

// dQ (and δ = rowsum(dO ∘ O) for the dK / dV kernel): a quad per query, keys streamed through LDS tiles.
// dS = P·(dP·keep − δ), dQ = scale·Σ_k dS·K_k (ops/reference.py attn_bwd).
__global__ __launch_bounds__(256) void f32_attn_dq_kernel(const float* __restrict__ dctx, const float* __restrict__ qkv,
                                                          const float* __restrict__ ctx, const float* __restrict__ lse,
                                                          const float* __restrict__ key_bias, float* __restrict__ dqkv,
                                                          float* __restrict__ delta, int B, int L, int nh, float scale,
                                                          HqDropKey kd, uint32_t thr, float ks) {
  __shared__ __attribute__((aligned(16))) float Ks[AT * AD], Vs[AT * AD], Bs[AT];
  const int z = blockIdx.y, b = z / nh, h = z - b * nh;
  const int H = nh * AD, H3 = 3 * H;
  const int lane = threadIdx.x & 63, sub = lane & 3;
  const int q = blockIdx.x * AQ + (threadIdx.x >> 2);
  const bool qv = q < L;
  const uint32_t key = kd.get();
  float qr[16], dor[16], dq[16];
  float dl = 0.f, ls = 0.f;
  if (qv) {
    load16(qkv + (size_t)(b * L + q) * H3 + h * AD + 16 * sub, qr);
    load16(dctx + (size_t)(b * L + q) * H + h * AD + 16 * sub, dor);
    float orr[16];
    load16(ctx + (size_t)(b * L + q) * H + h * AD + 16 * sub, orr);
    float d = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) d = fmaf(dor[i], orr[i], d);
    dl = quad_sum(d);
    ls = lse[(size_t)z * L + q];
    if (sub == 0) delta[(size_t)z * L + q] = dl;
  } else {
#pragma unroll
    for (int i = 0; i < 16; ++i) qr[i] = dor[i] = 0.f;
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) dq[i] = 0.f;
  const uint32_t rowidx = (uint32_t)(((size_t)z * L + (qv ? q : 0)) * L);
  for (int k0 = 0; k0 < L; k0 += AT) {
    __syncthreads();
    stage_rows(Ks, qkv, H3, H + h * AD, b, L, k0);
    stage_rows(Vs, qkv, H3, 2 * H + h * AD, b, L, k0);
    if (threadIdx.x < AT) Bs[threadIdx.x] = k0 + (int)threadIdx.x < L ? key_bias[b * L + k0 + threadIdx.x] : 0.f;
    __syncthreads();
    const int nk = min(AT, L - k0);
    for (int j = 0; j < nk; ++j) {
      const float s = quad_sum(dot16(qr, Ks + j * AD + 16 * sub)) * scale + Bs[j];
      const float p = expf(s - ls);
      const float dp = quad_sum(dot16(dor, Vs + j * AD + 16 * sub)) * keep_mul(rowidx + (uint32_t)(k0 + j), key, thr, ks);
      axpy16(dq, p * (dp - dl), Ks + j * AD + 16 * sub);
    }
  }
  if (!qv) return;
  float* out = dqkv + (size_t)(b * L + q) * H3 + h * AD + 16 * sub;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    reinterpret_cast<float4*>(out)[i] = make_float4(dq[4 * i] * scale, dq[4 * i + 1] * scale, dq[4 * i + 2] * scale,
                                                    dq[4 * i + 3] * scale);
}

// dK, dV: a quad per key, queries streamed through LDS tiles (Q, dO, LSE, δ).
__global__ __launch_bounds__(256) void f32_attn_dkdv_kernel(const float* __restrict__ dctx, const float* __restrict__ qkv,
                                                            const float* __restrict__ lse, const float* __restrict__ delta,
                                                            const float* __restrict__ key_bias, float* __restrict__ dqkv,
                                                            int B, int L, int nh, float scale, HqDropKey kd, uint32_t thr,
                                                            float ks) {
  __shared__ __attribute__((aligned(16))) float Qs[AT * AD], Os[AT * AD], Ls[AT], Ds[AT];
  const int z = blockIdx.y, b = z / nh, h = z - b * nh;
  const int H = nh * AD, H3 = 3 * H;
  const int lane = threadIdx.x & 63, sub = lane & 3;
  const int k = blockIdx.x * AQ + (threadIdx.x >> 2);
  const bool kv = k < L;
  const uint32_t key = kd.get();
  float kr[16], vr[16], dk[16], dv[16];
  float kb = 0.f;
  if (kv) {
    load16(qkv + (size_t)(b * L + k) * H3 + H + h * AD + 16 * sub, kr);
    load16(qkv + (size_t)(b * L + k) * H3 + 2 * H + h * AD + 16 * sub, vr);
    kb = key_bias[b * L + k];
  } else {
#pragma unroll
    for (int i = 0; i < 16; ++i) kr[i] = vr[i] = 0.f;
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) dk[i] = dv[i] = 0.f;
  for (int q0 = 0; q0 < L; q0 += AT) {
    __syncthreads();
    stage_rows(Qs, qkv, H3, h * AD, b, L, q0);
    stage_rows(Os, dctx, H, h * AD, b, L, q0);
    if (threadIdx.x < AT) {
      const bool ok = q0 + (int)threadIdx.x < L;
      Ls[threadIdx.x] = ok ? lse[(size_t)z * L + q0 + threadIdx.x] : 0.f;
      Ds[threadIdx.x] = ok ? delta[(size_t)z * L + q0 + threadIdx.x] : 0.f;
    }
    __syncthreads();
    const int nq = min(AT, L - q0);
    for (int j = 0; j < nq; ++j) {
      const float s = quad_sum(dot16(kr, Qs + j * AD + 16 * sub)) * scale + kb;
      const float p = expf(s - Ls[j]);
      const float km = keep_mul((uint32_t)(((size_t)z * L + q0 + j) * L + (kv ? k : 0)), key, thr, ks);
      axpy16(dv, p * km, Os + j * AD + 16 * sub);
      const float dp = quad_sum(dot16(vr, Os + j * AD + 16 * sub)) * km;
      axpy16(dk, p * (dp - Ds[j]), Qs + j * AD + 16 * sub);
    }
  }
  if (!kv) return;
  float* ok = dqkv + (size_t)(b * L + k) * H3 + H + h * AD + 16 * sub;
  float* ov = ok + H;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    reinterpret_cast<float4*>(ok)[i] = make_float4(dk[4 * i] * scale, dk[4 * i + 1] * scale, dk[4 * i + 2] * scale,
                                                   dk[4 * i + 3] * scale);
    reinterpret_cast<float4*>(ov)[i] = make_float4(dv[4 * i], dv[4 * i + 1], dv[4 * i + 2], dv[4 * i + 3]);
  }
}

}  // namespace

void hq_f32_attn_fwd(const float* qkv, const float* key_bias, float* ctx, float* lse, int B, int L, int nh, float p,
                     uint32_t seed, uint32_t opid, float scale, hipStream_t s) {
  const uint32_t thr = p > 0.f ? hq_threshold(p) : 0u;
  const HqDropKey kd = hq_drop_key(seed, opid);
  hipLaunchKernelGGL(f32_attn_fwd_kernel, dim3((L + AQ - 1) / AQ, B * nh), dim3(256), 0, s, qkv, key_bias, ctx, lse, B, L, nh,
                     scale, kd, thr, hq_keep_scale(thr));
}

void hq_f32_attn_bwd(const float* dctx, const float* qkv, const float* ctx, const float* lse, const float* key_bias,
                     float* dqkv, float* delta, int B, int L, int nh, float p, uint32_t seed, uint32_t opid, float scale,
                     hipStream_t s) {
  const uint32_t thr = p > 0.f ? hq_threshold(p) : 0u;
  const HqDropKey kd = hq_drop_key(seed, opid);
  const float kss = hq_keep_scale(thr);
  const dim3 grid((L + AQ - 1) / AQ, B * nh);
  hipLaunchKernelGGL(f32_attn_dq_kernel, grid, dim3(256), 0, s, dctx, qkv, ctx, lse, key_bias, dqkv, delta, B, L, nh, scale,
                     kd, thr, kss);
  hipLaunchKernelGGL(f32_attn_dkdv_kernel, grid, dim3(256), 0, s, dctx, qkv, lse, delta, key_bias, dqkv, B, L, nh, scale, kd,
                     thr, kss);
}
