// fp32 embedding layer of ``--precision fp32`` (the row layout of hq_f32_rowops.h).
//
//   f32_embed_fwd / _bwd : 3 gathers + LayerNorm + dropout; backward into the tables with f32 atomics (default) or,
//                          deterministic, by key-sorted runs summed in a fixed order (f32_embed_run_kernel /
//                          f32_embed_carry_kernel)
#include "hq_f32_rowops.h"

namespace {

// one wave per row; lane l holds columns c·64 + l (coalesced 256-B rows); NC = ceil(H / 64) <= 16
template <int NC>
__global__ __launch_bounds__(256) void f32_embed_fwd_kernel(const int64_t* __restrict__ ids, const int64_t* __restrict__ pids,
                                                            const int64_t* __restrict__ tids, const float* __restrict__ ww,
                                                            const float* __restrict__ wp, const float* __restrict__ wt,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta,
                                                            float* __restrict__ y, float* __restrict__ mean,
                                                            float* __restrict__ rstd, int T, int H, float eps, int V, int P,
                                                            int NTY, HqDropKey kd, uint32_t thr, float ks) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * kW + (threadIdx.x >> 6);
  if (row >= T) return;
  const uint32_t key = kd.get();
  const int64_t id = ids[row], pid = pids[row], tid = tids[row];
  HQ_DASSERT(id >= 0 && id < V && pid >= 0 && pid < P && tid >= 0 && tid < NTY);
  float x[NC];
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int col = c * 64 + lane;
    x[c] = col < H ? ww[id * H + col] + wp[pid * H + col] + wt[tid * H + col] : 0.f;
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
      const float o = (x[c] - mu) * rs * gamma[col] + beta[col];
      y[(size_t)row * H + col] = o * keep_mul((uint32_t)((size_t)row * H + col), key, thr, ks);
    }
  }
  if (lane == 0) { mean[row] = mu; rstd[row] = rs; }
}

// The LayerNorm backward of one row from the recomputed x̂, per column; f32_embed_bwd_kernel and the sorted-run
// kernel (f32_embed_run_kernel) both build a row's dx from these two.
// column col < H of row `row`: x̂ and g = the dropout-masked dy
__device__ __forceinline__ void f32_emb_xg(const float* __restrict__ dy, const float* __restrict__ ww,
                                           const float* __restrict__ wp, const float* __restrict__ wt, size_t row, int64_t id,
                                           int64_t pid, int64_t tid, float mu, float rs, uint32_t key, uint32_t thr, float ks,
                                           int H, int col, float& xh, float& g) {
  const float x = ww[id * H + col] + wp[pid * H + col] + wt[tid * H + col];
  xh = (x - mu) * rs;
  g = dy[row * H + col] * keep_mul((uint32_t)(row * H + col), key, thr, ks);
}
// dx = ∂/∂(word+pos+type) from the row's s1 = Σ g·γ / H and s2 = Σ g·γ·x̂ / H.  CONTRACT is whether the expression may
// contract into FMAs: f32_embed_bwd_kernel always compiled it under the default contraction and the sorted-run kernel
// with contraction off, so the two kernels' dx are NOT the same bit for bit.  Each keeps its form (both are results
// the project has published); a table row of the sorted-run path is the documented sum of the run kernel's dx.
template <bool CONTRACT>
__device__ __forceinline__ float f32_emb_dx(float rs, float g, float gam, float s1, float xh, float s2) {
  if constexpr (CONTRACT) {
    return rs * (g * gam - s1 - xh * s2);
  } else {
#pragma clang fp contract(off)
    return rs * (g * gam - s1 - xh * s2);
  }
}

// rows [blockIdx.x·kRowsPerBlock, +kRowsPerBlock), one wave per row at a time; γ / β partials per block.
// DET: no table scatter here — the word / position / type (NTY > 2) rows come from f32_embed_run_kernel.
template <int NC, bool DET>
__global__ __launch_bounds__(256) void f32_embed_bwd_kernel(const float* __restrict__ dy, const int64_t* __restrict__ ids,
                                                            const int64_t* __restrict__ pids, const int64_t* __restrict__ tids,
                                                            const float* __restrict__ ww, const float* __restrict__ wp,
                                                            const float* __restrict__ wt, const float* __restrict__ gamma,
                                                            const float* __restrict__ mean, const float* __restrict__ rstd,
                                                            float* __restrict__ g_word, float* __restrict__ g_pos,
                                                            float* __restrict__ g_type, float* __restrict__ part, int T, int H,
                                                            int pad_word, int pad_pos, int V, int P, int NTY, HqDropKey kd,
                                                            uint32_t thr, float ks) {
  // γ | β | type-0 | type-1 partials per block (the type rows as partials when NTY <= 2: every row of the batch
  // hits one of two rows, which f32 atomics serialise)
  __shared__ float red[kW][4][NC * 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t key = kd.get();
  const bool tpart = NTY <= 2;
  float ag[NC], ab[NC], at0[NC], at1[NC], gam[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    ag[c] = ab[c] = at0[c] = at1[c] = 0.f;
    gam[c] = c * 64 + lane < H ? gamma[c * 64 + lane] : 0.f;
  }
  const int r0 = blockIdx.x * kRowsPerBlock, r1 = min(T, r0 + kRowsPerBlock);
  for (int row = r0 + wave; row < r1; row += kW) {
    const int64_t id = ids[row], pid = pids[row], tid = tids[row];
    HQ_DASSERT(id >= 0 && id < V && pid >= 0 && pid < P && tid >= 0 && tid < NTY);
    const float mu = mean[row], rs = rstd[row];
    float xh[NC], g[NC], s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int col = c * 64 + lane;
      if (col < H) f32_emb_xg(dy, ww, wp, wt, (size_t)row, id, pid, tid, mu, rs, key, thr, ks, H, col, xh[c], g[c]);
      else xh[c] = g[c] = 0.f;
      ag[c] += g[c] * xh[c];
      ab[c] += g[c];
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
        const float dx = f32_emb_dx<true>(rs, g[c], gam[c], s1, xh[c], s2);
        if (!DET) {
          if (id != pad_word) atomicAdd(g_word + id * H + col, dx);
          if (pid != pad_pos) atomicAdd(g_pos + pid * H + col, dx);
          if (!tpart) atomicAdd(g_type + tid * H + col, dx);
        }
        at0[c] += tid == 0 ? dx : 0.f;
        at1[c] += tid == 1 ? dx : 0.f;
      }
    }
  }
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    red[wave][0][c * 64 + lane] = ag[c];
    red[wave][1][c * 64 + lane] = ab[c];
    red[wave][2][c * 64 + lane] = at0[c];
    red[wave][3][c * 64 + lane] = at1[c];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 4 * H; i += 256) {
    const int w = i / H, col = i - w * H;
    part[(size_t)blockIdx.x * 4 * H + i] = (red[0][w][col] + red[1][w][col]) + (red[2][w][col] + red[3][w][col]);
  }
}

// ---- deterministic table gradients: sorted runs instead of atomics (hq_f32_embed_bwd with deterministic = true)
// The fp32 pair of the sorted-run kernels: chunks, pieces, carries and the summation order of a table row are
// stated once, above embed_word_kernel in embed.hip.  Specific to this pair: the lane owns the columns q·64 + lane
// (any H, no H % 4 requirement), and a row's dx is f32_embed_bwd_kernel's expression (f32_emb_dx) with contraction
// off (see there: not bit for bit that kernel's dx).
template <int NC, int KEY>
__global__ __launch_bounds__(256) void f32_embed_run_kernel(
    const int32_t* __restrict__ skeys, const int32_t* __restrict__ srows, const float* __restrict__ dy,
    const int64_t* __restrict__ ids, const int64_t* __restrict__ pids, const int64_t* __restrict__ tids,
    const float* __restrict__ ww, const float* __restrict__ wp, const float* __restrict__ wt,
    const float* __restrict__ gamma, const float* __restrict__ mean, const float* __restrict__ rstd,
    float* __restrict__ g_dst, float* __restrict__ carry, int T, int H, int pad_key, int accumulate, int NK, int V,
    int P, int NTY, HqDropKey kd, uint32_t thr, float ks) {
  static_assert(kHqEmbRunChunk <= 64, "one row's metadata per lane");
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = blockIdx.x * kW + wave;
  const int j0 = c * kHqEmbRunChunk;
  if (j0 >= T) return;
  const int j1 = min(T, j0 + kHqEmbRunChunk);
  const uint32_t key = kd.get();
  float gam[NC], acc[NC];
#pragma unroll
  for (int q = 0; q < NC; ++q) {
    acc[q] = 0.f;
    gam[q] = q * 64 + lane < H ? gamma[q * 64 + lane] : 0.f;
  }
  const int first = __builtin_amdgcn_readfirstlane(skeys[j0]);
  const bool head_cont = c > 0 && __builtin_amdgcn_readfirstlane(skeys[j0 - 1]) == first;
  const int after = j1 < T ? __builtin_amdgcn_readfirstlane(skeys[j1]) : -1;
  auto flush = [&](int k, int kind) {   // kind 0: carry slot 0, 1: carry slot 1, 2: the gradient row
    if (k != pad_key) {
      HQ_DASSERT(kind == 2 ? (k >= 0 && k < NK) : (kind >= 0 && kind < 2 && c >= 0 && c * kHqEmbRunChunk < T));
      float* dst = kind == 2 ? g_dst + (size_t)k * H : carry + ((size_t)c * 2 + kind) * H;
#pragma unroll
      for (int q = 0; q < NC; ++q) {
        const int col = q * 64 + lane;
        if (col < H) dst[col] = (kind == 2 && accumulate) ? acc[q] + dst[col] : acc[q];
      }
    }
#pragma unroll
    for (int q = 0; q < NC; ++q) acc[q] = 0.f;
  };
  // the chunk's sorted rows and their metadata, one per lane
  const bool ok = lane < j1 - j0;
  const int myrow = ok ? srows[j0 + lane] : 0;
  HQ_DASSERT(myrow >= 0 && myrow < T);
  const int mid = ok ? (int)ids[myrow] : 0, mpid = ok ? (int)pids[myrow] : 0, mtid = ok ? (int)tids[myrow] : 0;
  const float mmu = ok ? mean[myrow] : 0.f, mrs = ok ? rstd[myrow] : 0.f;
  int seg = first;
  bool seg_first = true;
#pragma unroll 1
  for (int j = j0; j < j1; ++j) {
    const int r = j - j0;
    const size_t row = (size_t)__builtin_amdgcn_readlane(myrow, r);
    const int id = __builtin_amdgcn_readlane(mid, r), pid = __builtin_amdgcn_readlane(mpid, r),
              tid = __builtin_amdgcn_readlane(mtid, r);
    const float mu = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mmu), r));
    const float rs = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mrs), r));
    HQ_DASSERT(id >= 0 && id < V && pid >= 0 && pid < P && tid >= 0 && tid < NTY && row < (size_t)T);
    const int k = KEY == 0 ? id : (KEY == 1 ? pid : tid);
    HQ_DASSERT(k == skeys[j] && k >= 0 && k < NK);
    if (k != seg) {
      flush(seg, seg_first && head_cont ? 0 : 2);
      seg = k;
      seg_first = false;
    }
    float xh[NC], g[NC], s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int q = 0; q < NC; ++q) {
      const int col = q * 64 + lane;
      if (col < H) f32_emb_xg(dy, ww, wp, wt, row, id, pid, tid, mu, rs, key, thr, ks, H, col, xh[q], g[q]);
      else xh[q] = g[q] = 0.f;
      const float d = g[q] * gam[q];
      s1 += d;
      s2 += d * xh[q];
    }
    s1 = hq_wave_sum(s1) / H;
    s2 = hq_wave_sum(s2) / H;
#pragma unroll
    for (int q = 0; q < NC; ++q) {
      // dx is rounded on its own and then added: a multiply fused into the running sum would make the piece
      // something other than the sum of its rows' dx
#pragma clang fp contract(off)
      const float dx = f32_emb_dx<false>(rs, g[q], gam[q], s1, xh[q], s2);
      if (q * 64 + lane < H) acc[q] += dx;
    }
  }
  const bool from_prev = seg_first && head_cont;
  flush(seg, from_prev ? 0 : (after == seg ? 1 : 2));
}

// Runs that cross chunk boundaries: the chunk holding a run's first piece (carry slot 1) adds the following chunks'
// slot-0 pieces in chunk order, then the existing row (accumulate), and stores the gradient row.
template <int NC>
__global__ __launch_bounds__(256) void f32_embed_carry_kernel(const int32_t* __restrict__ skeys,
                                                              const float* __restrict__ carry, float* __restrict__ g_dst,
                                                              int T, int H, int pad_key, int accumulate, int NK) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = blockIdx.x * kW + wave;
  const int j0 = c * kHqEmbRunChunk;
  if (j0 >= T) return;
  const int j1 = min(T, j0 + kHqEmbRunChunk);
  const int last = __builtin_amdgcn_readfirstlane(skeys[j1 - 1]);
  if (j1 >= T || skeys[j1] != last || last == pad_key) return;        // the last run ends here (or gets nothing)
  if (skeys[j0] == last && c > 0 && skeys[j0 - 1] == last) return;    // ... or began before: that chunk completes it
  // end of the run: the first sorted position past j1 whose key differs, by a 64-ary search over the sorted keys
  int lo = j1, hi = T;   // skeys[lo] == last; the end lies in (lo, hi]
  while (hi - lo > 1) {
    const int step = (hi - lo + 63) / 64;
    const int q = lo + lane * step;
    const bool in = q < hi && skeys[q] == last;
    const uint64_t m = __ballot(in);   // a non-empty prefix of the lanes (sorted keys, skeys[lo] == last)
    const int k = 63 - __builtin_clzll(m);
    lo = lo + k * step;
    hi = min(hi, lo + step);
  }
  const int ce = (hi - 1) / kHqEmbRunChunk;   // the last chunk holding rows of the run: pieces of chunks c+1 … ce
  HQ_DASSERT(last >= 0 && last < NK && hi <= T && ce * kHqEmbRunChunk < T && ce > c);
  float acc[NC];
#pragma unroll
  for (int q = 0; q < NC; ++q) acc[q] = q * 64 + lane < H ? carry[((size_t)c * 2 + 1) * H + q * 64 + lane] : 0.f;
  for (int cc = c + 1; cc <= ce; ++cc) {
    float v[NC];
#pragma unroll
    for (int q = 0; q < NC; ++q) v[q] = q * 64 + lane < H ? carry[(size_t)cc * 2 * H + q * 64 + lane] : 0.f;
#pragma unroll
    for (int q = 0; q < NC; ++q) acc[q] += v[q];
  }
  float* dst = g_dst + (size_t)last * H;
#pragma unroll
  for (int q = 0; q < NC; ++q) {
    const int col = q * 64 + lane;
    if (col < H) dst[col] = accumulate ? acc[q] + dst[col] : acc[q];
  }
}

}  // namespace

void hq_f32_embed_fwd(const int64_t* ids, const int64_t* pids, const int64_t* tids, const float* ww, const float* wp,
                      const float* wt, const float* gamma, const float* beta, float* y, float* mean, float* rstd, int T, int H,
                      float eps, float p, uint32_t seed, uint32_t opid, int V, int P, int NTY, hipStream_t s) {
  const uint32_t thr = p > 0.f ? hq_threshold(p) : 0u;
  const HqDropKey kd = hq_drop_key(seed, opid);
  dispatch_nc(H, [&](auto nc) {
    hipLaunchKernelGGL(f32_embed_fwd_kernel<decltype(nc)::value>, dim3((T + kW - 1) / kW), dim3(256), 0, s, ids, pids, tids,
                       ww, wp, wt, gamma, beta, y, mean, rstd, T, H, eps, V, P, NTY, kd, thr, hq_keep_scale(thr));
  });
}

void hq_f32_embed_bwd(const float* dy, const int64_t* ids, const int64_t* pids, const int64_t* tids, const float* ww,
                      const float* wp, const float* wt, const float* gamma, const float* mean, const float* rstd,
                      float* g_word, float* g_pos, float* g_type, float* part, HqOuts outs, int T, int H, int pad_word,
                      int pad_pos, float p, uint32_t seed, uint32_t opid, bool accumulate, int V, int P, int NTY,
                      hipStream_t s, const HqEmbScratch* det) {
  const uint32_t thr = p > 0.f ? hq_threshold(p) : 0u;
  const HqDropKey kd = hq_drop_key(seed, opid);
  const float kss = hq_keep_scale(thr);
  const int nb = hq_f32_row_partials(T);
  dispatch_nc(H, [&](auto nc) {
    constexpr int C = decltype(nc)::value;
    auto go = [&](auto kern) {
      hipLaunchKernelGGL(kern, dim3(nb), dim3(256), 0, s, dy, ids, pids, tids, ww, wp, wt, gamma, mean, rstd, g_word, g_pos,
                         g_type, part, T, H, pad_word, pad_pos, V, P, NTY, kd, thr, kss);
    };
    if (det == nullptr) { go(f32_embed_bwd_kernel<C, false>); return; }
    go(f32_embed_bwd_kernel<C, true>);
    // one table at a time through the same scratch (stream order): sort by the table's key, sum the runs, complete
    // the runs that cross chunks.  The type table only when its rows are not the block partials (NTY > 2).
    const int nwb = (hq_emb_run_chunks(T) + kW - 1) / kW;
    auto table = [&](auto run, const int64_t* keys, int NK, float* g_dst, int pad_key) {
      hq_sort_ids(keys, T, NK, det->keys, det->rows, det->skeys, det->srows, det->sort_tmp, det->sort_bytes, s);
      hipLaunchKernelGGL(run, dim3(nwb), dim3(256), 0, s, det->skeys, det->srows, dy, ids, pids, tids, ww, wp, wt, gamma,
                         mean, rstd, g_dst, det->carry, T, H, pad_key, accumulate ? 1 : 0, NK, V, P, NTY, kd, thr, kss);
      hipLaunchKernelGGL(f32_embed_carry_kernel<C>, dim3(nwb), dim3(256), 0, s, det->skeys, det->carry, g_dst, T, H,
                         pad_key, accumulate ? 1 : 0, NK);
    };
    table(f32_embed_run_kernel<C, 0>, ids, V, g_word, pad_word);
    table(f32_embed_run_kernel<C, 1>, pids, P, g_pos, pad_pos);
    if (NTY > 2) table(f32_embed_run_kernel<C, 2>, tids, NTY, g_type, -1);
  });
  hq_f32_fold(part, nb, H, 4, outs, accumulate, s);
}
