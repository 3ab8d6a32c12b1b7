// Embedding layer of the BERT encoder (gfx950, wave64; the row layout of hq_rowops.h).
//
//   embed_fwd: y = dropout(LN(word[id] + pos[pid] + type[tid]))
//   embed_bwd: recompute x̂, LN_bwd; word grads summed per id over the id-sorted rows (no atomics),
//              position grads summed per wave over the batch (position-major walk) into partial rows,
//              type/γ/β grads through deterministic partials
//
// Column partial sums are reduced per block through LDS and finished by hq_colsum_outs (rowops.hip), so every
// gradient is bitwise deterministic (position ids other than 0 … L-1 and more than 2 types scatter those rows with
// float atomics by default; hq_embed_bwd's det_pos / det_type modes sum them over pid- / tid-sorted runs instead).

#include "hq_common.h"
#include "hq_kernels.h"
#include "hq_rowops.h"

namespace {

template <int NCH>
__global__ __launch_bounds__(256) void embed_fwd_kernel(const int64_t* __restrict__ ids, const int64_t* __restrict__ pids,
                                                        const int64_t* __restrict__ tids, const uint16_t* __restrict__ ww,
                                                        const uint16_t* __restrict__ wp, const uint16_t* __restrict__ wt,
                                                        const float* __restrict__ gamma, const float* __restrict__ beta,
                                                        uint16_t* __restrict__ y, float* __restrict__ mean_out,
                                                        float* __restrict__ rstd_out, int T, int H, float eps, HqDropKey kd_,
                                                        uint32_t thr, float kscale, int V, int P, int NTY) {
  const uint32_t key = kd_.get();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = blockIdx.x * kWaves + wave;
  if (row >= T) return;
  HQ_DASSERT(ids[row] >= 0 && ids[row] < V && pids[row] >= 0 && pids[row] < P && tids[row] >= 0 && tids[row] < NTY);
  const size_t rw = (size_t)ids[row] * H, rp = (size_t)pids[row] * H, rt = (size_t)tids[row] * H;
  float v[NCH][4];
  float sum = 0.f;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int col = c * 256 + lane * 4;
    if (col < H) {
      float f1[4], f2[4], f3[4];
      hq_unpack4(*reinterpret_cast<const uint2*>(ww + rw + col), f1);
      hq_unpack4(*reinterpret_cast<const uint2*>(wp + rp + col), f2);
      hq_unpack4(*reinterpret_cast<const uint2*>(wt + rt + col), f3);
#pragma unroll
      for (int i = 0; i < 4; ++i) { v[c][i] = f1[i] + f2[i] + f3[i]; sum += v[c][i]; }
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) v[c][i] = 0.f;
    }
  }
  const float mu = hq_wave_sum(sum) / H;
  float sq = 0.f;
#pragma unroll
  for (int c = 0; c < NCH; ++c)
    if (c * 256 + lane * 4 < H)
#pragma unroll
      for (int i = 0; i < 4; ++i) { float d = v[c][i] - mu; sq += d * d; }
  const float rs = rsqrtf(hq_wave_sum(sq) / H + eps);
  const size_t base = (size_t)row * H;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int col = c * 256 + lane * 4;
    if (col < H) {
      const float4 g = *reinterpret_cast<const float4*>(gamma + col);
      const float4 b = *reinterpret_cast<const float4*>(beta + col);
      float m[4] = {1.f, 1.f, 1.f, 1.f};
      if (thr) hq_keep4((uint32_t)(base + col), key, thr, kscale, m);
      float o[4] = {((v[c][0] - mu) * rs * g.x + b.x) * m[0], ((v[c][1] - mu) * rs * g.y + b.y) * m[1],
                    ((v[c][2] - mu) * rs * g.z + b.z) * m[2], ((v[c][3] - mu) * rs * g.w + b.w) * m[3]};
      *reinterpret_cast<uint2*>(y + base + col) = hq_pack4(o);
    }
  }
  if (lane == 0) { mean_out[row] = mu; rstd_out[row] = rs; }
}

// Deterministic embedding backward (no float atomics at the default position ids):
//   1. sort: the token rows by word id (hq_sort_ids: own LSD radix sort of (id, row) pairs — stable, so each
//      id's rows stay in token order);
//   2. embed_bwd_kernel (position-major): recompute x̂ and the LayerNorm backward per row; γ / β / type
//      gradients as per-block partials, the position gradient summed per wave over its kEmbNB batch rows and
//      stored as that wave's partial row [blockIdx.y][l] (folded by colsum in a fixed order);
//   3. embed_word_kernel (id-major): the same per-row recompute over the SORTED rows, kEmbCH per wave, summing
//      each id's run in registers; a run inside the chunk is stored straight into its gradient row, the
//      pieces of a run that crosses chunk boundaries go to two carry rows per chunk;
//   4. embed_carry_kernel: the chunk where a crossing run starts adds its pieces in chunk order.
// Every sum has a fixed order, so the result is bitwise reproducible (the round-4 kernel scattered 75 M f32
// atomics into the word gradients: 316 µs at T = 98304 and run-to-run different low bits).
// Position ids other than l (RoBERTa's, user-supplied ids) fall back to f32 atomics for those rows by default, as
// do the type rows of more than 2 types.  The caller-selected deterministic modes remove both: det_pos runs
// embed_bwd_kernel without any position work and takes every position gradient from a sort of the position ids
// plus the position instantiation of steps 3-4; det_type does the same for the type rows with the type ids.
//
// part layout per block: [gamma | beta | type0 | type1] × H
//
// Position-major traversal: wave w of block (x, y) owns sequence position l = x·4 + w and walks the
// kEmbNB batch rows b = y·kEmbNB … (row = b·L + l).  The next row's dy / embedding rows / statistics are
// loaded while the current row is reduced (one dependent HBM round trip per row otherwise).
constexpr int kEmbNB = 16;       // batch rows per wave in the position pass (<= 64, as kEmbCH)
constexpr int kEmbCH = kHqEmbRunChunk;   // sorted rows per wave in the sorted-run pass (16; <= 64: one row's metadata per lane)
constexpr int kEmbMaxL = 4096;   // position partials [T / L / kEmbNB][min(L, P)][H] only for real sequence layouts

template <int NCH>
struct EmbRow {
  int64_t id, pid, tid;
  float mu, rs;
  uint2 w[NCH], p[NCH], t[NCH], d[NCH];
};

// Row metadata of up to 64 rows, one row per lane (ids, position / type ids, LayerNorm statistics), loaded once
// up front: the per-row loop then reads them with v_readlane and issues only the row-data loads — no dependent
// index → row round trip inside the loop.
struct EmbMeta {
  int id, pid, tid;
  float mu, rs;
};
__device__ __forceinline__ EmbMeta emb_meta_load(int64_t row, bool ok, const int64_t* __restrict__ ids,
                                                 const int64_t* __restrict__ pids, const int64_t* __restrict__ tids,
                                                 const float* __restrict__ mean, const float* __restrict__ rstd) {
  EmbMeta m{0, 0, 0, 0.f, 0.f};
  if (ok) { m.id = (int)ids[row]; m.pid = (int)pids[row]; m.tid = (int)tids[row]; m.mu = mean[row]; m.rs = rstd[row]; }
  return m;
}
// row data of the row whose metadata lane k holds
template <int NCH>
__device__ __forceinline__ void emb_load_k(EmbRow<NCH>& r, const EmbMeta& m, int k, size_t row, const uint16_t* __restrict__ dy,
                                           const uint16_t* __restrict__ ww, const uint16_t* __restrict__ wp,
                                           const uint16_t* __restrict__ wt, int H, int lane) {
  r.id = __builtin_amdgcn_readlane(m.id, k);
  r.pid = __builtin_amdgcn_readlane(m.pid, k);
  r.tid = __builtin_amdgcn_readlane(m.tid, k);
  r.mu = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(m.mu), k));
  r.rs = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(m.rs), k));
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int col = c * 256 + lane * 4;
    if (col < H) {
      r.w[c] = *reinterpret_cast<const uint2*>(ww + (size_t)r.id * H + col);
      r.p[c] = *reinterpret_cast<const uint2*>(wp + (size_t)r.pid * H + col);
      r.t[c] = *reinterpret_cast<const uint2*>(wt + (size_t)r.tid * H + col);
      r.d[c] = *reinterpret_cast<const uint2*>(dy + row * H + col);
    }
  }
}

// One row's LayerNorm backward from the recomputed x̂: g = dropout-masked dy, x̂, and dx = ∂/∂(word+pos+type).
template <int NCH>
__device__ __forceinline__ void emb_row_grad(const EmbRow<NCH>& cur, size_t base, const float (&gam)[NCH][4],
                                             uint32_t key, uint32_t thr, float kscale, int H, int lane,
                                             float (&g)[NCH][4], float (&xh)[NCH][4], float (&dx)[NCH][4]) {
  const float mu = cur.mu, rs = cur.rs;
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int col = c * 256 + lane * 4;
    if (col < H) {
      float f1[4], f2[4], f3[4], m[4] = {1.f, 1.f, 1.f, 1.f};
      hq_unpack4(cur.w[c], f1);
      hq_unpack4(cur.p[c], f2);
      hq_unpack4(cur.t[c], f3);
      hq_unpack4(cur.d[c], g[c]);
      if (thr) hq_keep4((uint32_t)(base + col), key, thr, kscale, m);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        g[c][i] *= m[i];
        xh[c][i] = (f1[i] + f2[i] + f3[i] - mu) * rs;
        const float dxh = g[c][i] * gam[c][i];
        s1 += dxh;
        s2 += dxh * xh[c][i];
      }
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) { g[c][i] = 0.f; xh[c][i] = 0.f; }
    }
  }
  s1 = hq_wave_sum(s1) / H;
  s2 = hq_wave_sum(s2) / H;
#pragma unroll
  for (int c = 0; c < NCH; ++c)
#pragma unroll
    for (int i = 0; i < 4; ++i) dx[c][i] = c * 256 + lane * 4 < H ? rs * (g[c][i] * gam[c][i] - s1 - xh[c][i] * s2) : 0.f;
}

template <int NCH>
__device__ __forceinline__ void emb_gamma(const float* __restrict__ gamma, int H, int lane, float (&gam)[NCH][4]) {
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int col = c * 256 + lane * 4;
    const float4 g = col < H ? *reinterpret_cast<const float4*>(gamma + col) : make_float4(0.f, 0.f, 0.f, 0.f);
    gam[c][0] = g.x; gam[c][1] = g.y; gam[c][2] = g.z; gam[c][3] = g.w;
  }
}

// NOPOS (deterministic-positions mode): no position work at all — no partial rows, no flushes; the position
// gradients come from the position instantiation of embed_word_kernel.  NOTYPE: likewise no type atomics at
// n_types > 2 (the type instantiation).  <NCH, false, false> is the kernel as it always was.
template <int NCH, bool NOPOS = false, bool NOTYPE = false>
__global__ __launch_bounds__(256) void embed_bwd_kernel(
    const uint16_t* __restrict__ dy, const int64_t* __restrict__ ids, const int64_t* __restrict__ pids,
    const int64_t* __restrict__ tids, const uint16_t* __restrict__ ww, const uint16_t* __restrict__ wp,
    const uint16_t* __restrict__ wt, const float* __restrict__ gamma, const float* __restrict__ mean,
    const float* __restrict__ rstd, float* __restrict__ g_pos, float* __restrict__ g_type, float* __restrict__ ppart,
    float* __restrict__ part, int T, int H, int n_types, int pad_pos, HqDropKey kd_, uint32_t thr, float kscale, int V,
    int P, int B, int L, int PL) {
  const uint32_t key = kd_.get();
  extern __shared__ __attribute__((aligned(16))) float lds[];  // [4][H] block-partial scratch
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  float acc[4][NCH][4];
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[q][c][i] = 0.f;
  float gam[NCH][4], pacc[NCH][4];
  emb_gamma<NCH>(gamma, H, lane, gam);
#pragma unroll
  for (int c = 0; c < NCH; ++c)
#pragma unroll
    for (int i = 0; i < 4; ++i) pacc[c][i] = 0.f;
  const int l = blockIdx.x * kWaves + wave;
  // this wave's position-partial row [blockIdx.y][l] (l < PL = min(L, P): pid == l needs l < P; ppart = null:
  // every position flush is atomic)
  float* prow = (!NOPOS && ppart != nullptr && l < PL) ? ppart + ((size_t)blockIdx.y * PL + l) * H : nullptr;
  // the partial rows are [ceil(B / kEmbNB)][PL][H] with PL = min(L, P): row l exists only for l < PL (77ab202: the
  // flat layout, L = T > P, once wrote rows past the buffer)
  HQ_DASSERT(prow == nullptr || (l < PL && PL <= P && (int)blockIdx.y < (B + kEmbNB - 1) / kEmbNB));
  bool pstored = false;
  int pcur = -1;
  auto flush_pos = [&]() {
    if (pcur >= 0 && pcur != pad_pos) {
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const int col = c * 256 + lane * 4;
        if (col < H) {
          if (prow != nullptr && pcur == l) {   // the default ids: the wave's own partial row, plain stores
            float4 v = make_float4(pacc[c][0], pacc[c][1], pacc[c][2], pacc[c][3]);
            if (pstored) {
              const float4 o = *reinterpret_cast<const float4*>(prow + col);
              v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w;
            }
            *reinterpret_cast<float4*>(prow + col) = v;
          } else {
            HQ_DASSERT(pcur >= 0 && pcur < P);
#pragma unroll
            for (int i = 0; i < 4; ++i) atomicAdd(g_pos + (size_t)pcur * H + col + i, pacc[c][i]);
          }
        }
      }
      if (prow != nullptr && pcur == l) pstored = true;
    }
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
      for (int i = 0; i < 4; ++i) pacc[c][i] = 0.f;
  };
  const int b0 = blockIdx.y * kEmbNB, b1 = l < L ? min(B, b0 + kEmbNB) : b0;
  // rows two ahead in a ring of three (compile-time slots in the unrolled loop: a rotation by copies would wait
  // for the newest loads at every copy)
  const EmbMeta meta = emb_meta_load((int64_t)(b0 + lane) * L + l, lane < b1 - b0, ids, pids, tids, mean, rstd);
  EmbRow<NCH> cur, nxt;
  if (b0 < b1) emb_load_k<NCH>(nxt, meta, 0, (size_t)b0 * L + l, dy, ww, wp, wt, H, lane);
#pragma unroll 1
  for (int b = b0; b < b1; ++b) {
    const size_t row = (size_t)b * L + l;
    cur = nxt;
    if (b + 1 < b1) emb_load_k<NCH>(nxt, meta, b + 1 - b0, row + L, dy, ww, wp, wt, H, lane);
    const int64_t pid = cur.pid, tid = cur.tid;
    HQ_DASSERT(cur.id >= 0 && cur.id < V && pid >= 0 && pid < P && tid >= 0 && tid < n_types);
    float g[NCH][4], xh[NCH][4], dx[NCH][4];
    emb_row_grad<NCH>(cur, row * H, gam, key, thr, kscale, H, lane, g, xh, dx);
    if (!NOPOS && (int)pid != pcur) {  // wave-uniform: the running position sum belongs to another position
      flush_pos();
      pcur = (int)pid;
    }
    const bool t1 = (tid & 1) != 0;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int col = c * 256 + lane * 4;
      if (col < H) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          acc[0][c][i] += g[c][i] * xh[c][i];
          acc[1][c][i] += g[c][i];
          if (!NOPOS) pacc[c][i] += dx[c][i];
        }
        if (n_types <= 2) {  // static indices only: acc[2 + (tid & 1)] put the whole array in scratch memory
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            acc[2][c][i] += t1 ? 0.f : dx[c][i];
            acc[3][c][i] += t1 ? dx[c][i] : 0.f;
          }
        } else if (!NOTYPE) {
#pragma unroll
          for (int i = 0; i < 4; ++i) atomicAdd(g_type + (size_t)tid * H + col + i, dx[c][i]);
        }
      }
    }
  }
  if (!NOPOS) flush_pos();
  if (prow != nullptr && !pstored) {   // no row at position l in this batch slice: a zero partial
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int col = c * 256 + lane * 4;
      if (col < H) *reinterpret_cast<float4*>(prow + col) = make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  __syncthreads();
  block_partials<NCH, 4>(acc, lds, part, H);
}

// ---- table gradients over key-sorted runs (this file's embed_word_kernel / embed_carry_kernel and the fp32 pair
// f32_embed_run_kernel / f32_embed_carry_kernel of f32_embed.hip) -----------------------------------------------
// One pair of kernels serves the word, position and type tables; KEY picks which id of a token is the key
// (0: ids, 1: pids, 2: tids).  The tokens are sorted by key with the stable hq_sort_ids, so the tokens of one key
// (its "run") are contiguous in the sorted list and stay in token order.  The summation order of a table row is:
//   * the sorted list is cut into chunks of kHqEmbRunChunk consecutive sorted positions, chunk c =
//     [c·kHqEmbRunChunk, (c+1)·kHqEmbRunChunk), one wave per chunk; the rows of ONE key inside ONE chunk form a piece;
//   * a piece is summed from zero in token order: piece = ((0 + dx[t0]) + dx[t1]) + …, every dx recomputed by the
//     wave exactly as the position-major backward kernel of its precision computes it;
//   * a run that lies inside one chunk is one piece; a run that crosses chunk boundaries has one piece per chunk
//     it touches, and the pieces are added in chunk order onto the first: total = ((piece_c + piece_c+1) + …);
//   * accumulate adds the existing table row last: row = total + row; fresh stores row = total;
//   * the skipped key (the padding id / padding position) gets no gradient, a key that never occurs keeps its row.
// Pieces of crossing runs travel through the carry buffer [chunks][2][H]: slot 0 of chunk c holds the chunk's first
// piece when its run began in an earlier chunk (a run covering the whole chunk from both sides is slot 0), slot 1 the
// chunk's last piece when its run began in this chunk and continues into the next; the carry kernel, run by the
// chunk that holds slot 1, completes the row.
//
// Here: dx comes from emb_row_grad (as in embed_bwd_kernel), lane owns 4 consecutive columns per 256-column chunk.
// KEY picks the table (0: word ids -> g_word, 1: position ids -> g_pos in the deterministic-positions mode, 2: type
// ids -> g_type at n_types > 2); g_word / pad_word / V are then that table's gradient, skipped key and row count.
template <int NCH, int KEY = 0>
__global__ __launch_bounds__(256) void embed_word_kernel(
    const int32_t* __restrict__ skeys, const int32_t* __restrict__ srows, const uint16_t* __restrict__ dy,
    const int64_t* __restrict__ ids, const int64_t* __restrict__ pids, const int64_t* __restrict__ tids,
    const uint16_t* __restrict__ ww, const uint16_t* __restrict__ wp, const uint16_t* __restrict__ wt,
    const float* __restrict__ gamma, const float* __restrict__ mean, const float* __restrict__ rstd,
    float* __restrict__ g_word, float* __restrict__ carry, int T, int H, int pad_word, int accumulate, HqDropKey kd_,
    uint32_t thr, float kscale, int V) {
  const uint32_t key = kd_.get();
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int c = blockIdx.x * kWaves + wave;
  const int j0 = c * kEmbCH;
  if (j0 >= T) return;
  const int j1 = min(T, j0 + kEmbCH);
  float gam[NCH][4], acc[NCH][4];
  emb_gamma<NCH>(gamma, H, lane, gam);
#pragma unroll
  for (int q = 0; q < NCH; ++q)
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[q][i] = 0.f;
  const int first = __builtin_amdgcn_readfirstlane(skeys[j0]);
  const bool head_cont = c > 0 && __builtin_amdgcn_readfirstlane(skeys[j0 - 1]) == first;
  const int after = j1 < T ? __builtin_amdgcn_readfirstlane(skeys[j1]) : -1;
  auto flush = [&](int id, int kind) {   // kind 0: carry slot 0, 1: carry slot 1, 2: the gradient row
    if (id != pad_word) {
      // a gradient row of a real id, or carry slot (c, kind) of the [chunks][2][H] carry buffer
      HQ_DASSERT(kind == 2 ? (id >= 0 && id < V) : (kind >= 0 && kind < 2 && c * kEmbCH < T));
      float* dst = kind == 2 ? g_word + (size_t)id * H : carry + ((size_t)c * 2 + kind) * H;
#pragma unroll
      for (int q = 0; q < NCH; ++q) {
        const int col = q * 256 + lane * 4;
        if (col < H) {
          float4 v = make_float4(acc[q][0], acc[q][1], acc[q][2], acc[q][3]);
          if (kind == 2 && accumulate) {
            const float4 o = *reinterpret_cast<const float4*>(dst + col);
            v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w;
          }
          *reinterpret_cast<float4*>(dst + col) = v;
        }
      }
    }
#pragma unroll
    for (int q = 0; q < NCH; ++q)
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[q][i] = 0.f;
  };
  int seg = first;
  bool seg_first = true;
  // the chunk's sorted rows and their metadata, one per lane (kEmbCH <= 64)
  const int myrow = lane < j1 - j0 ? srows[j0 + lane] : 0;
  const EmbMeta meta = emb_meta_load(myrow, lane < j1 - j0, ids, pids, tids, mean, rstd);
  EmbRow<NCH> cur, nxt;
  emb_load_k<NCH>(nxt, meta, 0, (size_t)__builtin_amdgcn_readlane(myrow, 0), dy, ww, wp, wt, H, lane);
#pragma unroll 1
  for (int j = j0; j < j1; ++j) {
    const size_t row = (size_t)__builtin_amdgcn_readlane(myrow, j - j0);
    cur = nxt;
    if (j + 1 < j1)
      emb_load_k<NCH>(nxt, meta, j + 1 - j0, (size_t)__builtin_amdgcn_readlane(myrow, j + 1 - j0), dy, ww, wp, wt, H, lane);
    const int id = (int)(KEY == 0 ? cur.id : (KEY == 1 ? cur.pid : cur.tid));   // the row's key
    HQ_DASSERT(id >= 0 && id < V && row < (size_t)T && id == skeys[j]);
    if (id != seg) {
      flush(seg, seg_first && head_cont ? 0 : 2);
      seg = id;
      seg_first = false;
    }
    float g[NCH][4], xh[NCH][4], dx[NCH][4];
    emb_row_grad<NCH>(cur, row * H, gam, key, thr, kscale, H, lane, g, xh, dx);
#pragma unroll
    for (int q = 0; q < NCH; ++q)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        // a plain add of the row's rounded dx (never a multiply fused into the running sum): the piece is the
        // sum of its rows' dx, which is the documented order
#pragma clang fp contract(off)
        acc[q][i] += dx[q][i];
      }
  }
  const bool from_prev = seg_first && head_cont;
  flush(seg, from_prev ? 0 : (after == seg ? 1 : 2));
}

// Runs that cross chunk boundaries: the chunk holding a run's start piece (carry slot 1) adds the following
// chunks' slot-0 pieces in chunk order and stores the gradient row.
template <int NCH>
__global__ __launch_bounds__(256) void embed_carry_kernel(const int32_t* __restrict__ skeys, const float* __restrict__ carry,
                                                          float* __restrict__ g_word, int T, int H, int pad_word,
                                                          int accumulate, int V) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int c = blockIdx.x * kWaves + wave;
  const int j0 = c * kEmbCH;
  if (j0 >= T) return;
  const int j1 = min(T, j0 + kEmbCH);
  const int last = __builtin_amdgcn_readfirstlane(skeys[j1 - 1]);
  if (j1 >= T || skeys[j1] != last || last == pad_word) return;                  // the last run ends here
  if (skeys[j0] == last && c > 0 && skeys[j0 - 1] == last) return;               // ... or began before
  // end of the run: the first sorted position past j1 whose key differs, by a 64-ary search over the sorted keys
  int lo = j1, hi = T;   // skeys[lo] == last; the end lies in (lo, hi]
  while (hi - lo > 1) {
    const int step = (hi - lo + 63) / 64;
    const int q = lo + lane * step;
    const bool in = q < hi && skeys[q] == last;
    const uint64_t m = __ballot(in);   // a prefix of the lanes (sorted keys)
    const int k = 63 - __builtin_clzll(m);
    lo = lo + k * step;
    hi = min(hi, lo + step);
  }
  const int ce = (hi - 1) / kEmbCH;   // the last chunk holding rows of the run: pieces of chunks c+1 … ce
  HQ_DASSERT(last >= 0 && last < V && hi <= T && ce * kEmbCH < T && ce > c);
  float acc[NCH][4];
#pragma unroll
  for (int q = 0; q < NCH; ++q) {
    const int col = q * 256 + lane * 4;
    const float4 v = col < H ? *reinterpret_cast<const float4*>(carry + ((size_t)c * 2 + 1) * H + col)
                             : make_float4(0.f, 0.f, 0.f, 0.f);
    acc[q][0] = v.x; acc[q][1] = v.y; acc[q][2] = v.z; acc[q][3] = v.w;
  }
  for (int cc = c + 1; cc <= ce; cc += 8) {   // 8 pieces in flight, added in chunk order
    float4 v[8][NCH];
#pragma unroll
    for (int u = 0; u < 8; ++u)
#pragma unroll
      for (int q = 0; q < NCH; ++q) {
        const int col = q * 256 + lane * 4;
        v[u][q] = (cc + u <= ce && col < H) ? *reinterpret_cast<const float4*>(carry + ((size_t)(cc + u) * 2) * H + col)
                                            : make_float4(0.f, 0.f, 0.f, 0.f);
      }
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (cc + u <= ce)
#pragma unroll
        for (int q = 0; q < NCH; ++q) {
          acc[q][0] += v[u][q].x; acc[q][1] += v[u][q].y; acc[q][2] += v[u][q].z; acc[q][3] += v[u][q].w;
        }
  }
  float* dst = g_word + (size_t)last * H;
#pragma unroll
  for (int q = 0; q < NCH; ++q) {
    const int col = q * 256 + lane * 4;
    if (col < H) {
      float4 v = make_float4(acc[q][0], acc[q][1], acc[q][2], acc[q][3]);
      if (accumulate) {
        const float4 o = *reinterpret_cast<const float4*>(dst + col);
        v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w;
      }
      *reinterpret_cast<float4*>(dst + col) = v;
    }
  }
}

}  // namespace

// ================================================================================== launchers
int hq_embed_bwd_partials(int T, int L) {
  if (L <= 0 || T % L) L = T;
  return ((L + kWaves - 1) / kWaves) * ((T / L + kEmbNB - 1) / kEmbNB);
}

void hq_embed_fwd(const int64_t* ids, const int64_t* pids, const int64_t* tids, const uint16_t* ww, const uint16_t* wp,
                  const uint16_t* wt, const float* gamma, const float* beta, uint16_t* y, float* mean, float* rstd, int T,
                  int H, float eps, float p, uint32_t seed, uint32_t opid, int V, int P, int NTY, hipStream_t s) {
  const uint32_t thr = p > 0.f ? hq_threshold(p) : 0u;
  const HqDropKey key = hq_drop_key(seed, opid);
  const float ks = hq_keep_scale(thr);
  dispatch_nch(H, [&](auto nch) {
    hipLaunchKernelGGL(embed_fwd_kernel<decltype(nch)::value>, dim3((T + kWaves - 1) / kWaves), dim3(256), 0, s, ids,
                       pids, tids, ww, wp, wt, gamma, beta, y, mean, rstd, T, H, eps, key, thr, ks, V, P, NTY);
  });
}

HqEmbScratchSizes hq_embed_bwd_scratch(int T, int V, int L, int P) {
  HqEmbScratchSizes z{};
  z.sort_bytes = hq_sort_ids_bytes(T, V);   // one [256][tiles] digit histogram per radix pass
  z.chunks = (T + kEmbCH - 1) / kEmbCH;
  if (L <= 0 || T % L) L = T;
  // partial rows exist for the positions l < min(L, P) only: a row whose pid == l needs l < P
  z.pos_rows = L <= kEmbMaxL ? ((T / L + kEmbNB - 1) / kEmbNB) * std::min(L, P) : 0;
  return z;
}

void hq_embed_bwd(const uint16_t* dy, const int64_t* ids, const int64_t* pids, const int64_t* tids, const uint16_t* ww,
                  const uint16_t* wp, const uint16_t* wt, const float* gamma, const float* mean, const float* rstd,
                  float* g_word, float* g_pos, float* g_type, float* part, HqOuts outs, int T, int H,
                  int n_types, int pad_word, int pad_pos, float p, uint32_t seed, uint32_t opid, bool accumulate,
                  int V, int P, int L, const HqEmbScratch& sc, hipStream_t s, bool det_pos, bool det_type) {
  const uint32_t thr = p > 0.f ? hq_threshold(p) : 0u;
  const HqDropKey key = hq_drop_key(seed, opid);
  const float ks = hq_keep_scale(thr);
  if (L <= 0 || T % L) L = T;  // rows are b·L + l; any other layout is one "sequence" of T positions
  const int B = T / L;
  const dim3 grid((L + kWaves - 1) / kWaves, (B + kEmbNB - 1) / kEmbNB);
  const int nb = hq_embed_bwd_partials(T, L);
  const HqEmbScratchSizes z = hq_embed_bwd_scratch(T, V, L, P);
  const int PL = std::min(L, P);   // position-partial rows per batch slice
  float* ppart = (z.pos_rows > 0 && !det_pos) ? sc.ppart : nullptr;
  det_type = det_type && n_types > 2;   // n_types <= 2: the type rows are block partials, no atomics to replace
  // (id, row) sort: the own stable radix sort, so every id's rows stay in token order
  hq_sort_ids(ids, T, V, sc.keys, sc.rows, sc.skeys, sc.srows, sc.sort_tmp, sc.sort_bytes, s);
  const int nwb = (z.chunks + kWaves - 1) / kWaves;
  dispatch_nch(H, [&](auto nch) {
    constexpr int C = decltype(nch)::value;
    auto bwd = [&](auto kern) {
      hipLaunchKernelGGL(kern, grid, dim3(256), 4 * H * sizeof(float), s, dy, ids, pids, tids, ww, wp, wt, gamma, mean,
                         rstd, g_pos, g_type, ppart, part, T, H, n_types, pad_pos, key, thr, ks, V, P, B, L, PL);
    };
    if (det_pos) { if (det_type) bwd(embed_bwd_kernel<C, true, true>); else bwd(embed_bwd_kernel<C, true, false>); }
    else if (det_type) bwd(embed_bwd_kernel<C, false, true>);
    else bwd(embed_bwd_kernel<C>);
    // the rows sorted by one table's key: sum the runs, complete the runs that cross chunks
    auto table = [&](auto run, float* g_dst, int pad_key, int NK) {
      hipLaunchKernelGGL(run, dim3(nwb), dim3(256), 0, s, sc.skeys, sc.srows, dy, ids, pids, tids, ww, wp, wt, gamma, mean,
                         rstd, g_dst, sc.carry, T, H, pad_key, accumulate ? 1 : 0, key, thr, ks, NK);
      hipLaunchKernelGGL(embed_carry_kernel<C>, dim3(nwb), dim3(256), 0, s, sc.skeys, sc.carry, g_dst, T, H, pad_key,
                         accumulate ? 1 : 0, NK);
    };
    table(embed_word_kernel<C>, g_word, pad_word, V);
    // deterministic modes: the same sort scratch and carry rows, one table after the other (stream order)
    if (det_pos) {
      hq_sort_ids(pids, T, P, sc.keys, sc.rows, sc.skeys, sc.srows, sc.sort_tmp, sc.sort_bytes, s);
      table(embed_word_kernel<C, 1>, g_pos, pad_pos, P);
    }
    if (det_type) {
      hq_sort_ids(tids, T, n_types, sc.keys, sc.rows, sc.skeys, sc.srows, sc.sort_tmp, sc.sort_bytes, s);
      table(embed_word_kernel<C, 2>, g_type, -1, n_types);
    }
  });
  // outs: gamma, beta, type0, type1 (type rows only when n_types <= 2)
  hq_colsum_outs(part, nb, 4 * H, outs, H, accumulate, s);
  // position partials [B / kEmbNB][min(L, P)][H] -> rows 0 … min(L, P)-1 of g_pos, on top of its zeroed (or
  // accumulated) rows and the atomic flushes of non-default position ids
  if (ppart)
    hq_colsum_outs(ppart, (B + kEmbNB - 1) / kEmbNB, PL * H, HqOuts{{g_pos, nullptr, nullptr, nullptr}}, PL * H, true, s);
}
