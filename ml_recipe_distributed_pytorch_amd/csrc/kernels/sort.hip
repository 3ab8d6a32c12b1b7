// Own stable LSD radix sort of (id, row) pairs on gfx950: 8-bit digits, ceil(bits / 8) passes.  The deterministic
// embedding backward (embed.hip, f32_embed.hip) sorts the token rows by word / position / type id with it.
#include "hq_common.h"
#include "hq_kernels.h"

namespace {

// Each pass is a stable counting sort over 256 bins in tiles of kSortTile rows:
//   sort_hist_kernel (first pass only): per-tile digit counts -> hist[digit][tile] (LDS integer atomics);
//   sort_scan_kernel: one block, exclusive scan of hist in (digit, tile) order -> every tile's start per digit;
//                     also zeroes the next pass's histogram;
//   sort_scatter_kernel: each wave ranks its 64-row batches by digit with 8 ballots (the lanes holding the same
//                     digit, in lane order), batch counts are scanned per digit in LDS, and every row goes to
//                     tile start + earlier batches + rank — stable, so each id's rows keep token order.  It also
//                     counts the NEXT pass's digits of the tile each row lands in (integer atomics).
// Integer counts and fixed ranks: the output is the same permutation every run (no float, no order race).
constexpr int kSortTile = 1024;   // 256 threads × 4 batches of 64

__global__ __launch_bounds__(256) void sort_hist_kernel(const int64_t* __restrict__ ids, int T, int* __restrict__ hist,
                                                        int ntiles) {
  __shared__ int cnt[256];
  cnt[threadIdx.x] = 0;
  __syncthreads();
  const int t0 = blockIdx.x * kSortTile;
  for (int i = threadIdx.x; i < kSortTile; i += 256)
    if (t0 + i < T) atomicAdd(&cnt[(int)ids[t0 + i] & 255], 1);
  __syncthreads();
  hist[threadIdx.x * ntiles + blockIdx.x] = cnt[threadIdx.x];
}

// Exclusive scan of the (digit, tile) histogram by one block: coalesced 16 K-entry chunks through LDS (a thread's
// contiguous run read straight from global memory was latency-bound: 35 µs), each thread scans 16 consecutive
// entries, the 1024 run totals are scanned wave by wave, a running carry links the chunks.
__global__ __launch_bounds__(1024) void sort_scan_kernel(int* __restrict__ hist, int n, int* __restrict__ next_hist) {
  constexpr int kPer = 16, kChunk = 1024 * kPer;
  __shared__ int buf[kChunk];
  __shared__ int wsum[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int carry = 0;
  for (int base = 0; base < n; base += kChunk) {
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
      const int i = base + k * 1024 + tid;
      buf[k * 1024 + tid] = i < n ? hist[i] : 0;
    }
    __syncthreads();
    int v[kPer], run = 0;
#pragma unroll
    for (int k = 0; k < kPer; ++k) { v[k] = buf[tid * kPer + k]; run += v[k]; }
    int incl = run;   // inclusive scan of the run totals within the wave
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int o = __shfl_up(incl, off, 64);
      if (lane >= off) incl += o;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int before = carry;
    for (int w = 0; w < wave; ++w) before += wsum[w];
    int total = carry;
    for (int w = 0; w < 16; ++w) total += wsum[w];
    int ex = before + incl - run;
#pragma unroll
    for (int k = 0; k < kPer; ++k) { buf[tid * kPer + k] = ex; ex += v[k]; }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
      const int i = base + k * 1024 + tid;
      if (i < n) hist[i] = buf[k * 1024 + tid];
    }
    carry = total;
    __syncthreads();
  }
  if (next_hist)
    for (int i = tid; i < n; i += 1024) next_hist[i] = 0;
}

__global__ __launch_bounds__(256) void sort_scatter_kernel(const int64_t* __restrict__ ids, const int32_t* __restrict__ kin,
                                                           const int32_t* __restrict__ vin, int32_t* __restrict__ kout,
                                                           int32_t* __restrict__ vout, const int* __restrict__ start,
                                                           int* __restrict__ next_hist, int T, int shift, int ntiles) {
  __shared__ int bcnt[16][256];   // [batch][digit]: rows of the digit in the batch, then their exclusive prefix
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < 16 * 256; i += 256) (&bcnt[0][0])[i] = 0;
  __syncthreads();
  const int t0 = blockIdx.x * kSortTile;
  const uint64_t lt = (1ull << lane) - 1ull;
  int key[4], val[4], dig[4], rank[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int q = wave * 4 + j;            // batch q covers tile rows q·64 … q·64 + 63 (tile order)
    const int i = t0 + q * 64 + lane;
    const bool ok = i < T;
    key[j] = ok ? (kin ? kin[i] : (int)ids[i]) : 0;
    val[j] = ok ? (vin ? vin[i] : i) : 0;
    dig[j] = (key[j] >> shift) & 255;
    uint64_t peers = __ballot(ok);
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
      const bool on = (dig[j] >> bit) & 1;
      const uint64_t m = __ballot(on);
      peers &= on ? m : ~m;
    }
    rank[j] = __popcll(peers & lt);
    if (ok && rank[j] == 0) bcnt[q][dig[j]] = __popcll(peers);   // the digit's first lane writes the batch count
    if (!ok) rank[j] = -1;
  }
  __syncthreads();
  {   // per digit (one per thread): exclusive prefix over the 16 batches, in batch order
    int run = 0;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int c = bcnt[q][tid];
      bcnt[q][tid] = run;
      run += c;
    }
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (rank[j] < 0) continue;
    const int q = wave * 4 + j;
    const int pos = start[dig[j] * ntiles + blockIdx.x] + bcnt[q][dig[j]] + rank[j];
    HQ_DASSERT(pos >= 0 && pos < T);
    kout[pos] = key[j];
    vout[pos] = val[j];
    if (next_hist) atomicAdd(&next_hist[((key[j] >> (shift + 8)) & 255) * ntiles + pos / kSortTile], 1);
  }
}

}  // namespace

// ================================================================================== launchers
static int emb_sort_bits(int V) { return V > 1 ? 32 - __builtin_clz((unsigned)(V - 1)) : 1; }
static int emb_sort_passes(int V) { return (emb_sort_bits(V) + 7) / 8; }
static int emb_sort_tiles(int T) { return (T + kSortTile - 1) / kSortTile; }

size_t hq_sort_ids_bytes(int T, int V) { return (size_t)emb_sort_passes(V) * 256 * emb_sort_tiles(T) * sizeof(int); }

// Stable sort of (ids[t], t) by id (sort_*_kernel): sorted ids -> skeys, their rows -> srows; keys / rows are the
// ping-pong buffers of the odd passes (all [T]); hist: hq_sort_ids_bytes(T, V) bytes.  Passes alternate so that
// the last one lands in (skeys, srows).
void hq_sort_ids(const int64_t* ids, int T, int V, int32_t* keys, int32_t* rows, int32_t* skeys, int32_t* srows,
                 void* hist_buf, size_t hist_bytes, hipStream_t s) {
  const int np = emb_sort_passes(V), nt = emb_sort_tiles(T);
  if (T <= 0) return;
  if (hist_bytes < hq_sort_ids_bytes(T, V)) {
    fprintf(stderr, "hq_sort_ids: histogram scratch too small (%zu < %zu)\n", hist_bytes, hq_sort_ids_bytes(T, V));
    abort();
  }
  int* hist = reinterpret_cast<int*>(hist_buf);
  hipLaunchKernelGGL(sort_hist_kernel, dim3(nt), dim3(256), 0, s, ids, T, hist, nt);
  const int32_t *kin = nullptr, *vin = nullptr;
  for (int p = 0; p < np; ++p) {
    int* h = hist + (size_t)p * 256 * nt;
    int* hn = p + 1 < np ? h + 256 * nt : nullptr;
    const bool to_final = (np - 1 - p) % 2 == 0;
    int32_t* kout = to_final ? skeys : keys;
    int32_t* vout = to_final ? srows : rows;
    hipLaunchKernelGGL(sort_scan_kernel, dim3(1), dim3(1024), 0, s, h, 256 * nt, hn);
    hipLaunchKernelGGL(sort_scatter_kernel, dim3(nt), dim3(256), 0, s, ids, kin, vin, kout, vout, h, hn, T, 8 * p, nt);
    kin = kout;
    vin = vout;
  }
}
