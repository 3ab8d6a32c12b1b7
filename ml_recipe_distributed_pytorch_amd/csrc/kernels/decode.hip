// Joint valid-span decoding for QA inference (gfx950, wave64): for every chunk the best (start, end) pair inside the
// document window with a bounded answer length, the rule of arXiv:1901.08634 — not two independent argmaxes.
//
// Semantics (ops/reference.py::qa_decode is the same definition in torch; the two agree bit for bit):
//   lo' = clamp(lo, 0, L), hi' = clamp(hi, 0, L)
//   C     = {(s, e) : lo' <= s <= e < hi', e - s < W}
//   key   = fl32(start[s] + end[e])                     one rounded add
//   winner: largest key, then smallest s, then smallest e
//   score = fl32(key - fl32(start[0] + end[0]))
//   C empty: s = e = -1, score = -inf
//   label = first argmax of cls[b, :NL]
//   out[b] = (score, s, e, start_reg, end_reg, label)   indices <= 512 are exact in fp32
// There is no multiply anywhere, so nothing contracts to an FMA.
//
// Work split: one wave per row, four rows per 256-thread block.  The wave stages the row's start and end logits
// in its own LDS slice (2 x 512 floats), lane i owns s = lo' + i, lo' + i + 64, ... and walks e upward with a strict
// `>` (first occurrence wins inside the lane: its s ascend, and for one s its e ascend).  Lanes hold interleaved s,
// so the wave reduction compares (key, s, e) in full instead of relying on lane order.  O(L·min(W, L)) LDS reads
// per row; lanes of one wave read consecutive end[] words (s consecutive, same e - s), so no bank conflicts.
// The LDS slices are wave-private; the one block barrier between staging and search is reached by every wave,
// including those whose row is past B (they skip the work, not the barrier).
#include "hq_common.h"
#include "hq_kernels.h"

namespace {

constexpr int kRows = 4;   // rows (waves) per block

struct Best {
  float key;
  int s, e;   // s < 0: no candidate yet
};

// true when b beats a: greater key, then smaller s, then smaller e; a lane without a candidate loses to any with one
__device__ __forceinline__ bool beats(const Best& b, const Best& a) {
  if (b.s < 0) return false;
  if (a.s < 0) return true;
  if (b.key != a.key) return b.key > a.key;
  if (b.s != a.s) return b.s < a.s;
  return b.e < a.e;
}

template <bool INTER>
__global__ __launch_bounds__(256) void qa_decode_kernel(HqDecodeIn in, float* __restrict__ out, int B, int L, int NL,
                                                        int W) {
  __shared__ float lds[kRows][2][kHqDecodeMaxL];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int b = blockIdx.x * kRows + wv;
  const bool live = b < B;   // wave-uniform
  float* st = lds[wv][0];
  float* en = lds[wv][1];
  if (live) {
    if constexpr (INTER) {
      const float2* row = reinterpret_cast<const float2*>(in.start + (long long)b * in.start_row);
      for (int j = lane; j < L; j += 64) {
        const float2 z = row[j];
        st[j] = z.x;
        en[j] = z.y;
      }
    } else {
      const float* srow = in.start + (long long)b * in.start_row;
      const float* erow = in.end + (long long)b * in.end_row;
      for (int j = lane; j < L; j += 64) {
        st[j] = srow[(long long)j * in.start_elem];
        en[j] = erow[(long long)j * in.end_elem];
      }
    }
  }
  __syncthreads();
  if (!live) return;
  const int lo = min(max(in.lo[b], 0), L), hi = min(max(in.hi[b], 0), L);
  Best best{-INFINITY, -1, -1};
  for (int s = lo + lane; s < hi; s += 64) {
    const float vs = st[s];
    const int e1 = min(s + W, hi);   // W <= L (the launcher clamps it), so s + W cannot overflow
    for (int e = s; e < e1; ++e) {
      HQ_DASSERT(s >= 0 && e < L);
      const float key = vs + en[e];
      if (best.s < 0 || key > best.key) best = Best{key, s, e};
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const Best other{__shfl_xor(best.key, o, 64), __shfl_xor(best.s, o, 64), __shfl_xor(best.e, o, 64)};
    if (beats(other, best)) best = other;
  }
  if (lane != 0) return;
  const float* c = in.cls + (long long)b * in.cls_row;
  float cmax = c[0];
  int label = 0;
  for (int k = 1; k < NL; ++k) {
    const float v = c[(long long)k * in.cls_elem];
    if (v > cmax) { cmax = v; label = k; }
  }
  const float cls0 = st[0] + en[0];
  float* o = out + (size_t)b * 6;
  o[0] = best.s < 0 ? -INFINITY : best.key - cls0;
  o[1] = (float)best.s;
  o[2] = (float)best.e;
  o[3] = in.start_reg[(long long)b * in.start_reg_elem];
  o[4] = in.end_reg[(long long)b * in.end_reg_elem];
  o[5] = (float)label;
}

}  // namespace

bool hq_qa_decode_interleaved(const HqDecodeIn& in) {
  return in.end == in.start + 1 && in.start_elem == 2 && in.end_elem == 2 && in.start_row == in.end_row &&
         in.start_row % 2 == 0 && reinterpret_cast<uintptr_t>(in.start) % 8 == 0;
}

void hq_qa_decode(const HqDecodeIn& in, float* out, int B, int L, int NL, int W, hipStream_t s) {
  if (B <= 0) return;
  W = std::min(W, L);   // W >= L is "unbounded"
  const dim3 grid((B + kRows - 1) / kRows), block(256);
  if (hq_qa_decode_interleaved(in))
    hipLaunchKernelGGL(qa_decode_kernel<true>, grid, block, 0, s, in, out, B, L, NL, W);
  else
    hipLaunchKernelGGL(qa_decode_kernel<false>, grid, block, 0, s, in, out, B, L, NL, W);
}
