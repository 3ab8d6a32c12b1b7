// Flash attention backward (hq_attn.h: layout, MFMA orientation, the K/V ring): dQ first — it also produces δ —
// then dK/dV, which reads δ.
// * dQ: 4-wave workgroups of 32 queries each; K and V tiles stream through the LDS-DMA ring; Q·c, dO
//   and the dropout words of the wave's rows are loaded before the ring starts; bias and −LSE ride in the
//   5th MFMA (A' = [K | b_hi, b_lo, 1, 1, 1], B' = [Q·c | 1, 1, −l_hi, −l_mid, −l_lo]: LSE to ~24 bits).
// * dK/dV: ONE pass (S, dP, dV, dK per tile: 17 MFMAs instead of the two-pass 20) in 4-wave workgroups
//   of 32 keys each; Q·c, dO, LSE and δ of each 32-query tile are register-staged into a 2-slot LDS
//   ring (issue the loads before the tile's MFMAs, write after: T14) — Q must be prescaled on its way
//   into LDS to reproduce the forward's rounded Q·c, which an LDS-DMA cannot do; it gathers its key's dropout
//   bits from the forward's words with one 8-byte LDS read per row group.
#include "hq_attn.h"

namespace {

// MODE 0: bf16 dQKV; 1: bf16 + e5m2 copy (fp8 backward, calibrating); 2: e5m2 only + column partials of the
// QKV bias gradient into bpart [B·n32][3H] (fp8 backward, calibrated: every consumer reads the e5m2 copy)
template <bool DROP, int NT, int RAHEAD, int MODE = 0>
__global__ __launch_bounds__(RW * 64, MODE == 0 && NT > 0 ? 4 : 3) void attn_bwd_dq_ring_kernel(
    const uint16_t* __restrict__ qkv, const uint16_t* __restrict__ dctx, const uint16_t* __restrict__ ctx,
    const float* __restrict__ lse, const float* __restrict__ key_bias, const uint16_t* __restrict__ mbits,
    float* __restrict__ delta, uint16_t* __restrict__ dqkv, int L, int nh, int n_qb, float c_scale, float scale,
    float kscale, uint8_t* __restrict__ dqkv8, const float* __restrict__ q8, float* __restrict__ part8, int phase,
    float* __restrict__ bpart) {
  constexpr bool Q8 = MODE > 0;
  if constexpr (Q8) hq_fp8_publish_scale(q8, phase, kHqBf8Max);   // dQKV's state (dK/dV share it)
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  using Lds = RingLds<RAHEAD, uint32_t>;
  const int Lp = NT > 0 ? NT * 32 : (L + 31) & ~31, n32 = Lp >> 5;
  char* ring = reinterpret_cast<char*>(smem);
  uint32_t* sA = reinterpret_cast<uint32_t*>(ring + Lds::sA);       // [Lp] A' word 0 (b_hi,b_lo); 1-3 constant
  uint16_t* sM = reinterpret_cast<uint16_t*>(sA + Lp);              // = ring + Lds::sM(Lp): [RW][n32][64] dropout words
  const int nblk = gridDim.x, lin = hq_xcd_tile(blockIdx.x, nblk);
  const int bh = lin / n_qb, qb = lin - bh * n_qb;
  const int b = bh / nh, h = bh - b * nh;
  const int H = nh * D, ld = 3 * H;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, hh = lane >> 5;
  const int qs = qb * RW + wave;
  const int qi = qs * 32 + (lane & 31);
  const bool active = qs * 32 < L;
  const bool qok = qi < L;
  const uint16_t* base = qkv + (size_t)b * L * ld + h * D;
  HQ_DASSERT(L > 0 && L <= 512 && (NT == 0 || L == NT * 32));

  // ---- prologue (plain loads, issued before any LDS-DMA): Q·c, dO, δ = rowsum(dO·O), −LSE words, bits
  const int qr = qok ? qi : L - 1;
  const size_t orow = ((size_t)b * L + qr) * H + h * D;
  bf16x8_t qf[4], of[4];
  float dpart = 0.f;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    qf[s] = prescale8(*reinterpret_cast<const bf16x8_t*>(base + (size_t)qr * ld + 16 * s + 8 * hh), c_scale);
    of[s] = *reinterpret_cast<const bf16x8_t*>(dctx + orow + 16 * s + 8 * hh);
    float x[8], y[8];
    hq_unpack8(__builtin_bit_cast(uint4, of[s]), x);
    hq_unpack8(*reinterpret_cast<const uint4*>(ctx + orow + 16 * s + 8 * hh), y);
#pragma unroll
    for (int j = 0; j < 8; ++j) dpart += x[j] * y[j];
  }
  const float dlt = xor32_sum(dpart);  // δ over all 64 dims (lanes q and q+32 hold 32 each)
  if (active && qok && hh == 0) delta[(size_t)bh * L + qi] = dlt;
  const float lq = lse[(size_t)bh * L + qr] * LOG2E;
  uint16_t lh, lm, ll;
  split3(-lq, lh, lm, ll);
  const u32x4 qaw = hh ? u32x4{0u, 0u, 0u, 0u}
                       : u32x4{0x3F803F80u, (uint32_t)lh | ((uint32_t)lm << 16), (uint32_t)ll, 0u};
  const bf16x8_t qa = __builtin_bit_cast(bf16x8_t, qaw);
  if constexpr (DROP) {
    constexpr int kMaxT = 16;
    uint16_t mw[kMaxT];
    const uint16_t* gbits = mbits + (((size_t)bh * n32 + qs) * n32) * 64 + lane;
#pragma unroll
    for (int t = 0; t < kMaxT; ++t)
      if (active && t < n32) mw[t] = gbits[(size_t)t * 64];
#pragma unroll
    for (int t = 0; t < kMaxT; ++t)
      if (active && t < n32) sM[(wave * n32 + t) * 64 + lane] = mw[t];
  }
  for (int t = threadIdx.x; t < Lp; t += RW * 64) {  // finite −1e30 past L: see bias_word
    const float bl = t < L ? key_bias[(size_t)b * L + t] * LOG2E : -1e30f;
    sA[t] = bias_word(bl, t < L);
  }
  const int kv_off = dma_lane_off(wave * 8, ld, lane) + wave * 8 * ld;
  auto stage = [&](int kt) { kv_stage<Lds, (NT > 0)>(ring, base, H, ld, L, kv_off, wave, lane, kt); };
#pragma unroll
  for (int t = 0; t < RAHEAD; ++t)
    if (t < n32) stage(t);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  auto wait_tile = [&](int kt) { kv_wait<RAHEAD>(kt, n32, 0); };   // nothing of the loop's own is younger
  constexpr int UNR = NT > 0 ? NT : 1;
  if (!active) {
#pragma unroll UNR
    for (int kt = 0; kt < n32; ++kt) {
      wait_tile(kt);
      __builtin_amdgcn_s_barrier();
      if (kt + RAHEAD < n32) stage(kt + RAHEAD);
    }
    if (Q8 && lane == 0) part8[blockIdx.x * RW + wave] = 0.f;   // its (empty) amax partial
    return;
  }
  LdsOffsets lo_;
  lo_.init(lane);
  const uint32_t* aug_src = sA + (lane & 31);
  const uint16_t* my_bits = sM + wave * n32 * 64 + lane;
  const f32x16_t zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  f32x16_t dq[2] = {zero16, zero16};
  const f2_t dl2 = {dlt, dlt};
#pragma unroll UNR
  for (int kt = 0; kt < n32; ++kt) {
    wait_tile(kt);
    __builtin_amdgcn_s_barrier();
    if (kt + RAHEAD < n32) stage(kt + RAHEAD);
    const char* sK = ring + (kt % Lds::RNS) * Lds::SLOT;
    const uint16_t* tK = reinterpret_cast<const uint16_t*>(sK);
    const uint16_t* tV = reinterpret_cast<const uint16_t*>(sK + RTILE);
    const bf16x8_t ka = __builtin_bit_cast(bf16x8_t, u32x4{aug_src[kt * 32], 0x3F803F80u, 0x3F80u, 0u});
    // without dropout the MFMA groups run at s_setprio 1 (backward −9 % at p = 0, profiles/r6_attn_prio_not_adopted;
    // with dropout it gains nothing, and dK/dV and the forward lose with it)
    if constexpr (!DROP) __builtin_amdgcn_s_setprio(1);
    f32x16_t s_acc = mfma32(row8(tK, 0, lo_, 0), qf[0], zero16);
#pragma unroll
    for (int s = 1; s < 4; ++s) s_acc = mfma32(row8(tK, 0, lo_, s), qf[s], s_acc);
    s_acc = mfma32(ka, qa, s_acc);                      // S' = c·q·k + bias − lse (log2 domain)
    f32x16_t p_acc = mfma32(row8(tV, 0, lo_, 0), of[0], zero16);
#pragma unroll
    for (int s = 1; s < 4; ++s) p_acc = mfma32(row8(tV, 0, lo_, s), of[s], p_acc);
    if constexpr (!DROP) __builtin_amdgcn_s_setprio(0);
    uint32_t bits = 0xFFFFu;
    f2_t ksc = {1.f, 1.f};
    if constexpr (DROP) {
      bits = (uint32_t)my_bits[kt * 64];
      ksc = f2_t{kscale, kscale};
    }
    float ds[16];
#pragma unroll
    for (int r = 0; r < 16; r += 2) {  // dS = P·(dP·mask·ksc − δ): mask as an all-ones/zero AND (v_bfe_i32)
      const f2_t P = {__builtin_amdgcn_exp2f(s_acc[r]), __builtin_amdgcn_exp2f(s_acc[r + 1])};
      f2_t dp = {p_acc[r], p_acc[r + 1]};
      if constexpr (DROP) dp = f2_t{keep_and(dp.x, bits, kbit(r)), keep_and(dp.y, bits, kbit(r + 1))};
      const f2_t v = (dp * ksc - dl2) * P;
      ds[r] = v.x; ds[r + 1] = v.y;
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const bf16x8_t sb = pack_b(ds, s);
      if constexpr (!DROP) __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int d = 0; d < 2; ++d) dq[d] = mfma32(tr8(tK, 0, lo_, s, d), sb, dq[d]);
      if constexpr (!DROP) __builtin_amdgcn_s_setprio(0);
    }
  }
  const size_t orow_q = ((size_t)b * L + qi) * ld + h * D;
  if constexpr (Q8) {   // --precision fp8: dQ also as e5m2 for the QKV dgrad (delayed scaling)
    const float inv8 = 1.f / hq_fp8_delayed_scale(q8, phase, kHqBf8Max);
    float amax = qok ? store_row64_e5<MODE == 1>(dqkv + orow_q, dqkv8 + orow_q, dq, scale, inv8, hh) : 0.f;
    amax = hq_wave_max(amax);
    if (lane == 0) part8[blockIdx.x * RW + wave] = amax;
    if constexpr (MODE == 2)
      colsum_row64(bpart + ((size_t)b * n32 + qs) * 3 * H + h * D, dq, scale, qok, lane, hh);
    return;
  }
  // (dQ keeps the quarter-line store_row64: the staged whole-line form pushed this 128-VGPR loop into 43 spills)
  if (qok) store_row64(dqkv + orow_q, dq, scale, hh);
}

// dK/dV: keys on the lanes.  Per 32-query tile: S = Q'·Kᵀ (+ aug: −LSE, bias), dP = dO·Vᵀ, then
// dVᵀ += dOᵀ·(P∘mask) and dKᵀ += Q'ᵀ·dS with P/dS fed from the accumulators (no LDS round trip).
template <bool DROP, int NT, int MODE = 0>   // MODE: as attn_bwd_dq_ring_kernel
__global__ __launch_bounds__(RW * 64, 2) void attn_bwd_dkdv_ring_kernel(
    const uint16_t* __restrict__ qkv, const uint16_t* __restrict__ dctx, const float* __restrict__ lse,
    const float* __restrict__ delta, const float* __restrict__ key_bias, const uint16_t* __restrict__ mbits,
    uint16_t* __restrict__ dqkv, int L, int nh, int n_kb, float c_scale, float scale, float kscale,
    uint8_t* __restrict__ dqkv8, const float* __restrict__ q8, float* __restrict__ part8, int phase,
    float* __restrict__ bpart) {
  constexpr bool Q8 = MODE > 0;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  using Lds = DkvLds;
  const int Lp = NT > 0 ? NT * 32 : (L + 31) & ~31, n32 = Lp >> 5;
  const int nblk = gridDim.x, lin = hq_xcd_tile(blockIdx.x, nblk);
  const int bh = lin / n_kb, kbk = lin - bh * n_kb;
  const int b = bh / nh, h = bh - b * nh;
  const int H = nh * D, ld = 3 * H;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, hh = lane >> 5;
  const int tid = threadIdx.x;
  const int ks_idx = kbk * RW + wave;                  // this wave's 32-key subtile
  const int kj = ks_idx * 32 + (lane & 31);
  const bool active = ks_idx * 32 < L;
  const bool kok = kj < L;
  const uint16_t* base = qkv + (size_t)b * L * ld + h * D;
  HQ_DASSERT(L > 0 && L <= 512 && (NT == 0 || L == NT * 32));

  // per-wave key fragments (B operands of S and dP) and the B' words (1,1,1,b_hi | b_lo,0,…)
  const int kr = kok ? kj : L - 1;
  bf16x8_t kf[4], vf[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    kf[s] = *reinterpret_cast<const bf16x8_t*>(base + (size_t)kr * ld + H + 16 * s + 8 * hh);
    vf[s] = *reinterpret_cast<const bf16x8_t*>(base + (size_t)kr * ld + 2 * H + 16 * s + 8 * hh);
  }
  bf16x8_t kaug;
  {
    const float bl = kok ? key_bias[(size_t)b * L + kj] * LOG2E : -1e30f;
    const uint32_t bw = bias_word(bl, kok);
    const uint32_t bhi = bw & 0xFFFFu, blo = bw >> 16;
    const u32x4 w = hh ? u32x4{0u, 0u, 0u, 0u}
                       : u32x4{0x3F803F80u, 0x3F80u | (bhi << 16), blo, 0u};
    kaug = __builtin_bit_cast(bf16x8_t, w);
  }
  // register staging of query tile t: thread tid → row tid>>3, 16-B chunk tid&7 of Q and dO; threads
  // 0..31 the A' words (−l_hi,−l_mid | −l_lo,1 | 1,0 | 0) of query tid, 32..63 δ; each wave its bit words.
  // Three tiles in flight in registers (HBM latency under load ≈ 2-3 tile bodies); two LDS slots.
  const int srow = tid >> 3, schunk = tid & 7;
  struct Stage {
    uint4 q, o;
    float l;
    uint16_t bits;
  };
  auto issue = [&](int t, Stage& st) {
    const int q = min(t * 32 + srow, L - 1);
    st.q = *reinterpret_cast<const uint4*>(base + (size_t)q * ld + schunk * 8);
    st.o = *reinterpret_cast<const uint4*>(dctx + ((size_t)b * L + q) * H + h * D + schunk * 8);
    // every thread issues every load (wave 0's lse/δ values are the ones committed; the other waves load
    // them redundantly): exec-masked loads would make hipcc's vmcnt counting assume they were skipped and
    // wait for a tile too many
    {
      const int qq2 = min(t * 32 + (lane & 31), L - 1);
      st.l = (lane < 32 ? lse : delta)[(size_t)bh * L + qq2];
      if (t * 32 + (lane & 31) >= L) st.l = lane < 32 ? 1e30f : 0.f;  // queries past L: P = 0 (finite: split3)
    }
    st.bits = 0;
    if constexpr (DROP) st.bits = mbits[(((size_t)bh * n32 + t) * n32 + min(ks_idx, n32 - 1)) * 64 + lane];
  };
  auto commit = [&](int t, const Stage& st) {
    char* slot = reinterpret_cast<char*>(smem) + Lds::slot(t);
    uint16_t* sq = reinterpret_cast<uint16_t*>(slot + Lds::Q);
    uint16_t* so = reinterpret_cast<uint16_t*>(slot + Lds::DO);
    float f[8];
    hq_unpack8(st.q, f);
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] *= c_scale;       // Q·c rounded exactly as the forward's prescale8
    *reinterpret_cast<uint4*>(sq + lds_off(srow, schunk * 8)) = hq_pack8(f);
    *reinterpret_cast<uint4*>(so + lds_off(srow, schunk * 8)) = st.o;
    if (tid < 32) {
      uint16_t lh, lm, ll;
      split3(-st.l * LOG2E, lh, lm, ll);
      reinterpret_cast<uint4*>(slot + Lds::AW)[tid] =
          make_uint4((uint32_t)lh | ((uint32_t)lm << 16), (uint32_t)ll | (0x3F80u << 16), 0x3F80u, 0u);
    } else if (tid < 64) {
      reinterpret_cast<float*>(slot + Lds::DELTA)[tid - 32] = st.l;
    }
    if constexpr (DROP) reinterpret_cast<uint16_t*>(slot + Lds::BITS)[wave * 64 + lane] = st.bits;
  };
  LdsOffsets lo_;
  lo_.init(lane);
  const f32x16_t zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  f32x16_t dv[2] = {zero16, zero16}, dk[2] = {zero16, zero16};
  const int krel = lane & 31;
  const int hh_f = (krel >> 2) & 1;
  const int r_f = kbit((krel & 3) + 4 * (krel >> 3));   // bit position in the forward's keep word
  const float ksc = DROP ? kscale : 1.f;
  const f2_t ksc2 = {ksc, ksc};
  // S = Q'·Kᵀ (+ bias_k − lse_q through the A'/B' words) and dP = dO·Vᵀ of tile t.  All eight operand reads are
  // issued before the first MFMA (sched_barrier): left to itself hipcc reads each operand just before its
  // MFMA and waits lgkmcnt(0) there, exposing the LDS latency once per MFMA.
  auto scores = [&](int t, f32x16_t& s_acc, f32x16_t& p_acc) {
    const char* slot = reinterpret_cast<const char*>(smem) + Lds::slot(t);
    const uint16_t* tq = reinterpret_cast<const uint16_t*>(slot + Lds::Q);
    const uint16_t* to = reinterpret_cast<const uint16_t*>(slot + Lds::DO);
    bf16x8_t fq[4], fo[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      fq[s] = row8(tq, 0, lo_, s);
      fo[s] = row8(to, 0, lo_, s);
    }
    const uint4 aw = reinterpret_cast<const uint4*>(slot + Lds::AW)[hh ? 0 : krel];
    __builtin_amdgcn_sched_barrier(0);
    const bf16x8_t qa = hh ? bf16x8_t{0, 0, 0, 0, 0, 0, 0, 0} : __builtin_bit_cast(bf16x8_t, u32x4{aw.x, aw.y, aw.z, aw.w});
    s_acc = mfma32(fq[0], kf[0], zero16);
    p_acc = mfma32(fo[0], vf[0], zero16);
#pragma unroll
    for (int s = 1; s < 4; ++s) {
      s_acc = mfma32(fq[s], kf[s], s_acc);
      p_acc = mfma32(fo[s], vf[s], p_acc);
    }
    s_acc = mfma32(qa, kaug, s_acc);                   // + bias_k − lse_q
  };
  // P, dS of tile t from its accumulators, then dVᵀ += dOᵀ·(P∘mask), dKᵀ += Q'ᵀ·dS
  auto grads = [&](int t, const f32x16_t& s_acc, const f32x16_t& p_acc) {
    const char* slot = reinterpret_cast<const char*>(smem) + Lds::slot(t);
    const uint16_t* tq = reinterpret_cast<const uint16_t*>(slot + Lds::Q);
    const uint16_t* to = reinterpret_cast<const uint16_t*>(slot + Lds::DO);
    // mask: the forward word of fwd-lane l' = q + 32·hh' holds bit r' for key acc_row(r', hh'); this lane
    // (key krel) needs, for query rows acc_row(r, hh) = 8g + 4hh + i, bit r_f of the words of fwd-lanes
    // 8g + 4hh + i + 32·hh_f: four consecutive words per g, one 8-byte LDS read per g
    const uint16_t* wsrc = reinterpret_cast<const uint16_t*>(slot + Lds::BITS) + wave * 64 + 4 * hh + 32 * hh_f;
    const float* sdl = reinterpret_cast<const float*>(slot + Lds::DELTA);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      // this half's dV / dK operands read ahead of the exp / mask VALU that produces the other operand
      bf16x8_t ov[2], oq[2];
#pragma unroll
      for (int d = 0; d < 2; ++d) {
        ov[d] = tr8(to, 0, lo_, s, d);
        oq[d] = tr8(tq, 0, lo_, s, d);
      }
      __builtin_amdgcn_sched_barrier(0);
      float pd[8], dsv[8];
#pragma unroll
      for (int gg = 0; gg < 2; ++gg) {
        const int g = 2 * s + gg;
        const float4 d4 = *reinterpret_cast<const float4*>(sdl + 8 * g + 4 * hh);
        const f2_t dl[2] = {f2_t{d4.x, d4.y}, f2_t{d4.z, d4.w}};
        float P[4], dp[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          P[i] = __builtin_amdgcn_exp2f(s_acc[4 * g + i]);
          dp[i] = p_acc[4 * g + i];
        }
        // keep bits as AND masks: pd = P·mask (kscale is applied once, at the dV store), dS = P·(dP·mask·ksc − δ)
        float pm[4] = {P[0], P[1], P[2], P[3]};
        if constexpr (DROP) {
          const uint64_t w = *reinterpret_cast<const uint64_t*>(wsrc + 8 * g);
          const uint32_t wl = (uint32_t)w, wh = (uint32_t)(w >> 32);
          const int pos[4] = {r_f, r_f + 16, r_f, r_f + 16};
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            pm[i] = keep_and(P[i], i < 2 ? wl : wh, pos[i]);
            dp[i] = keep_and(dp[i], i < 2 ? wl : wh, pos[i]);
          }
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const f2_t Pj = {P[2 * j], P[2 * j + 1]}, dpj = {dp[2 * j], dp[2 * j + 1]};
          const f2_t v = (dpj * ksc2 - dl[j]) * Pj;
          pd[4 * gg + 2 * j] = pm[2 * j];
          pd[4 * gg + 2 * j + 1] = pm[2 * j + 1];
          dsv[4 * gg + 2 * j] = v.x;
          dsv[4 * gg + 2 * j + 1] = v.y;
        }
      }
      const bf16x8_t pb = pack_b(pd, 0), sb = pack_b(dsv, 0);
#pragma unroll
      for (int d = 0; d < 2; ++d) {
        dv[d] = mfma32(ov[d], pb, dv[d]);
        dk[d] = mfma32(oq[d], sb, dk[d]);
      }
    }
  };
  // Tile t lives in register set st[t % 3] (compile-time index in the unrolled NT > 0 loop: a rotation by
  // copies would make hipcc wait for the NEWER tile's loads before each copy); the rolled NT = 0 loop
  // rotates by copies (one tile less lookahead).
  Stage st[3];
  issue(0, st[0]);
  if (n32 > 1) issue(1, st[1]);
  if (n32 > 2) issue(2, st[2]);
  constexpr int UNR = NT > 0 ? NT : 1;
  {
    commit(0, st[0]);
    __syncthreads();
    if constexpr (NT > 0) {
      if (n32 > 3) issue(3, st[0]);
    } else {
      st[0] = st[1];
      st[1] = st[2];
      if (n32 > 3) issue(3, st[2]);
    }
#pragma unroll UNR
    for (int t = 0; t < n32; ++t) {
      if constexpr (NT > 0) {
        // tile t+1 into the other slot BEFORE this tile's work, so its LDS writes overlap the MFMA chains: that
        // slot's last reader (tile t-1) finished before the previous barrier
        if (t + 1 < n32) {
          commit(t + 1, st[(t + 1) % 3]);
          if (t + 4 < n32) issue(t + 4, st[(t + 1) % 3]);
        }
      }
      if (active) {
        f32x16_t s_acc, p_acc;
        scores(t, s_acc, p_acc);
        grads(t, s_acc, p_acc);
      }
      if (t + 1 < n32) {                                  // the other slot: last read before this barrier
        if constexpr (NT > 0) {
          __syncthreads();
        } else {
          commit(t + 1, st[0]);
          __syncthreads();
          st[0] = st[1];
          st[1] = st[2];
          if (t + 4 < n32) issue(t + 4, st[2]);
        }
      }
    }
  }
  if constexpr (Q8) {   // dK, dV also as e5m2; partial slots after the dQ kernel's
    const size_t orow_k = ((size_t)b * L + kj) * ld + h * D;
    const float inv8 = 1.f / hq_fp8_delayed_scale(q8, phase, kHqBf8Max);
    float amax = 0.f;
    if (active && kok) {
      amax = store_row64_e5<MODE == 1>(dqkv + orow_k + 2 * H, dqkv8 + orow_k + 2 * H, dv, ksc, inv8, hh);
      amax = fmaxf(amax, store_row64_e5<MODE == 1>(dqkv + orow_k + H, dqkv8 + orow_k + H, dk, LN2, inv8, hh));
    }
    amax = hq_wave_max(amax);
    if (lane == 0) part8[(gridDim.x + blockIdx.x) * RW + wave] = amax;
    if constexpr (MODE == 2) {
      if (active) {   // every key subtile < n32 is active (L ≤ 32·n32): each partial row is written once
        float* row = bpart + ((size_t)b * n32 + ks_idx) * 3 * H + h * D;
        colsum_row64(row + 2 * H, dv, ksc, kok, lane, hh);
        colsum_row64(row + H, dk, LN2, kok, lane, hh);
      }
    }
    return;
  }
  // dV, dK as whole 128-B lines: every wave is past its last slot read after this barrier; one region per wave
  __syncthreads();
  if (active) {
    uint16_t* out = dqkv + ((size_t)b * L + ks_idx * 32) * ld + h * D;
    char* reg = reinterpret_cast<char*>(smem) + wave * LINES_BYTES;
    store_tile64_lines(out + 2 * H, ld, L - ks_idx * 32, dv, ksc, lane, reg);   // pd carried the mask only
    store_tile64_lines(out + H, ld, L - ks_idx * 32, dk, LN2, lane, reg);       // Q' = c·Q, c = scale·log2e
  }
}

}  // namespace

void hq_attn_bwd(const uint16_t* dctx, const uint16_t* qkv, const uint16_t* ctx, const float* lse, const float* key_bias,
                 const uint16_t* mbits, uint16_t* dqkv, float* delta, int B, int L, int nh, int dh, float p,
                 float scale, hipStream_t s, uint8_t* dqkv8, float* q8, int phase, float* bpart) {
  if (dh != D || L > 512) { fprintf(stderr, "hq_attn_bwd: head_dim %d / L %d unsupported\n", dh, L); abort(); }
  const uint32_t thr = p > 0.f ? hq_threshold(p) : 0u;
  const float ks = hq_keep_scale(thr);
  const uint16_t* bits = thr ? mbits : nullptr;
  const int Lp = (L + 31) & ~31, n32 = Lp / 32;
  const int nb = (L + RQ - 1) / RQ;                 // 128-row blocks (queries for dQ, keys for dK/dV)
  // ring depth: 2 tiles ahead on the bf16 path (39.5 KB of LDS per workgroup at L = 384 with dropout, so
  // 4 workgroups — 4 waves per SIMD — share a CU), 3 on the fp8 paths (their e5m2 epilogues need > 128 VGPRs)
  constexpr int AH = 2, AH8 = 3;
  const size_t lds_dq = dqkv8 ? RingLds<AH8, uint32_t>::bytes(Lp, n32, bits != nullptr)
                              : RingLds<AH, uint32_t>::bytes(Lp, n32, bits != nullptr);
  const size_t lds_kv = DkvLds::bytes();
  // dQ and dK/dV grids are the same size: partials [dQ waves | dK/dV waves], one fold after both
  const int nparts = B * nh * nb * RW;
  float* part8 = dqkv8 ? hq_fp8_amax_parts((size_t)2 * nparts, q8, s) : nullptr;
  dispatch_nt(L, [&](auto cn) {
    constexpr int NT = decltype(cn)::value;
    auto launch = [&](auto kdq, auto kkv) {
      [[maybe_unused]] static const bool once = hq_raise_lds_limit({(const void*)kdq}, 64 * 1024);
      hipLaunchKernelGGL(kdq, dim3(B * nh * nb), dim3(RW * 64), lds_dq, s, qkv, dctx, ctx, lse, key_bias, bits, delta,
                         dqkv, L, nh, nb, scale * LOG2E, scale, ks, dqkv8, q8, part8, phase, bpart);
      hipLaunchKernelGGL(kkv, dim3(B * nh * nb), dim3(RW * 64), lds_kv, s, qkv, dctx, lse, delta, key_bias, bits, dqkv,
                         L, nh, nb, scale * LOG2E, scale, ks, dqkv8, q8, part8, phase, bpart);
    };
    if (dqkv8 && bpart) {   // --precision fp8, calibrated: e5m2 + bias partials, no bf16
      if (bits) launch(attn_bwd_dq_ring_kernel<true, NT, AH8, 2>, attn_bwd_dkdv_ring_kernel<true, NT, 2>);
      else launch(attn_bwd_dq_ring_kernel<false, NT, AH8, 2>, attn_bwd_dkdv_ring_kernel<false, NT, 2>);
    } else if (dqkv8) {   // --precision fp8: the e5m2-writing variants
      if (bits) launch(attn_bwd_dq_ring_kernel<true, NT, AH8, 1>, attn_bwd_dkdv_ring_kernel<true, NT, 1>);
      else launch(attn_bwd_dq_ring_kernel<false, NT, AH8, 1>, attn_bwd_dkdv_ring_kernel<false, NT, 1>);
    } else {
      if (bits) launch(attn_bwd_dq_ring_kernel<true, NT, AH>, attn_bwd_dkdv_ring_kernel<true, NT>);
      else launch(attn_bwd_dq_ring_kernel<false, NT, AH>, attn_bwd_dkdv_ring_kernel<false, NT>);
    }
  });
  if (dqkv8) hq_fp8_amax_fold(part8, 2 * nparts, q8, phase, s, kHqBf8Max);
}
