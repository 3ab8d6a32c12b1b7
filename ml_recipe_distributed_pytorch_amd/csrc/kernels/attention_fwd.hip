// Flash attention forward (hq_attn.h: layout, MFMA orientation, the K/V ring).
// * a workgroup is 4 waves × 32 queries of one head; three workgroups per CU;
// * the key-mask bias and the running row max ride in a 5th MFMA per tile: K' = [K | b_hi, b_lo, 1, 0…]
//   and Q' = [Q·c | 1, 1, −m, 0…] (bf16; b_hi + b_lo = bias·log2e to ~16 bits, m kept bf16-exact), so
//   S' = c·QKᵀ + bias − m leaves the MFMA ready for exp2 — no accumulator init, no subtraction in VALU;
// * no per-tile max and no rescale: m is the first tile's row max (a lower bound of the row max, so
//   P ≤ 2^(rowmax − m) and l ≥ 1); bf16/fp32 relative precision does not depend on magnitude, and a
//   workgroup with a row whose l exceeds 2^64 recomputes its rows on an in-kernel slow path (per-tile max
//   + rescale, per-wave LDS staging) after the fast loop.  LSE = m + log2 l.
#include "hq_attn.h"

namespace {

template <bool DROP, bool EVEN, int NT, int RAHEAD>
__global__ __launch_bounds__(RW * 64, 4) void attn_fwd_ring_kernel(const uint16_t* __restrict__ qkv,
                                                                   const float* __restrict__ key_bias,
                                                                   uint16_t* __restrict__ ctx, float* __restrict__ lse,
                                                                   uint16_t* __restrict__ mbits, int L, int nh,
                                                                   int n_qb, float c_scale, HqDropKey kd_,
                                                                   uint32_t thr, float kscale, int force_slow,
                                                                   uint8_t* __restrict__ ctx8,
                                                                   const float* __restrict__ q8,
                                                                   float* __restrict__ part8, int phase) {
  const uint32_t key = kd_.get();
  if (ctx8 != nullptr) hq_fp8_publish_scale(q8, phase);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int Lp = NT > 0 ? NT * 32 : (L + 31) & ~31, n32 = Lp >> 5;
  using Lds = RingLds<RAHEAD, uint2>;
  static_assert(RAHEAD >= 2 && RAHEAD <= 4, "ring depth (>= RW slots: per-wave slow-path / store regions)");
  char* ring = reinterpret_cast<char*>(smem);
  char* sQ = ring + Lds::sQ;
  uint2* sA = reinterpret_cast<uint2*>(ring + Lds::sA);             // [Lp]: (pk(b_hi, b_lo), pk(1, 0))
  // XCD-aware block order (bijective): blocks b, b+8, … share an XCD; give each XCD a contiguous run of
  // (head, query-block) pairs with the query block fastest, so a head's blocks are co-resident on one L2
  const int nblk = gridDim.x, lin = hq_xcd_tile(blockIdx.x, nblk);
  const int bh = lin / n_qb, qb = lin - bh * n_qb;
  const int b = bh / nh, h = bh - b * nh;
  const int H = nh * D, ld = 3 * H;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, hh = lane >> 5;
  const int qs = qb * RW + wave;                       // this wave's 32-query subtile (of the head)
  const int qi = qs * 32 + (lane & 31);
  const bool active = qs * 32 < L;                     // waves past L (last block) only help with DMA
  const uint16_t* base = qkv + (size_t)b * L * ld + h * D;
  HQ_DASSERT(L > 0 && L <= 512 && (NT == 0 || L == NT * 32) && bh < nblk / n_qb);

  // ---- prologue: Q block (this wave's 8 row-pieces... 32 rows = 4 pieces) + the first RAHEAD tiles
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int r0 = wave * 32 + p * 8;                  // row within the workgroup's 128 queries
    const int rows = L - qb * RQ;                      // valid query rows of this block
    dma_rows8(base + (size_t)qb * RQ * ld, ld, r0, rows > 0 ? rows : 1, sQ, lane);
  }
  const int kv_off = dma_lane_off(wave * 8, ld, lane) + wave * 8 * ld;
  auto stage = [&](int kt) { kv_stage<Lds, EVEN>(ring, base, H, ld, L, kv_off, wave, lane, kt); };
#pragma unroll
  for (int t = 0; t < RAHEAD; ++t)
    if (t < n32) stage(t);
  // keys past L: finite −1e30 (bias_word); the hh = 1 lanes read these same words as k-dims 8..15, which meet zeros in Q'
  for (int t = threadIdx.x; t < Lp; t += RW * 64) {
    const float bl = t < L ? key_bias[(size_t)b * L + t] * LOG2E : -1e30f;
    sA[t] = make_uint2(bias_word(bl, t < L), 0x3F80u);  // (b_hi, b_lo, 1.0, 0)
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  LdsOffsets lo_;
  lo_.init(lane);
  bf16x8_t qf[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const bf16x8_t raw = *reinterpret_cast<const bf16x8_t*>(sQ + 2 * (wave * 32 * D + lo_.row[s]));
    qf[s] = prescale8(raw, c_scale);
  }
  const uint2* aug_src = sA + (lane & 31);
  float m_b = 0.f;                                        // bf16-exact running max (log2 domain)
  const uint32_t qaug_w0 = hh ? 0u : 0x3F803F80u;         // (1, 1) against (b_hi, b_lo)
  uint32_t qaug_w = 0u;                                   // (−m, 0) against (1, 0); −0 until the first tile
  f32x16_t o[2];
#pragma unroll
  for (int d = 0; d < 2; ++d)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[d][r] = 0.f;
  f2_t l2 = {0.f, 0.f};
  const uint32_t row_idx = ((uint32_t)bh * L + (uint32_t)min(qi, L - 1)) * (uint32_t)L;
  uint16_t* my_bits = mbits + (((size_t)bh * n32 + qs) * n32) * 64 + lane;
  const f32x16_t zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

  // the memory operations of this wave younger than tile kt's stage, beside the later stages: with dropout, the
  // RAHEAD bit stores of iterations kt − RAHEAD … kt − 1 (each iteration stages, then stores its bits)
  auto wait_tile = [&](int kt, bool with_stores) { kv_wait<RAHEAD>(kt, n32, with_stores ? RAHEAD : 0); };
  constexpr int UNR = NT > 0 ? NT : 1;
  if (!active) {  // waves past L (last query block): their share of the DMA and every barrier, nothing else
#pragma unroll UNR
    for (int kt = 0; kt < n32; ++kt) {
      wait_tile(kt, false);
      __builtin_amdgcn_s_barrier();
      if (kt + RAHEAD < n32) stage(kt + RAHEAD);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    (void)__syncthreads_or(0);                         // the workgroup's slow-path vote (below)
    if (ctx8 != nullptr && lane == 0) part8[blockIdx.x * RW + wave] = 0.f;   // its (empty) amax partial
    return;
  }
  // Branch-free tile loop: a per-tile rescale branch makes hipcc copy the 32 O registers across the join
  // (43 v_mov_b64 per tile measured).  m stays the first tile's row max, so every P ≤ 2^(rowmax − m); a
  // workgroup with a row whose l outgrew 2^64 redoes its rows on the slow path after the loop (never
  // triggered by BERT activations; a left-padded row with a fully masked first tile is the realistic case).
#pragma unroll UNR
  for (int kt = 0; kt < n32; ++kt) {
    wait_tile(kt, DROP);
    __builtin_amdgcn_s_barrier();
    if (kt + RAHEAD < n32) stage(kt + RAHEAD);         // its slot was last read two barriers ago
    const char* sK = ring + (kt % Lds::RNS) * Lds::SLOT;
    const uint16_t* tK = reinterpret_cast<const uint16_t*>(sK);
    const uint16_t* tV = reinterpret_cast<const uint16_t*>(sK + RTILE);
    bf16x8_t kf[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) kf[s] = row8(tK, 0, lo_, s);
    const uint2 aw = aug_src[kt * 32];
    const bf16x8_t ka = __builtin_bit_cast(bf16x8_t, u32x4{aw.x, aw.y, 0u, 0u});
    const bf16x8_t qa = __builtin_bit_cast(bf16x8_t, u32x4{qaug_w0, qaug_w, 0u, 0u});
    f32x16_t acc = mfma32(kf[0], qf[0], zero16);
#pragma unroll
    for (int s = 1; s < 4; ++s) acc = mfma32(kf[s], qf[s], acc);
    acc = mfma32(ka, qa, acc);                          // + bias_k − m_q
    float sc[16];
    if (kt == 0) {                                      // first tile: the row max over the full tile
      const float mx = xor32_max(max16(acc));
      m_b = hq_bf2f(bf16_rne(mx == -INFINITY ? 0.f : mx));
      qaug_w = hh ? 0u : (uint32_t)bf16_rne(-m_b);
#pragma unroll
      for (int r = 0; r < 16; ++r) sc[r] = __builtin_amdgcn_exp2f(acc[r] - m_b);
    } else {
#pragma unroll
      for (int r = 0; r < 16; ++r) sc[r] = __builtin_amdgcn_exp2f(acc[r]);
    }
    {  // the softmax denominator counts every key (dropout only thins P·V); pairwise tree, not a chain
      const f2_t a0 = f2_t{sc[0], sc[1]} + f2_t{sc[2], sc[3]}, a1 = f2_t{sc[4], sc[5]} + f2_t{sc[6], sc[7]};
      const f2_t a2 = f2_t{sc[8], sc[9]} + f2_t{sc[10], sc[11]}, a3 = f2_t{sc[12], sc[13]} + f2_t{sc[14], sc[15]};
      l2 += (a0 + a1) + (a2 + a3);
    }
    // dropout on the PACKED bf16 P: element pair p = (2p, 2p + 1) is one bf16x2 word of pack_b and one
    // 32-bit hash (low half → element 2p).  Packed u16 saturating ops turn the hash halves into keep flags
    // (z = sat(thr − h) is 0 iff kept; sat(1 − z) is the flag) and the flags into a per-half AND mask —
    // 5 VALU per pair instead of two compares, two f32 selects and a bit insert per element.
    uint32_t km[8];
    if constexpr (DROP) {
      uint32_t kb = 0;   // keep flags: element 2p at bit p, element 2p + 1 at bit 16 + p
      if constexpr (EVEN) {
        uint32_t pk = (((row_idx >> 1) + (uint32_t)kt * 16u) ^ key) ^ (2u * (uint32_t)hh);
        pk ^= pk >> 16;                                   // hq_mix24's first xorshift, once per tile
        const u16x2_t thr2 = {(uint16_t)thr, (uint16_t)thr}, one2 = {1, 1}, zero2 = {0, 0};
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
          for (int ip = 0; ip < 2; ++ip) {
            const uint32_t hsh = hq_mix24_post(pk ^ (uint32_t)(4 * g + ip));   // = hq_mix24(pair ^ key)
            const int p = 2 * g + ip;
            const u16x2_t z = __builtin_elementwise_sub_sat(thr2, __builtin_bit_cast(u16x2_t, hsh));
            const u16x2_t kf = __builtin_elementwise_sub_sat(one2, z);
            km[p] = __builtin_bit_cast(uint32_t, zero2 - kf);
            kb |= __builtin_bit_cast(uint32_t, kf) << p;
          }
      } else {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const uint32_t idx0 = row_idx + kt * 32 + 8 * g + 4 * hh;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int r = 4 * g + i;
            kb |= (uint32_t)hq_keep(idx0 + i, key, thr) << ((r >> 1) + 16 * (r & 1));
          }
        }
#pragma unroll
        for (int p = 0; p < 8; ++p)
          km[p] = ((kb >> p) & 1u ? 0xFFFFu : 0u) | ((kb >> (16 + p)) & 1u ? 0xFFFF0000u : 0u);
      }
      // stored word: element r at bit kbit(r) (bytes 0 and 2 of kb)
      my_bits[(size_t)kt * 64] = (uint16_t)((kb & 0xFFu) | ((kb >> 8) & 0xFF00u));
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      bf16x8_t pb = pack_b(sc, s);
      if constexpr (DROP) {
        u32x4 u = __builtin_bit_cast(u32x4, pb);
        u &= u32x4{km[4 * s], km[4 * s + 1], km[4 * s + 2], km[4 * s + 3]};
        pb = __builtin_bit_cast(bf16x8_t, u);
      }
#pragma unroll
      for (int d = 0; d < 2; ++d) o[d] = mfma32(tr8(tV, 0, lo_, s, d), pb, o[d]);
    }
  }
  float l_tot = xor32_sum(l2.x + l2.y);
  // slow-path vote: any row of the workgroup whose l left [1, 2^64) (P could have overflowed) — or every
  // workgroup when force_slow (tests) — recomputes with a per-tile max and rescale.  The ring is idle now
  // (every tile consumed; only bit stores may be in flight), so each wave stages K/V in a private 8 KB of it.
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (__syncthreads_or(force_slow || (qi < L && !(l_tot < 0x1p64f)))) {
    uint16_t* pK = reinterpret_cast<uint16_t*>(ring + wave * Lds::SLOT);
    uint16_t* pV = pK + 32 * D;
#pragma unroll
    for (int d = 0; d < 2; ++d)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[d][r] = 0.f;
    l2 = f2_t{0.f, 0.f};
    float m_run = -INFINITY;
    const uint16_t* kbase = base + H;
    for (int kt = 0; kt < n32; ++kt) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {  // private staging: plain loads, ds_write; LDS is in order per wave
        const int r = i * 8 + (lane >> 3), c = (lane & 7) * 8;
        const int kr = min(kt * 32 + r, L - 1);
        const uint4 kv = *reinterpret_cast<const uint4*>(kbase + (size_t)kr * ld + c);
        const uint4 vv = *reinterpret_cast<const uint4*>(kbase + H + (size_t)kr * ld + c);
        *reinterpret_cast<uint4*>(pK + lds_off(r, c)) = kv;
        *reinterpret_cast<uint4*>(pV + lds_off(r, c)) = vv;
      }
      bf16x8_t kf[4];
#pragma unroll
      for (int s = 0; s < 4; ++s) kf[s] = row8(pK, 0, lo_, s);
      const uint2 aw = aug_src[kt * 32];
      const bf16x8_t ka = __builtin_bit_cast(bf16x8_t, u32x4{aw.x, aw.y, 0u, 0u});
      const bf16x8_t qa = __builtin_bit_cast(bf16x8_t, u32x4{qaug_w0, 0u, 0u, 0u});  // m = 0: exact scores
      f32x16_t acc = mfma32(kf[0], qf[0], zero16);
#pragma unroll
      for (int s = 1; s < 4; ++s) acc = mfma32(kf[s], qf[s], acc);
      acc = mfma32(ka, qa, acc);
      const float m_new = fmaxf(m_run, xor32_max(max16(acc)));
      const float ms = m_new == -INFINITY ? 0.f : m_new;
      const float alpha = __builtin_amdgcn_exp2f(m_run - ms);
      m_run = m_new;
      l2 *= f2_t{alpha, alpha};
#pragma unroll
      for (int d = 0; d < 2; ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[d][r] *= alpha;
      float sc[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        sc[r] = __builtin_amdgcn_exp2f(acc[r] - ms);
        l2.x += sc[r];
      }
      if constexpr (DROP) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const uint32_t idx0 = row_idx + kt * 32 + 8 * g + 4 * hh;
#pragma unroll
          for (int i = 0; i < 4; ++i) sc[4 * g + i] = hq_keep(idx0 + i, key, thr) ? sc[4 * g + i] : 0.f;
        }
      }
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const bf16x8_t pb = pack_b(sc, s);
#pragma unroll
        for (int d = 0; d < 2; ++d) o[d] = mfma32(tr8(pV, 0, lo_, s, d), pb, o[d]);
      }
    }
    m_b = m_run == -INFINITY ? 0.f : m_run;
    l_tot = xor32_sum(l2.x + l2.y);
  }
  const float inv = (DROP ? kscale : 1.f) / l_tot;
  if (ctx8 != nullptr) {   // --precision fp8: ctx also in e4m3 for the out-projection (delayed scaling)
    const float s8 = hq_fp8_delayed_scale(q8, phase);
    float amax = 0.f;
    if (qi < L) {
      const size_t row = ((size_t)b * L + qi) * H + h * D;
      amax = store_row64_q8(ctx + row, ctx8 + row, o, inv, 1.f / s8, hh);
      if (hh == 0) lse[(size_t)bh * L + qi] = (m_b + __builtin_amdgcn_logf(l_tot)) * LN2;
    }
    amax = hq_wave_max(amax);   // -> this wave's partial slot, folded by hq_fp8_amax_fold (no atomics)
    if (lane == 0) part8[blockIdx.x * RW + wave] = amax;
    return;
  }
  // ctx as whole 128-B lines through this wave's slow-path region of the ring (every tile was consumed before
  // the vote's barrier, and no other wave touches this region)
  store_tile64_lines(ctx + ((size_t)b * L + qs * 32) * H + h * D, H, L - qs * 32, o, inv, lane,
                     ring + wave * Lds::SLOT);
  if (qi < L && hh == 0) lse[(size_t)bh * L + qi] = (m_b + __builtin_amdgcn_logf(l_tot)) * LN2;  // v_log_f32 = log2
}

}  // namespace

size_t hq_attn_mask_bytes(int B, int L, int nh) {
  const size_t n32 = (size_t)(L + 31) / 32;
  return (size_t)B * nh * n32 * n32 * 64 * sizeof(uint16_t);
}

// HQ_ATTN_FORCE_SLOW=1 / attn_set_force_slow(1): every workgroup of the ring forward takes its slow path
// (tests only: the rare rescale branch gets its own coverage, kernel playbook rule 26)
static int g_attn_force_slow = [] {
  const char* e = getenv("HQ_ATTN_FORCE_SLOW");
  return e && atoi(e) ? 1 : 0;
}();
void hq_attn_set_force_slow(int v) { g_attn_force_slow = v ? 1 : 0; }

void hq_attn_fwd(const uint16_t* qkv, const float* key_bias, uint16_t* ctx, float* lse, uint16_t* mbits, int B, int L,
                 int nh, int dh, float p, uint32_t seed, uint32_t opid, float scale, hipStream_t s, uint8_t* ctx8,
                 float* q8, int phase) {
  if (dh != D || L > 512) { fprintf(stderr, "hq_attn_fwd: head_dim %d / L %d unsupported\n", dh, L); abort(); }
  const uint32_t thr = p > 0.f ? hq_threshold(p) : 0u;
  const HqDropKey key = hq_drop_key(seed, opid);
  const int Lp = (L + 31) & ~31;
  const int n_qb = (L + RQ - 1) / RQ;
  const int force_slow = g_attn_force_slow;
  constexpr int AH = 2;   // K/V tiles in flight (4-deep measured slower: profiles/r2_attn)
  const size_t lds = RingLds<AH, uint2>::bytes(Lp);
  const int nparts = B * nh * n_qb * RW;
  float* part8 = ctx8 ? hq_fp8_amax_parts((size_t)nparts, q8, s) : nullptr;
  dispatch_nt(L, [&](auto cn) {
    constexpr int NT = decltype(cn)::value;
    auto launch1 = [&](auto kern) {
      [[maybe_unused]] static const bool once = hq_raise_lds_limit({(const void*)kern}, 64 * 1024);
      hipLaunchKernelGGL(kern, dim3(B * nh * n_qb), dim3(RW * 64), lds, s, qkv, key_bias, ctx, lse,
                         thr ? mbits : nullptr, L, nh, n_qb, scale * LOG2E, key, thr, hq_keep_scale(thr), force_slow,
                         ctx8, q8, part8, phase);
    };
    if constexpr (NT > 0) {
      if (!thr) launch1(attn_fwd_ring_kernel<false, true, NT, AH>);
      else launch1(attn_fwd_ring_kernel<true, true, NT, AH>);
    } else {
      if (!thr && (L & 31) == 0) launch1(attn_fwd_ring_kernel<false, true, 0, AH>);
      else if (!thr) launch1(attn_fwd_ring_kernel<false, false, 0, AH>);
      else if ((L & 31) == 0) launch1(attn_fwd_ring_kernel<true, true, 0, AH>);
      else launch1(attn_fwd_ring_kernel<true, false, 0, AH>);
    }
  });
  if (ctx8) hq_fp8_amax_fold(part8, nparts, q8, phase, s);
}
