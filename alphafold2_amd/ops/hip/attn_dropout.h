// Attention-probability dropout: the keep/drop decision of element
// (bh, i, j) as a pure function of (seed, offset) and the position.
//
// Every kernel that needs the mask (forward, dQ, dK/dV, the mask dump)
// calls into this header, so they agree whatever their tiling or
// fragment layout.  Host-callable too: the definition can be checked on
// a CPU against at::Philox4_32.
//
// Definition (docs/PARITY.md):
//  * Philox4x32-10, key = 64-bit seed (low, high word), counter =
//    (offset_lo, offset_hi, subseq_lo, subseq_hi) — what
//    at::Philox4_32(seed, subsequence, offset) produces first.
//  * one 128-bit output covers the 4x4 block of rows 4*(i>>2)..+3 and
//    columns 4*(j>>2)..+3; with H4 = ceil(Lq/4), W4 = ceil(Lk/4):
//      subsequence = (bh*H4 + (i>>2))*W4 + (j>>2)          (64-bit)
//    element (i, j) owns byte (j&3) of output word (i&3).
//  * keep iff byte >= T, T = clamp(round(p*256), 1, 255); the kept
//    probabilities are rescaled by exactly 256/(256 - T).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define AF2_HD __host__ __device__ __forceinline__
#else
#define AF2_HD inline
#endif

namespace attn_drop {

struct U4 {
  uint32_t w[4];
};

AF2_HD void mulhilo(uint32_t a, uint32_t b, uint32_t& hi, uint32_t& lo) {
  const uint64_t p = (uint64_t)a * b;
  hi = (uint32_t)(p >> 32);
  lo = (uint32_t)p;
}

// first 128-bit output of Philox4x32-10 for (seed, subsequence, offset)
AF2_HD U4 philox4x32_10(uint64_t seed, uint64_t subseq, uint64_t offset) {
  uint32_t c0 = (uint32_t)offset, c1 = (uint32_t)(offset >> 32);
  uint32_t c2 = (uint32_t)subseq, c3 = (uint32_t)(subseq >> 32);
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    uint32_t hi0, lo0, hi1, lo1;
    mulhilo(0xD2511F53u, c0, hi0, lo0);
    mulhilo(0xCD9E8D57u, c2, hi1, lo1);
    const uint32_t n0 = hi1 ^ c1 ^ k0;
    const uint32_t n2 = hi0 ^ c3 ^ k1;
    c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return U4{{c0, c1, c2, c3}};
}

// T = clamp(round(p * 256), 1, 255)
inline uint32_t threshold(double p) {
  long t = (long)(p * 256.0 + 0.5);
  return (uint32_t)(t < 1 ? 1 : (t > 255 ? 255 : t));
}

inline float rescale(uint32_t thresh) {
  return 256.0f / (float)(256u - thresh);
}

// what the kernels need besides the position
struct Params {
  uint64_t seed, offset;
  uint32_t thresh;   // T
  float rescale;     // 256 / (256 - T)
  int H4, W4;        // ceil(Lq / 4), ceil(Lk / 4)
};

AF2_HD uint64_t block_subseq(const Params& p, int bh, int ib, int jb) {
  return ((uint64_t)bh * (uint64_t)p.H4 + (uint64_t)ib) * (uint64_t)p.W4
      + (uint64_t)jb;
}

// the 4x4 block (ib, jb) = (i>>2, j>>2) of head bh
AF2_HD U4 block_bits(const Params& p, int bh, int ib, int jb) {
  return philox4x32_10(p.seed, block_subseq(p, bh, ib, jb), p.offset);
}

AF2_HD bool keep_from_block(const U4& blk, int i, int j, uint32_t thresh) {
  // selects, not a dynamic index: the block stays in registers
  const int wi = i & 3;
  const uint32_t w = wi == 0 ? blk.w[0] : wi == 1 ? blk.w[1]
                   : wi == 2 ? blk.w[2] : blk.w[3];
  return ((w >> (8 * (j & 3))) & 0xffu) >= thresh;
}

// reference form: one Philox call per element
AF2_HD bool keep(const Params& p, int bh, int i, int j) {
  return keep_from_block(block_bits(p, bh, i >> 2, j >> 2), i, j, p.thresh);
}

#if defined(__HIPCC__)
// value of `v` in lane (lane & ~3) + SRC of the caller's aligned quad
template <int SRC>
__device__ __forceinline__ uint32_t quad_bcast(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, SRC * 0x55, 0xf, 0xf,
                                            true);
#else
  return v;  // host pass only parses the kernels
#endif
}

// The MFMA 16x16 C layout used by the attention kernels gives a lane,
// per 64-wide tile, 4 consecutive positions on one axis (`reg`) times
// the positions l + 16c (l = lane & 15, c = 0..3) on the other.  Those
// 16 elements lie in 4 blocks, and the 4 lanes of an aligned quad need
// the same 4: lane (quad base + c) generates block c once and the quad
// shares it with DPP moves, instead of 4 Philox calls per lane.
//
// Returns 16 keep bits, bit c*4 + reg.
//  * ROWS_IN_REG = true  (forward, dQ): reg walks the query rows
//    i4*4 + reg, columns are j16 + 16c + l.
//  * ROWS_IN_REG = false (dK/dV, transposed tile): reg walks the key
//    columns j4*4 + reg, query rows are i16 + 16c + l.
// a4 is the block index on the reg axis, b16 the first position of the
// tile on the other axis (a multiple of 16).  All 64 lanes must be active.
template <bool ROWS_IN_REG>
__device__ __forceinline__ uint32_t keep_bits_c_layout(const Params& p,
                                                       int bh, int a4,
                                                       int b16, int lane) {
  const int l = lane & 15;
  const int b4 = (b16 >> 2) + (lane & 3) * 4 + (l >> 2);
  const U4 mine = ROWS_IN_REG ? block_bits(p, bh, a4, b4)
                              : block_bits(p, bh, b4, a4);
  uint32_t bits = 0;
#define AF2_DROP_STEP(C)                                                      \
  {                                                                           \
    uint32_t w0 = quad_bcast<C>(mine.w[0]), w1 = quad_bcast<C>(mine.w[1]);    \
    uint32_t w2 = quad_bcast<C>(mine.w[2]), w3 = quad_bcast<C>(mine.w[3]);    \
    if (ROWS_IN_REG) {                                                        \
      const int sh = 8 * (lane & 3); /* byte j & 3 of word reg */             \
      bits |= (uint32_t)(((w0 >> sh) & 0xffu) >= p.thresh) << (C * 4 + 0);    \
      bits |= (uint32_t)(((w1 >> sh) & 0xffu) >= p.thresh) << (C * 4 + 1);    \
      bits |= (uint32_t)(((w2 >> sh) & 0xffu) >= p.thresh) << (C * 4 + 2);    \
      bits |= (uint32_t)(((w3 >> sh) & 0xffu) >= p.thresh) << (C * 4 + 3);    \
    } else {                                                                  \
      const int wi = lane & 3;       /* word i & 3, byte reg */               \
      const uint32_t w = wi == 0 ? w0 : wi == 1 ? w1 : wi == 2 ? w2 : w3;     \
      bits |= (uint32_t)((w & 0xffu) >= p.thresh) << (C * 4 + 0);             \
      bits |= (uint32_t)(((w >> 8) & 0xffu) >= p.thresh) << (C * 4 + 1);      \
      bits |= (uint32_t)(((w >> 16) & 0xffu) >= p.thresh) << (C * 4 + 2);     \
      bits |= (uint32_t)((w >> 24) >= p.thresh) << (C * 4 + 3);               \
    }                                                                         \
  }
  AF2_DROP_STEP(0)
  AF2_DROP_STEP(1)
  AF2_DROP_STEP(2)
  AF2_DROP_STEP(3)
#undef AF2_DROP_STEP
  return bits;
}
#endif

}  // namespace attn_drop
