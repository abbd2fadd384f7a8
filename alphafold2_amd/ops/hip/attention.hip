// Fused flash-style attention for the Evoformer — gfx950 (CDNA4).
//
// Covers K1 of SURVEY.md §2.17: softmax(Q K^T * scale + pair_bias + mask) V
// for every attention in the trunk — MSA row attention (batch b*m, len n),
// MSA column attention (batch b*n, len m), both triangle self-attentions
// (batch b*n, len n, pair bias), and template pointwise attention.
//
// MI355X-first design decisions:
//  * MFMA bf16 16x16x32 tiles; fp32 accumulation.  Forward: one
//    workgroup = 8 waves = 128 query rows (FBQ/FNT); backward kernels
//    run 4-wave workgroups over 64-row tiles (BQ/NWAVES).  KV tiled by
//    64 with double-buffered LDS staging (fwd: single barrier/tile).
//  * The pair bias is NOT materialized per folded axis: the kernel takes
//    bias of shape (B / bias_repeat, h, Lq, Lk) and folds the repeat in
//    the index — the eager path would replicate it axial_dim times
//    (reference alphafold2.py:248), ~268 MB per triangle attention at
//    n=256.
//  * LDS tiles are XOR-swizzled (byte ^= (row&7)<<4) — a row-major
//    [64][64] bf16 tile read down a column is a 16-way bank conflict
//    otherwise (guide §6 G4).
//  * Online softmax entirely in registers; the P tile round-trips
//    through a per-wave swizzled LDS scratch to reach MFMA A-fragment
//    layout for P·V.
//  * Backward is FlashAttention-2 style: delta = rowsum(dO*O), a dQ
//    kernel and a dK/dV kernel, each recomputing P from (Q,K,bias,lse).
//    With a bias gradient wanted, dK/dV instead stores its bf16 dS tile
//    to a scratch; dQ = scale dS K streams that scratch and dBias is a
//    one-writer sum of it over bias_repeat.  The older path (dBias by
//    fp32 atomics, bounded by the chip's float-atomic rate) stays
//    selectable with ds_scratch_bytes = 0.
//
// MFMA fragment conventions (verified on HW by tools/mfma_probe.hip):
//  * C/D: col = lane&15, row = (lane>>4)*4 + reg   [guide §3, measured]
//  * A/B: the k axis is a pure reduction axis — any lane->k permutation
//    works if A and B agree; we use k = (lane>>4)*8 + j (contiguous 8,
//    16-byte ds_read per fragment).
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <ATen/hip/HIPGeneratorImpl.h>
#include <ATen/hip/HIPGraphsUtils.cuh>

#include "attn_dropout.h"
#include "colsum.h"
#include "common.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16_t;

namespace {

constexpr int BQ = 64;     // query rows per workgroup
constexpr int BK = 64;     // kv rows per tile
constexpr int DH = 64;     // head dim (template-fixed)
constexpr int NWAVES = 4;  // waves per workgroup; each owns 16 q rows
constexpr int ROWB = DH * sizeof(bf16_t);  // 128 bytes per tile row
constexpr float NEG_INF = -1e30f;

// XOR swizzle: spread 16B chunks of a column access across banks
__device__ __forceinline__ int swz(int row, int byte_in_row) {
  return row * ROWB + (byte_in_row ^ ((row & 7) << 4));
}

// strided (B, h, L, 64) tensor view: element strides, innermost dim
// contiguous.  Lets the kernels consume the Linear outputs' natural
// (B, L, h*64) layout through a permuted view — no contiguous() copies.
struct TView {
  const bf16_t* p;
  long bs, hs, rs;  // batch, head, row strides (elements)
  __device__ const bf16_t* base(int b, int h) const {
    return p + (long)b * bs + (long)h * hs;
  }
};
struct TViewMut {
  bf16_t* p;
  long bs, hs, rs;
  __device__ bf16_t* base(int b, int h) const {
    return p + (long)b * bs + (long)h * hs;
  }
};

// cooperative stage of a [rows<=64][64] bf16 tile global->LDS (swizzled).
// Each of 256 threads moves 2 16-byte chunks.  OOB rows zero-filled.
// row_stride in elements (bf16); rows are 64-element contiguous.
__device__ __forceinline__ void stage_tile(const bf16_t* __restrict__ g,
                                           long row_stride, int rows,
                                           char* lds) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    int idx = tid + pass * 256;        // chunk index 0..511
    int row = idx >> 3;                // 8 chunks per row
    int c16 = (idx & 7) << 4;          // byte offset in row
    float4 val = {0, 0, 0, 0};
    if (row < rows) {
      val = *reinterpret_cast<const float4*>(
          reinterpret_cast<const char*>(g + row * row_stride) + c16);
    }
    *reinterpret_cast<float4*>(lds + swz(row, c16)) = val;
  }
}

// stage a [rows<=64][<=64] bf16 tile with arbitrary row stride into a
// swizzled LDS tile; used for the pair-bias tile in the dK/dV kernel
// (its transposed per-lane reads would otherwise scatter 2B loads).
__device__ __forceinline__ void stage_tile_rowstride(
    const bf16_t* __restrict__ g, long row_stride, int rows, int cols,
    char* lds) {
  const int tid = threadIdx.x;
  if ((row_stride % 8) == 0 && (((uintptr_t)g) & 15) == 0) {
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
      int idx = tid + pass * 256;
      int row = idx >> 3;
      int c16 = (idx & 7) << 4;
      float4 val = {0, 0, 0, 0};
      if (row < rows && c16 < cols * (int)sizeof(bf16_t)) {
        val = *reinterpret_cast<const float4*>(
            reinterpret_cast<const char*>(g + row * row_stride) + c16);
      }
      *reinterpret_cast<float4*>(lds + swz(row, c16)) = val;
    }
  } else {  // unaligned fallback: scalar u16 staging
    for (int idx = tid; idx < 64 * 64; idx += 256) {
      int row = idx >> 6;
      int col = idx & 63;
      bf16_t val = (bf16_t)0.f;
      if (row < rows && col < cols) val = g[row * row_stride + col];
      *reinterpret_cast<bf16_t*>(
          lds + swz(row, col * (int)sizeof(bf16_t))) = val;
    }
  }
}

// stage a [rows<=64][64] bf16 tile TRANSPOSED into LDS ([col][row],
// swizzled): the PV B-operand wants V^T rows so its fragments become
// single 16-byte ds_reads instead of 8 scalar strided reads.
__device__ __forceinline__ void stage_tile_t(const bf16_t* __restrict__ g,
                                             long row_stride, int rows,
                                             char* lds) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    int idx = tid + pass * 256;
    int row = idx >> 3;                // source row (kv)
    int c8 = (idx & 7) << 3;           // first of 8 source cols (dv)
    float4 val = {0, 0, 0, 0};
    if (row < rows) {
      val = *reinterpret_cast<const float4*>(
          reinterpret_cast<const char*>(g + row * row_stride) + c8 * 2);
    }
    const bf16_t* vv = reinterpret_cast<const bf16_t*>(&val);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      *reinterpret_cast<bf16_t*>(
          lds + swz(c8 + j, row * (int)sizeof(bf16_t))) = vv[j];
    }
  }
}

// async-stage split (guide T14): issue the tile's global loads into
// registers early (overlapping prior compute), write LDS after the
// barrier.  The same registers can be stored in BOTH layouts (normal +
// transposed), halving global traffic for double-layout tiles.
struct StageRegs {
  float4 v0, v1;
};

__device__ __forceinline__ void stage_load(const bf16_t* __restrict__ g,
                                           long row_stride, int rows,
                                           StageRegs& r) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    int idx = tid + pass * 256;
    int row = idx >> 3;
    int c16 = (idx & 7) << 4;
    float4 val = {0, 0, 0, 0};
    if (row < rows) {
      val = *reinterpret_cast<const float4*>(
          reinterpret_cast<const char*>(g + row * row_stride) + c16);
    }
    (pass ? r.v1 : r.v0) = val;
  }
}

__device__ __forceinline__ void stage_store(const StageRegs& r, char* lds) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    int idx = tid + pass * 256;
    int row = idx >> 3;
    int c16 = (idx & 7) << 4;
    *reinterpret_cast<float4*>(lds + swz(row, c16)) = (pass ? r.v1 : r.v0);
  }
}

__device__ __forceinline__ void stage_store_t(const StageRegs& r, char* lds) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    int idx = tid + pass * 256;
    int row = idx >> 3;
    int c8 = (idx & 7) << 3;  // first of 8 source cols
    const float4 val = pass ? r.v1 : r.v0;
    const bf16_t* vv = reinterpret_cast<const bf16_t*>(&val);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      *reinterpret_cast<bf16_t*>(
          lds + swz(c8 + j, row * (int)sizeof(bf16_t))) = vv[j];
    }
  }
}

// block-width/row-count generic staging (the fwd kernel runs 512
// threads over a 128-row Q tile and 64-row K/V tiles)
template <int NT, int R>
struct StageRegsN {
  float4 v[(R * 8 + NT - 1) / NT];
};

template <int NT, int R>
__device__ __forceinline__ void stage_load_n(const bf16_t* __restrict__ g,
                                             long row_stride, int rows,
                                             StageRegsN<NT, R>& r) {
  constexpr int P = (R * 8 + NT - 1) / NT;
#pragma unroll
  for (int pass = 0; pass < P; ++pass) {
    int idx = threadIdx.x + pass * NT;
    int row = idx >> 3;
    int c16 = (idx & 7) << 4;
    float4 val = {0, 0, 0, 0};
    if (row < rows) {
      val = *reinterpret_cast<const float4*>(
          reinterpret_cast<const char*>(g + row * row_stride) + c16);
    }
    r.v[pass] = val;
  }
}

template <int NT, int R>
__device__ __forceinline__ void stage_store_n(const StageRegsN<NT, R>& r,
                                              char* lds) {
  constexpr int P = (R * 8 + NT - 1) / NT;
#pragma unroll
  for (int pass = 0; pass < P; ++pass) {
    int idx = threadIdx.x + pass * NT;
    int row = idx >> 3;
    int c16 = (idx & 7) << 4;
    *reinterpret_cast<float4*>(lds + swz(row, c16)) = r.v[pass];
  }
}

// column-wise-mapped variant for tiles that are ONLY stored transposed
// (fwd V^T): thread idx -> (row = idx&63, chunk = idx>>6), so within a
// wave the transposed-store byte offset `row*2` spans the full 0..126
// range -> ~2-way LDS bank conflict instead of the 16-way conflict of
// the row-wise mapping (where row*2 spans only 0..14 for fixed j).
// Global-load cost: each 128-byte row cacheline is read in 16B chunks
// by 8 different waves (L2-served) instead of one coalesced pull.
template <int NT>
__device__ __forceinline__ void stage_load_colwise_n(
    const bf16_t* __restrict__ g, long row_stride, int rows,
    StageRegsN<NT, 64>& r) {
  constexpr int P = (64 * 8 + NT - 1) / NT;
#pragma unroll
  for (int pass = 0; pass < P; ++pass) {
    int idx = threadIdx.x + pass * NT;
    int row = idx & 63;
    int c16 = (idx >> 6) << 4;
    float4 val = {0, 0, 0, 0};
    if (row < rows) {
      val = *reinterpret_cast<const float4*>(
          reinterpret_cast<const char*>(g + row * row_stride) + c16);
    }
    r.v[pass] = val;
  }
}

template <int NT>
__device__ __forceinline__ void stage_store_t_colwise_n(
    const StageRegsN<NT, 64>& r, char* lds) {
  constexpr int P = (64 * 8 + NT - 1) / NT;
#pragma unroll
  for (int pass = 0; pass < P; ++pass) {
    int idx = threadIdx.x + pass * NT;
    int row = idx & 63;
    int c8 = (idx >> 6) << 3;
    const float4 val = r.v[pass];
    const bf16_t* vv = reinterpret_cast<const bf16_t*>(&val);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      *reinterpret_cast<bf16_t*>(
          lds + swz(c8 + j, row * (int)sizeof(bf16_t))) = vv[j];
    }
  }
}

template <int NT, int R>
__device__ __forceinline__ void stage_store_t_n(const StageRegsN<NT, R>& r,
                                                char* lds) {
  constexpr int P = (R * 8 + NT - 1) / NT;
#pragma unroll
  for (int pass = 0; pass < P; ++pass) {
    int idx = threadIdx.x + pass * NT;
    int row = idx >> 3;
    int c8 = (idx & 7) << 3;
    const float4 val = r.v[pass];
    const bf16_t* vv = reinterpret_cast<const bf16_t*>(&val);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      *reinterpret_cast<bf16_t*>(
          lds + swz(c8 + j, row * (int)sizeof(bf16_t))) = vv[j];
    }
  }
}

// read an 8-bf16 A/B fragment (k = (lane>>4)*8 + j) for tile row `row`,
// k-block `kblk` (32 wide) from a swizzled LDS tile
__device__ __forceinline__ bf16x8 frag_row(const char* lds, int row,
                                           int kblk) {
  const int lane = threadIdx.x & 63;
  int byte_in_row = kblk * 64 + ((lane >> 4) << 4);
  return *reinterpret_cast<const bf16x8*>(lds + swz(row, byte_in_row));
}

// B-fragment where the matrix is stored [k][col] (k = tile row):
// lane needs col = lane&15, k = (lane>>4)*8 + j  -> 8 strided u16 reads
__device__ __forceinline__ bf16x8 frag_col(const char* lds, int col,
                                           int kblk) {
  const int lane = threadIdx.x & 63;
  bf16x8 out;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    int k = kblk * 32 + ((lane >> 4) << 3) + j;
    out[j] = *reinterpret_cast<const bf16_t*>(
        lds + swz(k, col * (int)sizeof(bf16_t)));
  }
  return out;
}

// ---------------------------------------------------------------------------
// forward

// S-tile layout per wave: rows 16 (q), cols 64 (kv) as 4 col-blocks of
// f32x4.  Row r of the wave lives in lanes [16*(r/4), 16*(r/4)+16) at
// reg r%4; a full row reduce is 4 col-blocks + shfl_xor over 16 lanes.
__device__ __forceinline__ float rowred_max(const f32x4 s[4], int reg) {
  float v = fmaxf(fmaxf(s[0][reg], s[1][reg]), fmaxf(s[2][reg], s[3][reg]));
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 16));
  return v;
}

__device__ __forceinline__ float rowred_sum(const f32x4 s[4], int reg) {
  float v = s[0][reg] + s[1][reg] + s[2][reg] + s[3][reg];
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) v += __shfl_xor(v, off, 16);
  return v;
}

constexpr int FBQ = 128;    // fwd query rows per workgroup
constexpr int FNT = 512;    // fwd threads (8 waves x 16 q rows)

// Attention-probability dropout operands (attn_dropout.h).  The
// HAS_DROP = false specialisations are empty, so those instantiations
// keep the kernel arguments and the code they had without dropout.
template <bool HAS_DROP> struct FwdDrop {};
template <> struct FwdDrop<true> {
  at::PhiloxCudaState philox;  // drawn from the generator (graph-safe) ...
  const int64_t* state_in;     // ... unless the caller gave (seed, offset)
  int64_t* state_out;          // (seed, offset) handed on to the backward
  uint32_t thresh;
  float rescale;
};
template <bool HAS_DROP> struct BwdDrop {};
template <> struct BwdDrop<true> {
  const int64_t* state;        // (seed, offset) the forward used
  uint32_t thresh;
  float rescale;
};

__device__ __forceinline__ attn_drop::Params drop_params(
    const BwdDrop<true>& d, int Lq, int Lk) {
  return attn_drop::Params{(uint64_t)d.state[0], (uint64_t)d.state[1],
                           d.thresh, d.rescale, (Lq + 3) >> 2, (Lk + 3) >> 2};
}

template <bool HAS_BIAS, bool HAS_MASK, bool HAS_DROP>
// minWavesPerEU=4 caps VGPRs at 128: the <bias,mask> variant was
// 129 VGPRs = 3 waves/SIMD = only ONE 8-wave block resident per CU.
// The HAS_DROP variants need ~20 more live registers for the Philox
// rounds and would spill under that cap: they take the uncapped
// allocation (one resident block) instead of scratch traffic.
__global__ __launch_bounds__(FNT, HAS_DROP ? 2 : 4)
void attn_fwd_kernel(TView q, TView k, TView v,
                     const bf16_t* __restrict__ bias,
                     const unsigned char* __restrict__ mask,
                     TViewMut out, float* __restrict__ lse,
                     int Lq, int Lk, int heads, int bias_repeat, int q_repeat,
                     float scale, FwdDrop<HAS_DROP> drop) {
  __shared__ char q_lds[FBQ * ROWB];
  // K / V^T / mask tiles are DOUBLE-buffered so the loop needs a single
  // __syncthreads per KV tile (placed between store and compute): the
  // barrier bounds the wave spread to one iteration, so store(t+1)
  // writes buf[(t+1)&1] while the slowest wave still reads buf[t&1] —
  // never the same buffer.  (~64KB LDS total: 2 blocks/CU preserved.)
  __shared__ char k_lds[2][BK * ROWB];
  __shared__ char vt_lds[2][BK * ROWB];  // V transposed: [dv][kv]
  __shared__ char p_lds[FNT / 64][16 * ROWB];
  __shared__ unsigned char m_lds[2][BK];

  const int qtile = blockIdx.x;
  const int bh = blockIdx.y;            // batch*heads + head
  const int batch = bh / heads;
  const int head = bh - batch * heads;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;

  const bf16_t* q_g = q.base(batch / q_repeat, head) + (long)qtile * FBQ * q.rs;
  const bf16_t* k_g = k.base(batch, head);
  const bf16_t* v_g = v.base(batch, head);
  const bf16_t* bias_g = nullptr;
  if (HAS_BIAS) {
    const int bias_batch = batch / bias_repeat;
    bias_g = bias + ((long)(bias_batch * heads + head) * Lq
                     + (long)qtile * FBQ) * Lk;
  }

  attn_drop::Params dpar{};
  if constexpr (HAS_DROP) {
    uint64_t seed, offset;
    if (drop.state_in != nullptr) {
      seed = (uint64_t)drop.state_in[0];
      offset = (uint64_t)drop.state_in[1];
    } else {
      auto so = at::cuda::philox::unpack(drop.philox);
      seed = std::get<0>(so);
      offset = std::get<1>(so);
      if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
        drop.state_out[0] = (int64_t)seed;
        drop.state_out[1] = (int64_t)offset;
      }
    }
    dpar = attn_drop::Params{seed, offset, drop.thresh, drop.rescale,
                             (Lq + 3) >> 2, (Lk + 3) >> 2};
  }

  const int q_rows = min(FBQ, Lq - qtile * FBQ);
  {
    StageRegsN<FNT, FBQ> qr;
    stage_load_n<FNT, FBQ>(q_g, q.rs, q_rows, qr);
    stage_store_n<FNT, FBQ>(qr, q_lds);
  }
  __syncthreads();

  // per-wave Q fragments (rows wave*16 + (lane&15))
  bf16x8 q_frag[2];
  const int qrow = wave * 16 + (lane & 15);
#pragma unroll
  for (int dblk = 0; dblk < 2; ++dblk)
    q_frag[dblk] = frag_row(q_lds, qrow, dblk);

  float m_i[4], l_i[4];
  f32x4 o_acc[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    m_i[r] = NEG_INF;
    l_i[r] = 0.f;
    o_acc[r] = f32x4{0, 0, 0, 0};
  }

  const int n_kv = (Lk + BK - 1) / BK;
  StageRegsN<FNT, BK> kreg, vreg;
  stage_load_n<FNT, BK>(k_g, k.rs, min(BK, Lk), kreg);
  stage_load_colwise_n<FNT>(v_g, v.rs, min(BK, Lk), vreg);
  for (int t = 0; t < n_kv; ++t) {
    const int kv_rows = min(BK, Lk - t * BK);
    const int buf = t & 1;
    stage_store_n<FNT, BK>(kreg, k_lds[buf]);
    stage_store_t_colwise_n<FNT>(vreg, vt_lds[buf]);
    if (HAS_MASK && threadIdx.x < BK) {
      m_lds[buf][threadIdx.x] = (threadIdx.x < kv_rows)
          ? mask[(long)batch * Lk + t * BK + threadIdx.x] : 0;
    }
    if (t + 1 < n_kv) {
      // next tile's loads fly across the barrier and under compute
      // (the ds_writes above read kreg/vreg at issue, in order)
      const int next_rows = min(BK, Lk - (t + 1) * BK);
      stage_load_n<FNT, BK>(k_g + (long)(t + 1) * BK * k.rs, k.rs,
                            next_rows, kreg);
      stage_load_colwise_n<FNT>(v_g + (long)(t + 1) * BK * v.rs, v.rs,
                                next_rows, vreg);
    }
    __syncthreads();

    // this tile's 16 keep bits per lane, generated here where the fewest
    // registers are live (no S tile yet); the integer work overlaps the
    // LDS reads of the first MFMAs
    uint32_t kb = 0;
    if constexpr (HAS_DROP) {
      kb = attn_drop::keep_bits_c_layout<true>(
          dpar, bh, (qtile * FBQ + wave * 16 + (lane >> 4) * 4) >> 2, t * BK,
          lane);
    }

    // S = Q K^T  (16 q x 64 kv per wave); setprio favors the MFMA
    // cluster when co-resident waves are staging (guide T5)
    f32x4 s[4];
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      f32x4 acc = {0, 0, 0, 0};
#pragma unroll
      for (int dblk = 0; dblk < 2; ++dblk) {
        bf16x8 kf = frag_row(k_lds[buf], c * 16 + (lane & 15), dblk);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(q_frag[dblk], kf, acc,
                                                      0, 0, 0);
      }
      s[c] = acc;
    }
    __builtin_amdgcn_s_setprio(0);

    // scale + bias + masking (C layout: row=(lane>>4)*4+reg, col=lane&15)
    const bf16_t* brow[4];
    if (HAS_BIAS) {
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int row = wave * 16 + (lane >> 4) * 4 + reg;
        brow[reg] = (row < q_rows)
            ? bias_g + (long)row * Lk + t * BK : nullptr;
      }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int col = c * 16 + (lane & 15);
      const bool col_ok = col < kv_rows &&
          (!HAS_MASK || m_lds[buf][col]);
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        float val = s[c][reg] * scale;
        if (HAS_BIAS && col_ok && brow[reg] != nullptr)
          val += to_f32(brow[reg][col]);
        s[c][reg] = col_ok ? val : NEG_INF;
      }
    }

    // online softmax
    float alpha[4], m_new[4];
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      float tile_max = rowred_max(s, reg);
      m_new[reg] = fmaxf(m_i[reg], tile_max);
      alpha[reg] = (m_i[reg] <= NEG_INF) ? 0.f : __expf(m_i[reg] - m_new[reg]);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        s[c][reg] = (m_new[reg] <= NEG_INF) ? 0.f
            : __expf(s[c][reg] - m_new[reg]);
      }
      l_i[reg] = l_i[reg] * alpha[reg] + rowred_sum(s, reg);
      m_i[reg] = m_new[reg];
#pragma unroll
      for (int c = 0; c < 4; ++c) o_acc[c][reg] *= alpha[reg];
    }

    // dropout after the softmax statistics: m_i and l_i (and lse) are
    // those of the undropped probabilities, only the P.V operand drops
    if constexpr (HAS_DROP) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          s[c][reg] = ((kb >> (c * 4 + reg)) & 1u)
              ? s[c][reg] * dpar.rescale : 0.f;
        }
      }
    }

    // P tile -> per-wave swizzled LDS scratch (C layout -> A layout)
    char* pw = p_lds[wave];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int col = c * 16 + (lane & 15);
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int row = (lane >> 4) * 4 + reg;
        *reinterpret_cast<bf16_t*>(pw + swz(row, col * (int)sizeof(bf16_t)))
            = (bf16_t)s[c][reg];
      }
    }
    // wave-internal LDS dependency: ds ops from this wave only
    // LDS-only wait: vmcnt stays open so the prefetched next
    // K/V tile's global loads keep flying under the PV MFMAs
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

    bf16x8 p_frag[2];
#pragma unroll
    for (int kblk = 0; kblk < 2; ++kblk)
      p_frag[kblk] = frag_row(pw, lane & 15, kblk);

    // O += P V  (B-operand = V^T rows: one b128 read per fragment)
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      f32x4 acc = o_acc[c];
#pragma unroll
      for (int kblk = 0; kblk < 2; ++kblk) {
        bf16x8 vf = frag_row(vt_lds[buf], c * 16 + (lane & 15), kblk);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(p_frag[kblk], vf, acc,
                                                      0, 0, 0);
      }
      o_acc[c] = acc;
    }
    __builtin_amdgcn_s_setprio(0);
  }

  // epilogue: O /= l, store out + lse
  bf16_t* out_g = out.base(batch, head) + (long)qtile * FBQ * out.rs;
  float* lse_g = lse + (long)bh * Lq + (long)qtile * FBQ;
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const int row = wave * 16 + (lane >> 4) * 4 + reg;
    const float linv = l_i[reg] > 0.f ? 1.f / l_i[reg] : 0.f;
    if (row < q_rows) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        out_g[(long)row * out.rs + c * 16 + (lane & 15)] =
            (bf16_t)(o_acc[c][reg] * linv);
      }
      if ((lane & 15) == 0) {
        lse_g[row] = (l_i[reg] > 0.f) ? m_i[reg] + logf(l_i[reg]) : NEG_INF;
      }
    }
  }
}

// ---------------------------------------------------------------------------
// backward: delta = rowsum(dO * O)

__global__ void attn_delta_kernel(TView dout, TView out,
                                  float* __restrict__ delta,
                                  int heads, int Lq, long rows) {
  // 8 rows per 64-lane wave: lane l covers row (l>>3), 8 channels
  // starting at (l&7)*8 — 16-byte loads, 1 KiB per wave transaction
  const long row = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 3;
  if (row >= rows) return;
  const int sub = threadIdx.x & 7;
  const int l = row % Lq;
  const long bh = row / Lq;
  const int b = bh / heads, h = bh - (bh / heads) * heads;
  const bf16_t* dp = dout.base(b, h) + (long)l * dout.rs + sub * 8;
  const bf16_t* op = out.base(b, h) + (long)l * out.rs + sub * 8;
  bf16x8 dv8 = *reinterpret_cast<const bf16x8*>(dp);
  bf16x8 ov8 = *reinterpret_cast<const bf16x8*>(op);
  float v = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) v += to_f32(dv8[j]) * to_f32(ov8[j]);
#pragma unroll
  for (int off = 4; off > 0; off >>= 1) v += __shfl_xor(v, off, 8);
  if (sub == 0) delta[row] = v;
}

// ---------------------------------------------------------------------------
// backward dQ: loop kv tiles; dS = P*(dP - delta)*scale; dQ += dS K

template <bool HAS_BIAS, bool HAS_MASK, bool HAS_DROP>
// minWavesPerEU=3 caps VGPRs at 170 (the <bias,mask> variant was 178
// -> 2 waves/SIMD); 3 waves = 3 resident 4-wave blocks per CU.
// HAS_DROP variants: uncapped, see attn_fwd_kernel.
__global__ __launch_bounds__(256, HAS_DROP ? 2 : 3)
void attn_bwd_dq_kernel(TView q, TView k, TView v,
                        const bf16_t* __restrict__ bias,
                        const unsigned char* __restrict__ mask,
                        TView dout,
                        const float* __restrict__ lse,
                        const float* __restrict__ delta,
                        TViewMut dq,
                        int Lq, int Lk, int heads, int bias_repeat, int q_repeat,
                        float scale, BwdDrop<HAS_DROP> drop) {
  __shared__ char q_lds[BQ * ROWB];
  __shared__ char do_lds[BQ * ROWB];
  __shared__ char k_lds[BK * ROWB];
  __shared__ char kt_lds[BK * ROWB];  // K transposed: [d][kv]
  __shared__ char v_lds[BK * ROWB];
  __shared__ char s_lds[NWAVES][16 * ROWB];
  __shared__ unsigned char m_lds[BK];

  attn_drop::Params dpar{};
  if constexpr (HAS_DROP) dpar = drop_params(drop, Lq, Lk);

  const int qtile = blockIdx.x;
  const int bh = blockIdx.y;
  const int batch = bh / heads;
  const int head = bh - batch * heads;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;

  const bf16_t* q_g = q.base(batch / q_repeat, head) + (long)qtile * BQ * q.rs;
  const bf16_t* do_g = dout.base(batch, head) + (long)qtile * BQ * dout.rs;
  const bf16_t* k_g = k.base(batch, head);
  const bf16_t* v_g = v.base(batch, head);
  const float* lse_g = lse + (long)bh * Lq + (long)qtile * BQ;
  const float* delta_g = delta + (long)bh * Lq + (long)qtile * BQ;
  const bf16_t* bias_g = nullptr;
  if (HAS_BIAS) {
    const int bias_batch = batch / bias_repeat;
    bias_g = bias + ((long)(bias_batch * heads + head) * Lq
                     + (long)qtile * BQ) * Lk;
  }

  const int q_rows = min(BQ, Lq - qtile * BQ);
  stage_tile(q_g, q.rs, q_rows, q_lds);
  stage_tile(do_g, dout.rs, q_rows, do_lds);
  __syncthreads();

  const int qrow = wave * 16 + (lane & 15);
  bf16x8 q_frag[2], do_frag[2];
#pragma unroll
  for (int dblk = 0; dblk < 2; ++dblk) {
    q_frag[dblk] = frag_row(q_lds, qrow, dblk);
    do_frag[dblk] = frag_row(do_lds, qrow, dblk);
  }

  // per-row lse/delta (C layout rows)
  float lse_r[4], delta_r[4];
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const int row = wave * 16 + (lane >> 4) * 4 + reg;
    lse_r[reg] = (row < q_rows) ? lse_g[row] : NEG_INF;
    delta_r[reg] = (row < q_rows) ? delta_g[row] : 0.f;
  }

  f32x4 dq_acc[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) dq_acc[c] = f32x4{0, 0, 0, 0};

  const int n_kv = (Lk + BK - 1) / BK;
  StageRegs kreg, vreg;
  stage_load(k_g, k.rs, min(BK, Lk), kreg);
  stage_load(v_g, v.rs, min(BK, Lk), vreg);
  for (int t = 0; t < n_kv; ++t) {
    const int kv_rows = min(BK, Lk - t * BK);
    __syncthreads();
    stage_store(kreg, k_lds);
    stage_store_t(kreg, kt_lds);  // one load feeds both layouts
    stage_store(vreg, v_lds);
    if (HAS_MASK && threadIdx.x < BK) {
      m_lds[threadIdx.x] = (threadIdx.x < kv_rows)
          ? mask[(long)batch * Lk + t * BK + threadIdx.x] : 0;
    }
    __syncthreads();
    if (t + 1 < n_kv) {
      const int next_rows = min(BK, Lk - (t + 1) * BK);
      stage_load(k_g + (long)(t + 1) * BK * k.rs, k.rs, next_rows, kreg);
      stage_load(v_g + (long)(t + 1) * BK * v.rs, v.rs, next_rows, vreg);
    }

    // this tile's keep bits, generated before the S and dP tiles are live
    uint32_t kb = 0;
    if constexpr (HAS_DROP) {
      kb = attn_drop::keep_bits_c_layout<true>(
          dpar, bh, (qtile * BQ + wave * 16 + (lane >> 4) * 4) >> 2, t * BK,
          lane);
    }

    // recompute S then P = exp(S*scale + bias - lse)
    f32x4 p[4], dp[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      f32x4 acc = {0, 0, 0, 0};
#pragma unroll
      for (int dblk = 0; dblk < 2; ++dblk) {
        bf16x8 kf = frag_row(k_lds, c * 16 + (lane & 15), dblk);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(q_frag[dblk], kf, acc,
                                                      0, 0, 0);
      }
      p[c] = acc;
    }
    const bf16_t* brow[4];
    if (HAS_BIAS) {
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int row = wave * 16 + (lane >> 4) * 4 + reg;
        brow[reg] = (row < q_rows)
            ? bias_g + (long)row * Lk + t * BK : nullptr;
      }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int col = c * 16 + (lane & 15);
      const bool col_ok = col < kv_rows && (!HAS_MASK || m_lds[col]);
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        float val = p[c][reg] * scale;
        if (HAS_BIAS && col_ok && brow[reg] != nullptr)
          val += to_f32(brow[reg][col]);
        p[c][reg] = (col_ok && lse_r[reg] > NEG_INF)
            ? __expf(val - lse_r[reg]) : 0.f;
      }
    }

    // dP = dO V^T : A = dO (k=dv), B col=kv row of V (k=dv contiguous)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      f32x4 acc = {0, 0, 0, 0};
#pragma unroll
      for (int dblk = 0; dblk < 2; ++dblk) {
        bf16x8 vf = frag_row(v_lds, c * 16 + (lane & 15), dblk);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(do_frag[dblk], vf, acc,
                                                      0, 0, 0);
      }
      dp[c] = acc;
    }

    // dropped forward: O = (keep * rescale * P) V, so dP carries the
    // same factor and delta = rowsum(dO * O) is still sum_j P dP
    if constexpr (HAS_DROP) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          dp[c][reg] = ((kb >> (c * 4 + reg)) & 1u)
              ? dp[c][reg] * dpar.rescale : 0.f;
        }
      }
    }

    // dS = P * (dP - delta) * scale  -> bf16 via LDS scratch
    char* sw = s_lds[wave];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int col = c * 16 + (lane & 15);
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int row = (lane >> 4) * 4 + reg;
        float ds = p[c][reg] * (dp[c][reg] - delta_r[reg]) * scale;
        *reinterpret_cast<bf16_t*>(sw + swz(row, col * (int)sizeof(bf16_t)))
            = (bf16_t)ds;
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

    bf16x8 ds_frag[2];
#pragma unroll
    for (int kblk = 0; kblk < 2; ++kblk)
      ds_frag[kblk] = frag_row(sw, lane & 15, kblk);

    // dQ += dS K : B col = d, k = kv -> b128 rows of the K^T tile
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      f32x4 acc = dq_acc[c];
#pragma unroll
      for (int kblk = 0; kblk < 2; ++kblk) {
        bf16x8 kf = frag_row(kt_lds, c * 16 + (lane & 15), kblk);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ds_frag[kblk], kf, acc,
                                                      0, 0, 0);
      }
      dq_acc[c] = acc;
    }
    __builtin_amdgcn_s_setprio(0);
  }

  bf16_t* dq_g = dq.base(batch, head) + (long)qtile * BQ * dq.rs;
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const int row = wave * 16 + (lane >> 4) * 4 + reg;
    if (row < q_rows) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        dq_g[(long)row * dq.rs + c * 16 + (lane & 15)] =
            (bf16_t)dq_acc[c][reg];
      }
    }
  }
}

// ---------------------------------------------------------------------------
// backward dK/dV (+ dBias): one block per kv tile, loop q tiles.
// Computes transposed products so kv is the row axis:
//   S^T = K Q^T,  P^T,  dV += P^T dO,  dP^T = V dO^T,
//   dS^T = P^T (dP^T - delta) scale,  dK += dS^T Q.

// dBias modes of the dK/dV kernel.  DBIAS_ATOMIC folds dS into the fp32
// dbias with one atomic per element (plain stores at bias_repeat == 1);
// DBIAS_STORE writes the bf16 dS^T tile to a [plane][kv][q] scratch that
// attn_bwd_dq_from_ds_kernel and attn_dbias_sum_kernel consume.
constexpr int DBIAS_NONE = 0;
constexpr int DBIAS_ATOMIC = 1;
constexpr int DBIAS_STORE = 2;

// dS scratch: one [n_k * 64][n_q * 64] bf16 plane per (batch, head) of
// the slice, kv-major.  The producer stores whole 64x64 tiles (zeros
// where q >= Lq or kv >= Lk), so every element of a plane is written;
// the consumers still read only rows kv < Lk and 16-byte chunks that
// start at q < Lq.
struct DsView {
  bf16_t* p;
  long plane;   // elements per (batch, head) plane
  int pitch;    // elements per kv row (n_q * 64)
  int bh0;      // batch * heads + head of the slice's first plane
};

template <bool HAS_BIAS, bool HAS_MASK, int DBIAS, bool HAS_DROP>
__global__ __launch_bounds__(256, 2)
void attn_bwd_dkv_kernel(TView q, TView k, TView v,
                         const bf16_t* __restrict__ bias,
                         const unsigned char* __restrict__ mask,
                         TView dout,
                         const float* __restrict__ lse,
                         const float* __restrict__ delta,
                         TViewMut dk, TViewMut dv,
                         float* __restrict__ dbias,
                         int dbias_chunks, long dbias_stride, DsView ds,
                         int Lq, int Lk, int heads, int bias_repeat, int q_repeat,
                         float scale, BwdDrop<HAS_DROP> drop) {
  __shared__ char k_lds[BK * ROWB];
  __shared__ char v_lds[BK * ROWB];
  __shared__ char q_lds[BQ * ROWB];
  __shared__ char qt_lds[BQ * ROWB];   // Q transposed: [d][q]
  __shared__ char do_lds[BQ * ROWB];
  __shared__ char dot_lds[BQ * ROWB];  // dO transposed: [dv][q]
  __shared__ char s_lds[NWAVES][16 * ROWB];
  __shared__ char b_lds[BQ * ROWB];  // bias tile [q][kv], swizzled
  __shared__ float lse_lds[BQ];
  __shared__ float delta_lds[BQ];
  __shared__ unsigned char m_lds[BK];

  attn_drop::Params dpar{};
  if constexpr (HAS_DROP) dpar = drop_params(drop, Lq, Lk);

  const int ktile = blockIdx.x;
  const int bh = ds.bh0 + blockIdx.y;
  const int batch = bh / heads;
  const int head = bh - batch * heads;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;

  const bf16_t* k_g = k.base(batch, head) + (long)ktile * BK * k.rs;
  const bf16_t* v_g = v.base(batch, head) + (long)ktile * BK * v.rs;
  const bf16_t* q_g = q.base(batch / q_repeat, head);
  const bf16_t* do_g = dout.base(batch, head);
  const float* lse_g = lse + (long)bh * Lq;
  const float* delta_g = delta + (long)bh * Lq;
  const bf16_t* bias_g = nullptr;
  float* dbias_g = nullptr;
  const int bias_batch = batch / bias_repeat;
  if (HAS_BIAS)
    bias_g = bias + (long)(bias_batch * heads + head) * Lq * Lk;
  if (DBIAS == DBIAS_ATOMIC) {
    // fold into one of `dbias_chunks` scratch copies: the repeat group
    // splits across chunks, cutting same-address atomic chain depth
    const int chunk = (batch % bias_repeat) % dbias_chunks;
    dbias_g = dbias + (long)chunk * dbias_stride
        + (long)(bias_batch * heads + head) * Lq * Lk;
  }
  // this wave's 16 kv rows of the (batch, head) dS plane
  bf16_t* ds_g = nullptr;
  if (DBIAS == DBIAS_STORE) {
    ds_g = ds.p + (long)blockIdx.y * ds.plane
        + (long)(ktile * BK + wave * 16) * ds.pitch;
  }

  const int kv_rows = min(BK, Lk - ktile * BK);
  stage_tile(k_g, k.rs, kv_rows, k_lds);
  stage_tile(v_g, v.rs, kv_rows, v_lds);
  if (HAS_MASK && threadIdx.x < BK) {
    m_lds[threadIdx.x] = (threadIdx.x < kv_rows)
        ? mask[(long)batch * Lk + ktile * BK + threadIdx.x] : 0;
  }
  __syncthreads();

  const int krow = wave * 16 + (lane & 15);
  bf16x8 k_frag[2], v_frag[2];
#pragma unroll
  for (int dblk = 0; dblk < 2; ++dblk) {
    k_frag[dblk] = frag_row(k_lds, krow, dblk);
    v_frag[dblk] = frag_row(v_lds, krow, dblk);
  }
  const bool krow_ok = krow < kv_rows && (!HAS_MASK || m_lds[krow]);
  // C-layout kv rows for this wave
  bool krow_ok_c[4];
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const int row = wave * 16 + (lane >> 4) * 4 + reg;
    krow_ok_c[reg] = row < kv_rows && (!HAS_MASK || m_lds[row]);
  }
  (void)krow_ok;

  f32x4 dk_acc[4], dv_acc[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    dk_acc[c] = f32x4{0, 0, 0, 0};
    dv_acc[c] = f32x4{0, 0, 0, 0};
  }

  const int n_q = (Lq + BQ - 1) / BQ;
  StageRegs qreg, doreg;
  stage_load(q_g, q.rs, min(BQ, Lq), qreg);
  stage_load(do_g, dout.rs, min(BQ, Lq), doreg);
  for (int t = 0; t < n_q; ++t) {
    const int q_rows = min(BQ, Lq - t * BQ);
    __syncthreads();
    stage_store(qreg, q_lds);
    stage_store_t(qreg, qt_lds);    // one load feeds both layouts
    stage_store(doreg, do_lds);
    stage_store_t(doreg, dot_lds);
    if (HAS_BIAS) {
      stage_tile_rowstride(bias_g + (long)t * BQ * Lk + (long)ktile * BK,
                           Lk, q_rows, min(BK, Lk - ktile * BK), b_lds);
    }
    if (threadIdx.x < BQ) {
      const int qq = t * BQ + threadIdx.x;
      lse_lds[threadIdx.x] = (threadIdx.x < q_rows) ? lse_g[qq] : NEG_INF;
      delta_lds[threadIdx.x] = (threadIdx.x < q_rows) ? delta_g[qq] : 0.f;
    }
    __syncthreads();
    if (t + 1 < n_q) {
      const int next_rows = min(BQ, Lq - (t + 1) * BQ);
      stage_load(q_g + (long)(t + 1) * BQ * q.rs, q.rs, next_rows, qreg);
      stage_load(do_g + (long)(t + 1) * BQ * dout.rs, dout.rs, next_rows,
                 doreg);
    }

    // S^T = K Q^T : A = K (k = d), B col = q row of Q (k = d contiguous)
    f32x4 pt[4], dpt[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      f32x4 acc = {0, 0, 0, 0};
#pragma unroll
      for (int dblk = 0; dblk < 2; ++dblk) {
        bf16x8 qf = frag_row(q_lds, c * 16 + (lane & 15), dblk);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k_frag[dblk], qf, acc,
                                                      0, 0, 0);
      }
      pt[c] = acc;
    }
    // P^T = exp(S^T*scale + bias^T - lse[q])
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int qcol = c * 16 + (lane & 15);       // q index in tile
      const float l = lse_lds[qcol];
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int kvrow = wave * 16 + (lane >> 4) * 4 + reg;
        float val = pt[c][reg] * scale;
        if (HAS_BIAS && krow_ok_c[reg] && qcol < q_rows)
          val += to_f32(*reinterpret_cast<const bf16_t*>(
              b_lds + swz(qcol, kvrow * (int)sizeof(bf16_t))));
        pt[c][reg] = (krow_ok_c[reg] && qcol < q_rows && l > NEG_INF)
            ? __expf(val - l) : 0.f;
      }
    }

    // keep bits of this wave's (kv rows) x (q cols) transposed tile
    uint32_t kb = 0;
    if constexpr (HAS_DROP) {
      kb = attn_drop::keep_bits_c_layout<false>(
          dpar, bh, (ktile * BK + wave * 16 + (lane >> 4) * 4) >> 2, t * BQ,
          lane);
    }

    // dV += P^T dO : A = P^T (k = q, via LDS), B col = dv, k = q
    // (with dropout the operand is keep * rescale * P^T; pt itself stays
    // undropped for dS^T below)
    char* sw = s_lds[wave];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int col = c * 16 + (lane & 15);
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int row = (lane >> 4) * 4 + reg;
        float pv = pt[c][reg];
        if constexpr (HAS_DROP)
          pv = ((kb >> (c * 4 + reg)) & 1u) ? pv * dpar.rescale : 0.f;
        *reinterpret_cast<bf16_t*>(sw + swz(row, col * (int)sizeof(bf16_t)))
            = (bf16_t)pv;
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    bf16x8 pt_frag[2];
#pragma unroll
    for (int kblk = 0; kblk < 2; ++kblk)
      pt_frag[kblk] = frag_row(sw, lane & 15, kblk);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      f32x4 acc = dv_acc[c];
#pragma unroll
      for (int kblk = 0; kblk < 2; ++kblk) {
        bf16x8 dof = frag_row(dot_lds, c * 16 + (lane & 15), kblk);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pt_frag[kblk], dof, acc,
                                                      0, 0, 0);
      }
      dv_acc[c] = acc;
    }
    __builtin_amdgcn_s_setprio(0);

    // dP^T = V dO^T : A = V (k = dv), B col = q, k = dv (contiguous)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      f32x4 acc = {0, 0, 0, 0};
#pragma unroll
      for (int dblk = 0; dblk < 2; ++dblk) {
        bf16x8 dof = frag_row(do_lds, c * 16 + (lane & 15), dblk);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(v_frag[dblk], dof, acc,
                                                      0, 0, 0);
      }
      dpt[c] = acc;
    }
    if constexpr (HAS_DROP) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          dpt[c][reg] = ((kb >> (c * 4 + reg)) & 1u)
              ? dpt[c][reg] * dpar.rescale : 0.f;
        }
      }
    }

    // dS^T = P^T (dP^T - delta[q]) scale ; emit dBias; stage for dK
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int qcol = c * 16 + (lane & 15);
      const float dl = delta_lds[qcol];
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        // dL/d(S*scale + bias): stored UNscaled (it IS the bias
        // gradient); the 1/sqrt(d) scale is applied to dK at the
        // epilogue instead
        float ds_total = pt[c][reg] * (dpt[c][reg] - dl);
        const int row = (lane >> 4) * 4 + reg;
        *reinterpret_cast<bf16_t*>(sw + swz(row, qcol * (int)sizeof(bf16_t)))
            = (bf16_t)ds_total;
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    bf16x8 dst_frag[2];
#pragma unroll
    for (int kblk = 0; kblk < 2; ++kblk)
      dst_frag[kblk] = frag_row(sw, lane & 15, kblk);

    if (DBIAS == DBIAS_STORE) {
      // wave-local drain of the [16 kv][64 q] bf16 tile the dK MFMA
      // reads: 128-byte rows, eight lanes per row, 16-byte stores.  The
      // tile is this wave's own scratch, so no block barrier; rows and
      // columns past Lk / Lq hold the zeros that P^T = 0 gave them.
#pragma unroll
      for (int pass = 0; pass < 2; ++pass) {
        const int row = pass * 8 + (lane >> 3);
        const int c16 = (lane & 7) << 4;
        const float4 val =
            *reinterpret_cast<const float4*>(sw + swz(row, c16));
        *reinterpret_cast<float4*>(
            reinterpret_cast<char*>(ds_g + (long)row * ds.pitch + t * BQ)
            + c16) = val;
      }
    }

    if (DBIAS == DBIAS_ATOMIC) {
      // cooperative transposed drain of the 64x64 dS tile from the four
      // per-wave scratches into dbias.  Lanes map to CONTIGUOUS kv
      // addresses so each store/atomic instruction coalesces; when
      // bias_repeat == 1 this block is the sole writer of its (q, kv)
      // range and plain stores replace atomics.
      __syncthreads();
      const int kvr = lane;            // 0..63, contiguous per wave
      for (int j = 0; j < 16; ++j) {
        const int qq = j * NWAVES + wave;
        if (qq < q_rows && kvr < kv_rows) {
          float dsv = to_f32(*reinterpret_cast<const bf16_t*>(
              s_lds[kvr >> 4] + swz(kvr & 15, qq * (int)sizeof(bf16_t))));
          float* addr = dbias_g + (long)(t * BQ + qq) * Lk
              + (long)ktile * BK + kvr;
          if (bias_repeat == 1) *addr = dsv; else atomicAdd(addr, dsv);
        }
      }
    }

    // dK += dS^T Q : B col = d, k = q -> b128 rows of the Q^T tile
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      f32x4 acc = dk_acc[c];
#pragma unroll
      for (int kblk = 0; kblk < 2; ++kblk) {
        bf16x8 qf = frag_row(qt_lds, c * 16 + (lane & 15), kblk);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dst_frag[kblk], qf, acc,
                                                      0, 0, 0);
      }
      dk_acc[c] = acc;
    }
    __builtin_amdgcn_s_setprio(0);
  }

  bf16_t* dk_g = dk.base(batch, head) + (long)ktile * BK * dk.rs;
  bf16_t* dv_g = dv.base(batch, head) + (long)ktile * BK * dv.rs;
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const int row = wave * 16 + (lane >> 4) * 4 + reg;
    if (row < kv_rows) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        dk_g[(long)row * dk.rs + c * 16 + (lane & 15)] =
            (bf16_t)(dk_acc[c][reg] * scale);
        dv_g[(long)row * dv.rs + c * 16 + (lane & 15)] =
            (bf16_t)dv_acc[c][reg];
      }
    }
  }
}

// ---------------------------------------------------------------------------
// backward dQ from stored dS: dQ[b,h] = scale * dS[b,h] K[b,h].  The
// dK/dV kernel (DBIAS_STORE) has left the unscaled bf16 dS^T, dropout
// and masks applied, in the scratch; this kernel streams it once and
// knows nothing of bias, mask, lse, delta, dropout, Q, V or dO.  One
// block per (64 q rows, batch*head), loop over kv tiles.  Both operands
// arrive kv-major while the MFMA wants the kv reduction axis
// lane-contiguous: the tiles go to LDS as they are (16-byte writes) and
// the fragments come back through gfx950's transposing LDS read, so no
// 2-byte transposition stores.  LDS tiles are double buffered: one
// barrier per kv tile.

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));

// 8-element MFMA operand (k = (lane>>4)*8 + j, as frag_row) whose k axis
// is the ROW axis of a swizzled row-major [64][64] bf16 LDS tile: lane
// (i = lane&15) gets column col0 + i of rows kblk*32 + (lane>>4)*8 + j.
// ds_read_b64_tr_b16 serves a 16-lane group one 4-row x 16-column block:
// lane 4a+p gives the address of row a, columns 4p..4p+3, and receives
// column (lane&15) of the 4 rows; two reads cover j = 0..3 and 4..7.
// The 16-byte swizzle keeps each 8-byte piece whole.  EXEC must be full.
__device__ __forceinline__ bf16x8 frag_tr(const char* lds, int col0,
                                          int kblk) {
  typedef __attribute__((address_space(3))) s16x4* lds_ptr;
  const int lane = threadIdx.x & 63;
  const int i = lane & 15;
  const int row = kblk * 32 + ((lane >> 4) << 3) + (i >> 2);
  const int colb = (col0 + ((i & 3) << 2)) * (int)sizeof(bf16_t);
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (lds_ptr)(lds + swz(row, colb)));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (lds_ptr)(lds + swz(row + 4, colb)));
  return __builtin_bit_cast(
      bf16x8, (s16x8)__builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

// stage_load with a column bound: chunks starting at col >= cols are 0
__device__ __forceinline__ void stage_load_rc(const bf16_t* __restrict__ g,
                                              long row_stride, int rows,
                                              int cols, StageRegs& r) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    int idx = tid + pass * 256;
    int row = idx >> 3;
    int c8 = (idx & 7) << 3;
    float4 val = {0, 0, 0, 0};
    if (row < rows && c8 < cols) {
      val = *reinterpret_cast<const float4*>(g + row * row_stride + c8);
    }
    (pass ? r.v1 : r.v0) = val;
  }
}

__global__ __launch_bounds__(256)
void attn_bwd_dq_from_ds_kernel(DsView ds, TView k, TViewMut dq,
                                int Lq, int Lk, int heads, float scale) {
  __shared__ __attribute__((aligned(16))) char ds_lds[2][BK * ROWB];  // [kv][q]
  __shared__ __attribute__((aligned(16))) char k_lds[2][BK * ROWB];   // [kv][d]

  const int qtile = blockIdx.x;
  const int bh = ds.bh0 + blockIdx.y;
  const int batch = bh / heads;
  const int head = bh - batch * heads;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;

  const bf16_t* ds_g = ds.p + (long)blockIdx.y * ds.plane + qtile * BQ;
  const bf16_t* k_g = k.base(batch, head);
  const int q_rows = min(BQ, Lq - qtile * BQ);

  f32x4 dq_acc[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) dq_acc[c] = f32x4{0, 0, 0, 0};

  const int n_kv = (Lk + BK - 1) / BK;
  StageRegs dsreg, kreg;
  stage_load_rc(ds_g, ds.pitch, min(BK, Lk), q_rows, dsreg);
  stage_load(k_g, k.rs, min(BK, Lk), kreg);
  for (int t = 0; t < n_kv; ++t) {
    char* dsl = ds_lds[t & 1];
    char* kl = k_lds[t & 1];
    stage_store(dsreg, dsl);
    stage_store(kreg, kl);
    // the buffer written here was last read two tiles ago, before the
    // barrier of the previous iteration
    __syncthreads();
    if (t + 1 < n_kv) {
      const int next_rows = min(BK, Lk - (t + 1) * BK);
      stage_load_rc(ds_g + (long)(t + 1) * BK * ds.pitch, ds.pitch,
                    next_rows, q_rows, dsreg);
      stage_load(k_g + (long)(t + 1) * BK * k.rs, k.rs, next_rows, kreg);
    }

    bf16x8 ds_frag[2];
#pragma unroll
    for (int kblk = 0; kblk < 2; ++kblk)
      ds_frag[kblk] = frag_tr(dsl, wave * 16, kblk);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      f32x4 acc = dq_acc[c];
#pragma unroll
      for (int kblk = 0; kblk < 2; ++kblk) {
        bf16x8 kf = frag_tr(kl, c * 16, kblk);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ds_frag[kblk], kf, acc,
                                                      0, 0, 0);
      }
      dq_acc[c] = acc;
    }
  }

  bf16_t* dq_g = dq.base(batch, head) + (long)qtile * BQ * dq.rs;
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const int row = wave * 16 + (lane >> 4) * 4 + reg;
    if (row < q_rows) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        dq_g[(long)row * dq.rs + c * 16 + (lane & 15)] =
            (bf16_t)(dq_acc[c][reg] * scale);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// dBias from stored dS: dbias[g,h,q,kv] = sum over the batch entries b of
// repeat group g that lie in the slice [b0, b1) of dS[b,h,q,kv].  One
// block per (group, head, 64x64 tile): fp32 accumulation in registers in
// the scratch's kv-major layout, then one transposition through LDS and
// plain stores — a single writer per element, so the result does not
// depend on scheduling.  A group whose first entry lies before b0 was
// started by an earlier slice and is added to when `accumulate` is set.

__global__ __launch_bounds__(256)
void attn_dbias_sum_kernel(DsView ds, float* __restrict__ dbias,
                           int Lq, int Lk, int heads, int bias_repeat,
                           int b0, int b1, int g0, int accumulate) {
  __shared__ float tile[BQ][BK + 1];  // [q][kv], padded against conflicts

  const int n_k = (Lk + BK - 1) / BK;
  const int qtile = blockIdx.x / n_k;
  const int ktile = blockIdx.x - qtile * n_k;
  const int g = g0 + blockIdx.y / heads;
  const int head = blockIdx.y % heads;
  const int q_cols = min(BQ, Lq - qtile * BQ);
  const int kv_rows = min(BK, Lk - ktile * BK);
  const int r_lo = max(g * bias_repeat, b0);
  const int r_hi = min((g + 1) * bias_repeat, b1);

  // thread -> two 16-byte chunks of the [kv][q] tile, as stage_load
  float acc[2][8];
  const bf16_t* src[2];
  bool ok[2];
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    const int idx = threadIdx.x + pass * 256;
    const int row = idx >> 3;
    const int c8 = (idx & 7) << 3;
    ok[pass] = row < kv_rows && c8 < q_cols;
    src[pass] = ds.p + ((long)(r_lo - b0) * heads + head) * ds.plane
        + (long)(ktile * BK + row) * ds.pitch + qtile * BQ + c8;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[pass][j] = 0.f;
  }
  const long step = (long)heads * ds.plane;
#pragma unroll 4
  for (int b = r_lo; b < r_hi; ++b) {
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
      if (ok[pass]) {
        const bf16x8 val = *reinterpret_cast<const bf16x8*>(src[pass]);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[pass][j] += to_f32(val[j]);
      }
      src[pass] += step;
    }
  }

#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    const int idx = threadIdx.x + pass * 256;
    const int row = idx >> 3;
    const int c8 = (idx & 7) << 3;
#pragma unroll
    for (int j = 0; j < 8; ++j) tile[c8 + j][row] = acc[pass][j];
  }
  __syncthreads();

  const bool add = accumulate && g * bias_repeat < b0;
  float* out = dbias + ((long)(g * heads + head) * Lq + (long)qtile * BQ) * Lk
      + (long)ktile * BK;
  const int kvc = threadIdx.x & 63;
  for (int qq = threadIdx.x >> 6; qq < q_cols; qq += NWAVES) {
    if (kvc < kv_rows) {
      float* addr = out + (long)qq * Lk + kvc;
      const float val = tile[qq][kvc];
      *addr = add ? *addr + val : val;
    }
  }
}

// ---------------------------------------------------------------------------
// dQ from stored dS with the dBias sum taken on the way (r10): the dQ
// kernel already holds every dS element in registers on its way to LDS,
// so the sum needs no second read of the scratch.  A block owns a q
// tile, a (repeat group, head) and a chunk of `epb` consecutive batch
// entries of that group inside the slice [b0, b1).  Per entry it forms
// and writes dQ exactly as attn_bwd_dq_from_ds_kernel does (same MFMA
// order, same scale on the accumulator: bit-equal, whatever the chunking
// and slicing); the staging pipeline runs on across entries.  Across its
// entries it keeps the fp32 sum of the dS it staged, 16 values per
// thread and kv tile, so NKV = ceil(Lk / 64) is a template parameter and
// at most DQ_DBIAS_MAX_NKV.  The sums, dQ's accumulators and the two
// staged tiles come to 210 VGPRs at the flagship's four tiles (2
// waves/SIMD; holding the kernel to 3 waves/SIMD spills 152 bytes per
// lane); five and six tiles spill 56 and 64 bytes at the 256 of 2
// waves/SIMD, which is why automatic stops at four.  After the last
// entry every kv tile is transposed through LDS as in
// attn_dbias_sum_kernel.  With `direct` (one chunk per group) the block
// is the only writer of its dbias elements and adds to a group that an
// earlier slice started; otherwise it stores its partial
// [chunk][group in slice][head][Lq][Lk] and colsum_fold_launch adds the
// chunks in order.  A chunk past the group's last entry of the slice
// stores zeros.

__device__ __forceinline__ void ds_sum_add(const float4& v, float* a) {
  const unsigned int u[4] = {__float_as_uint(v.x), __float_as_uint(v.y),
                             __float_as_uint(v.z), __float_as_uint(v.w)};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    a[2 * i] += __uint_as_float(u[i] << 16);
    a[2 * i + 1] += __uint_as_float(u[i] & 0xffff0000u);
  }
}

constexpr int DQ_DBIAS_MAX_NKV = 6;

// stage_load / stage_load_rc from a wave-uniform tile base and the
// thread's two 32-bit element offsets, which are the same for every tile
// and entry: the tile bases stay in scalar registers
__device__ __forceinline__ void stage_load_off(const bf16_t* __restrict__ g,
                                               const unsigned (&off)[2],
                                               int rows, bool col_ok0,
                                               bool col_ok1, StageRegs& r) {
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    const int row = (threadIdx.x + pass * 256) >> 3;
    float4 val = {0, 0, 0, 0};
    if (row < rows && (pass ? col_ok1 : col_ok0))
      val = *reinterpret_cast<const float4*>(g + off[pass]);
    (pass ? r.v1 : r.v0) = val;
  }
}

template <int NKV>
__global__ __launch_bounds__(256, 2)
void attn_bwd_dq_dbias_kernel(DsView ds, TView k, TViewMut dq,
                              float* __restrict__ sum_out, long chunk_stride,
                              int Lq, int Lk, int heads, float scale,
                              int bias_repeat, int b0, int b1, int g0,
                              int epb, int direct, int accumulate) {
  // [0], [1]: dS tiles [kv][q]; [2], [3]: K tiles [kv][d]; the fp32
  // transposition tile of the epilogue lies over them
  __shared__ __attribute__((aligned(16))) char lds[4][BK * ROWB];
  static_assert(sizeof(float) * BQ * (BK + 1) <= 4 * BK * ROWB, "tile");

  const int qtile = blockIdx.x;
  const int gl = blockIdx.y / heads;
  const int head = blockIdx.y - gl * heads;
  const int g = g0 + gl;
  const int r_lo = max(g * bias_repeat, b0);
  const int r_hi = min((g + 1) * bias_repeat, b1);
  const int e_lo = r_lo + blockIdx.z * epb;
  const int e_hi = min(e_lo + epb, r_hi);
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int q_rows = min(BQ, Lq - qtile * BQ);

  float sum[NKV][16];
#pragma unroll
  for (int t = 0; t < NKV; ++t)
#pragma unroll
    for (int j = 0; j < 16; ++j) sum[t][j] = 0.f;

  unsigned ds_off[2], k_off[2];
  bool col_ok[2];
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    const int idx = threadIdx.x + pass * 256;
    const int row = idx >> 3;
    const int c8 = (idx & 7) << 3;
    ds_off[pass] = (unsigned)row * (unsigned)ds.pitch + c8;
    k_off[pass] = (unsigned)row * (unsigned)k.rs + c8;
    col_ok[pass] = c8 < q_rows;
  }

  StageRegs dsreg, kreg;
  if (e_lo < e_hi) {
    stage_load_off(ds.p + ((long)(e_lo - b0) * heads + head) * ds.plane
                       + qtile * BQ,
                   ds_off, min(BK, Lk), col_ok[0], col_ok[1], dsreg);
    stage_load_off(k.base(e_lo, head), k_off, min(BK, Lk), true, true, kreg);
  }
  int buf = 0;
  for (int e = e_lo; e < e_hi; ++e) {
    const bf16_t* ds_g = ds.p + ((long)(e - b0) * heads + head) * ds.plane
        + qtile * BQ;
    const bf16_t* k_g = k.base(e, head);
    f32x4 dq_acc[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) dq_acc[c] = f32x4{0, 0, 0, 0};

#pragma unroll
    for (int t = 0; t < NKV; ++t) {
      char* dsl = lds[buf];
      char* kl = lds[2 + buf];
      buf ^= 1;
      stage_store(dsreg, dsl);
      stage_store(kreg, kl);
      ds_sum_add(dsreg.v0, sum[t]);
      ds_sum_add(dsreg.v1, sum[t] + 8);
      // the buffer written here was last read two tiles ago, before the
      // barrier of the previous tile
      __syncthreads();
      if (t + 1 < NKV) {
        const int next_rows = min(BK, Lk - (t + 1) * BK);
        stage_load_off(ds_g + (long)(t + 1) * BK * ds.pitch, ds_off,
                       next_rows, col_ok[0], col_ok[1], dsreg);
        stage_load_off(k_g + (long)(t + 1) * BK * k.rs, k_off, next_rows,
                       true, true, kreg);
      } else if (e + 1 < e_hi) {
        stage_load_off(ds_g + (long)heads * ds.plane, ds_off, min(BK, Lk),
                       col_ok[0], col_ok[1], dsreg);
        stage_load_off(k.base(e + 1, head), k_off, min(BK, Lk), true, true,
                       kreg);
      }

      bf16x8 ds_frag[2];
#pragma unroll
      for (int kblk = 0; kblk < 2; ++kblk)
        ds_frag[kblk] = frag_tr(dsl, wave * 16, kblk);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        f32x4 acc = dq_acc[c];
#pragma unroll
        for (int kblk = 0; kblk < 2; ++kblk) {
          bf16x8 kf = frag_tr(kl, c * 16, kblk);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ds_frag[kblk], kf,
                                                        acc, 0, 0, 0);
        }
        dq_acc[c] = acc;
      }
    }

    bf16_t* dq_g = dq.base(e, head) + (long)qtile * BQ * dq.rs;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int row = wave * 16 + (lane >> 4) * 4 + reg;
      if (row < q_rows) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          dq_g[(long)row * dq.rs + c * 16 + (lane & 15)] =
              (bf16_t)(dq_acc[c][reg] * scale);
        }
      }
    }
  }

  float (*tile)[BK + 1] = reinterpret_cast<float (*)[BK + 1]>(&lds[0][0]);
  const bool add = direct && accumulate && g * bias_repeat < b0;
  float* out = sum_out + (long)blockIdx.z * chunk_stride
      + ((long)((direct ? g : gl) * heads + head) * Lq + (long)qtile * BQ)
          * Lk;
  const int kvc = threadIdx.x & 63;
#pragma unroll
  for (int t = 0; t < NKV; ++t) {
    __syncthreads();   // the tile's last readers: the MFMAs, or tile t - 1
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
      const int idx = threadIdx.x + pass * 256;
      const int row = idx >> 3;
      const int c8 = (idx & 7) << 3;
#pragma unroll
      for (int j = 0; j < 8; ++j) tile[c8 + j][row] = sum[t][pass * 8 + j];
    }
    __syncthreads();
    const int kv_rows = min(BK, Lk - t * BK);
    for (int qq = threadIdx.x >> 6; qq < q_rows; qq += NWAVES) {
      if (kvc < kv_rows) {
        float* addr = out + (long)qq * Lk + t * BK + kvc;
        const float val = tile[qq][kvc];
        *addr = add ? *addr + val : val;
      }
    }
  }
}

// ---------------------------------------------------------------------------
// split backward (r02): the combined dK/dV kernel sits at 196-249 VGPRs
// = 2 waves/SIMD.  Splitting recomputes S^T/P^T once more (5 -> 7
// GEMM-equivalents) but the dV pass drops to ~4 waves/SIMD and the dK
// pass to 3 — at single-digit MfmaUtil the residency win dominates.

template <bool HAS_BIAS, bool HAS_MASK>
__global__ __launch_bounds__(256, 4)
void attn_bwd_dv_kernel(TView q, TView k,
                        const bf16_t* __restrict__ bias,
                        const unsigned char* __restrict__ mask,
                        TView dout,
                        const float* __restrict__ lse,
                        TViewMut dv,
                        int Lq, int Lk, int heads, int bias_repeat, int q_repeat,
                        float scale) {
  __shared__ char k_lds[BK * ROWB];
  __shared__ char q_lds[BQ * ROWB];
  __shared__ char dot_lds[BQ * ROWB];  // dO transposed: [dv][q]
  // bias tile [q][kv] and the P^T scratch ALIAS: the bias is fully
  // consumed (P^T formed in regs) before the scratch write, and the
  // barrier below separates the cross-wave read/write windows.  Saves
  // 8 KB -> 4 workgroups/CU.
  __shared__ char sb_lds[BQ * ROWB];
  char* b_lds = sb_lds;
  char (*s_lds)[16 * ROWB] =
      reinterpret_cast<char (*)[16 * ROWB]>(sb_lds);
  __shared__ float lse_lds[BQ];
  __shared__ unsigned char m_lds[BK];

  const int ktile = blockIdx.x;
  const int bh = blockIdx.y;
  const int batch = bh / heads;
  const int head = bh - batch * heads;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;

  const bf16_t* k_g = k.base(batch, head) + (long)ktile * BK * k.rs;
  const bf16_t* q_g = q.base(batch / q_repeat, head);
  const bf16_t* do_g = dout.base(batch, head);
  const float* lse_g = lse + (long)bh * Lq;
  const bf16_t* bias_g = HAS_BIAS
      ? bias + (long)((batch / bias_repeat) * heads + head) * Lq * Lk
      : nullptr;

  const int kv_rows = min(BK, Lk - ktile * BK);
  stage_tile(k_g, k.rs, kv_rows, k_lds);
  if (HAS_MASK && threadIdx.x < BK) {
    m_lds[threadIdx.x] = (threadIdx.x < kv_rows)
        ? mask[(long)batch * Lk + ktile * BK + threadIdx.x] : 0;
  }
  __syncthreads();

  bf16x8 k_frag[2];
#pragma unroll
  for (int dblk = 0; dblk < 2; ++dblk)
    k_frag[dblk] = frag_row(k_lds, wave * 16 + (lane & 15), dblk);
  bool krow_ok_c[4];
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const int row = wave * 16 + (lane >> 4) * 4 + reg;
    krow_ok_c[reg] = row < kv_rows && (!HAS_MASK || m_lds[row]);
  }

  f32x4 dv_acc[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) dv_acc[c] = f32x4{0, 0, 0, 0};

  const int n_q = (Lq + BQ - 1) / BQ;
  // direct (prefetch-free) staging: this kernel trades the async-stage
  // register cost for residency — occupancy is its lever
  for (int t = 0; t < n_q; ++t) {
    const int q_rows = min(BQ, Lq - t * BQ);
    __syncthreads();
    stage_tile(q_g + (long)t * BQ * q.rs, q.rs, q_rows, q_lds);
    stage_tile_t(do_g + (long)t * BQ * dout.rs, dout.rs, q_rows, dot_lds);
    if (HAS_BIAS) {
      stage_tile_rowstride(bias_g + (long)t * BQ * Lk + (long)ktile * BK,
                           Lk, q_rows, min(BK, Lk - ktile * BK), b_lds);
    }
    if (threadIdx.x < BQ) {
      const int qq = t * BQ + threadIdx.x;
      lse_lds[threadIdx.x] = (threadIdx.x < q_rows) ? lse_g[qq] : NEG_INF;
    }
    __syncthreads();

    // S^T = K Q^T ; P^T = exp(S^T*scale + bias^T - lse[q])
    f32x4 pt[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      f32x4 acc = {0, 0, 0, 0};
#pragma unroll
      for (int dblk = 0; dblk < 2; ++dblk) {
        bf16x8 qf = frag_row(q_lds, c * 16 + (lane & 15), dblk);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k_frag[dblk], qf, acc,
                                                      0, 0, 0);
      }
      pt[c] = acc;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int qcol = c * 16 + (lane & 15);
      const float l = lse_lds[qcol];
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int kvrow = wave * 16 + (lane >> 4) * 4 + reg;
        float val = pt[c][reg] * scale;
        if (HAS_BIAS && krow_ok_c[reg] && qcol < q_rows)
          val += to_f32(*reinterpret_cast<const bf16_t*>(
              b_lds + swz(qcol, kvrow * (int)sizeof(bf16_t))));
        pt[c][reg] = (krow_ok_c[reg] && qcol < q_rows && l > NEG_INF)
            ? __expf(val - l) : 0.f;
      }
    }

    // dV += P^T dO : A = P^T (k = q, via per-wave LDS scratch).
    // The scratch aliases the bias tile: wait until EVERY wave has
    // finished its bias reads before overwriting.
    if (HAS_BIAS) __syncthreads();
    char* sw = s_lds[wave];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int col = c * 16 + (lane & 15);
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int row = (lane >> 4) * 4 + reg;
        *reinterpret_cast<bf16_t*>(sw + swz(row, col * (int)sizeof(bf16_t)))
            = (bf16_t)pt[c][reg];
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    bf16x8 pt_frag[2];
#pragma unroll
    for (int kblk = 0; kblk < 2; ++kblk)
      pt_frag[kblk] = frag_row(sw, lane & 15, kblk);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      f32x4 acc = dv_acc[c];
#pragma unroll
      for (int kblk = 0; kblk < 2; ++kblk) {
        bf16x8 dof = frag_row(dot_lds, c * 16 + (lane & 15), kblk);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pt_frag[kblk], dof, acc,
                                                      0, 0, 0);
      }
      dv_acc[c] = acc;
    }
    __builtin_amdgcn_s_setprio(0);
  }

  bf16_t* dv_g = dv.base(batch, head) + (long)ktile * BK * dv.rs;
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const int row = wave * 16 + (lane >> 4) * 4 + reg;
    if (row < kv_rows) {
#pragma unroll
      for (int c = 0; c < 4; ++c)
        dv_g[(long)row * dv.rs + c * 16 + (lane & 15)] =
            (bf16_t)dv_acc[c][reg];
    }
  }
}

template <bool HAS_BIAS, bool HAS_MASK, bool NEED_DBIAS>
__global__ __launch_bounds__(256, 3)
void attn_bwd_dk_kernel(TView q, TView k, TView v,
                        const bf16_t* __restrict__ bias,
                        const unsigned char* __restrict__ mask,
                        TView dout,
                        const float* __restrict__ lse,
                        const float* __restrict__ delta,
                        TViewMut dk,
                        float* __restrict__ dbias,
                        int dbias_chunks, long dbias_stride,
                        int Lq, int Lk, int heads, int bias_repeat, int q_repeat,
                        float scale) {
  __shared__ char k_lds[BK * ROWB];
  __shared__ char v_lds[BK * ROWB];
  __shared__ char q_lds[BQ * ROWB];
  __shared__ char qt_lds[BQ * ROWB];   // Q transposed: [d][q]
  __shared__ char do_lds[BQ * ROWB];
  // bias tile and dS scratch alias (see dv kernel) — 48 KB total LDS
  __shared__ char sb_lds[BQ * ROWB];
  char* b_lds = sb_lds;
  char (*s_lds)[16 * ROWB] =
      reinterpret_cast<char (*)[16 * ROWB]>(sb_lds);
  __shared__ float lse_lds[BQ];
  __shared__ float delta_lds[BQ];
  __shared__ unsigned char m_lds[BK];

  const int ktile = blockIdx.x;
  const int bh = blockIdx.y;
  const int batch = bh / heads;
  const int head = bh - batch * heads;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;

  const bf16_t* k_g = k.base(batch, head) + (long)ktile * BK * k.rs;
  const bf16_t* v_g = v.base(batch, head) + (long)ktile * BK * v.rs;
  const bf16_t* q_g = q.base(batch / q_repeat, head);
  const bf16_t* do_g = dout.base(batch, head);
  const float* lse_g = lse + (long)bh * Lq;
  const float* delta_g = delta + (long)bh * Lq;
  const int bias_batch = batch / bias_repeat;
  const bf16_t* bias_g = HAS_BIAS
      ? bias + (long)(bias_batch * heads + head) * Lq * Lk : nullptr;
  float* dbias_g = nullptr;
  if (NEED_DBIAS) {
    const int chunk = (batch % bias_repeat) % dbias_chunks;
    dbias_g = dbias + (long)chunk * dbias_stride
        + (long)(bias_batch * heads + head) * Lq * Lk;
  }

  const int kv_rows = min(BK, Lk - ktile * BK);
  stage_tile(k_g, k.rs, kv_rows, k_lds);
  stage_tile(v_g, v.rs, kv_rows, v_lds);
  if (HAS_MASK && threadIdx.x < BK) {
    m_lds[threadIdx.x] = (threadIdx.x < kv_rows)
        ? mask[(long)batch * Lk + ktile * BK + threadIdx.x] : 0;
  }
  __syncthreads();

  const int krow = wave * 16 + (lane & 15);
  bf16x8 k_frag[2], v_frag[2];
#pragma unroll
  for (int dblk = 0; dblk < 2; ++dblk) {
    k_frag[dblk] = frag_row(k_lds, krow, dblk);
    v_frag[dblk] = frag_row(v_lds, krow, dblk);
  }
  bool krow_ok_c[4];
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const int row = wave * 16 + (lane >> 4) * 4 + reg;
    krow_ok_c[reg] = row < kv_rows && (!HAS_MASK || m_lds[row]);
  }

  f32x4 dk_acc[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) dk_acc[c] = f32x4{0, 0, 0, 0};

  const int n_q = (Lq + BQ - 1) / BQ;
  // prefetch-free staging (register diet for residency); the dual
  // q layouts still come from one StageRegs load
  StageRegs qreg;
  for (int t = 0; t < n_q; ++t) {
    const int q_rows = min(BQ, Lq - t * BQ);
    stage_load(q_g + (long)t * BQ * q.rs, q.rs, q_rows, qreg);
    __syncthreads();
    stage_store(qreg, q_lds);
    stage_store_t(qreg, qt_lds);
    stage_tile(do_g + (long)t * BQ * dout.rs, dout.rs, q_rows, do_lds);
    if (HAS_BIAS) {
      stage_tile_rowstride(bias_g + (long)t * BQ * Lk + (long)ktile * BK,
                           Lk, q_rows, min(BK, Lk - ktile * BK), b_lds);
    }
    if (threadIdx.x < BQ) {
      const int qq = t * BQ + threadIdx.x;
      lse_lds[threadIdx.x] = (threadIdx.x < q_rows) ? lse_g[qq] : NEG_INF;
      delta_lds[threadIdx.x] = (threadIdx.x < q_rows) ? delta_g[qq] : 0.f;
    }
    __syncthreads();

    // S^T = K Q^T ; P^T
    f32x4 pt[4], dpt[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      f32x4 acc = {0, 0, 0, 0};
#pragma unroll
      for (int dblk = 0; dblk < 2; ++dblk) {
        bf16x8 qf = frag_row(q_lds, c * 16 + (lane & 15), dblk);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k_frag[dblk], qf, acc,
                                                      0, 0, 0);
      }
      pt[c] = acc;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int qcol = c * 16 + (lane & 15);
      const float l = lse_lds[qcol];
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int kvrow = wave * 16 + (lane >> 4) * 4 + reg;
        float val = pt[c][reg] * scale;
        if (HAS_BIAS && krow_ok_c[reg] && qcol < q_rows)
          val += to_f32(*reinterpret_cast<const bf16_t*>(
              b_lds + swz(qcol, kvrow * (int)sizeof(bf16_t))));
        pt[c][reg] = (krow_ok_c[reg] && qcol < q_rows && l > NEG_INF)
            ? __expf(val - l) : 0.f;
      }
    }

    // dP^T = V dO^T
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      f32x4 acc = {0, 0, 0, 0};
#pragma unroll
      for (int dblk = 0; dblk < 2; ++dblk) {
        bf16x8 dof = frag_row(do_lds, c * 16 + (lane & 15), dblk);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(v_frag[dblk], dof, acc,
                                                      0, 0, 0);
      }
      dpt[c] = acc;
    }

    // dS^T = P^T (dP^T - delta[q]) ; stage for dK (+ dBias drain).
    // the scratch aliases the bias tile — barrier off the bias reads
    if (HAS_BIAS) __syncthreads();
    char* sw = s_lds[wave];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int qcol = c * 16 + (lane & 15);
      const float dl = delta_lds[qcol];
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        float ds_total = pt[c][reg] * (dpt[c][reg] - dl);
        const int row = (lane >> 4) * 4 + reg;
        *reinterpret_cast<bf16_t*>(sw + swz(row, qcol * (int)sizeof(bf16_t)))
            = (bf16_t)ds_total;
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    bf16x8 dst_frag[2];
#pragma unroll
    for (int kblk = 0; kblk < 2; ++kblk)
      dst_frag[kblk] = frag_row(sw, lane & 15, kblk);

    if (NEED_DBIAS) {
      __syncthreads();
      const int kvr = lane;
      // unrolling this drain costs ~30 VGPRs of address computation —
      // keep it rolled (occupancy is this kernel's lever)
#pragma clang loop unroll(disable)
      for (int j = 0; j < 16; ++j) {
        const int qq = j * NWAVES + wave;
        if (qq < q_rows && kvr < kv_rows) {
          float dsv = to_f32(*reinterpret_cast<const bf16_t*>(
              s_lds[kvr >> 4] + swz(kvr & 15, qq * (int)sizeof(bf16_t))));
          float* addr = dbias_g + (long)(t * BQ + qq) * Lk
              + (long)ktile * BK + kvr;
          if (bias_repeat == 1) *addr = dsv; else atomicAdd(addr, dsv);
        }
      }
    }

    // dK += dS^T Q
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      f32x4 acc = dk_acc[c];
#pragma unroll
      for (int kblk = 0; kblk < 2; ++kblk) {
        bf16x8 qf = frag_row(qt_lds, c * 16 + (lane & 15), kblk);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dst_frag[kblk], qf, acc,
                                                      0, 0, 0);
      }
      dk_acc[c] = acc;
    }
    __builtin_amdgcn_s_setprio(0);
  }

  bf16_t* dk_g = dk.base(batch, head) + (long)ktile * BK * dk.rs;
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const int row = wave * 16 + (lane >> 4) * 4 + reg;
    if (row < kv_rows) {
#pragma unroll
      for (int c = 0; c < 4; ++c)
        dk_g[(long)row * dk.rs + c * 16 + (lane & 15)] =
            (bf16_t)(dk_acc[c][reg] * scale);
    }
  }
}

// ---------------------------------------------------------------------------
// dropout keep mask as a tensor (tests, debugging): one element per
// thread through the per-element form of the shared function

__global__ void attn_dropout_mask_kernel(const int64_t* __restrict__ state,
                                         unsigned char* __restrict__ keep,
                                         int Lq, int Lk, long total,
                                         uint32_t thresh) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const attn_drop::Params p{(uint64_t)state[0], (uint64_t)state[1], thresh,
                            0.f, (Lq + 3) >> 2, (Lk + 3) >> 2};
  const int j = (int)(idx % Lk);
  const long bi = idx / Lk;
  const int i = (int)(bi % Lq);
  const int bh = (int)(bi / Lq);
  keep[idx] = attn_drop::keep(p, bh, i, j) ? 1 : 0;
}

}  // namespace

// ---------------------------------------------------------------------------
// host launchers

namespace {

TView make_view(const at::Tensor& t) {
  TORCH_CHECK(t.dim() == 4 && t.size(3) == DH && t.stride(3) == 1,
              "attention tensors must be 4-D (B, h, L, 64), last dim dense");
  TORCH_CHECK(t.stride(2) % 8 == 0 && t.stride(1) % 8 == 0 &&
              (t.size(0) == 1 || t.stride(0) % 8 == 0) &&
              reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0,
              "attention tensor base and strides must be 16-byte aligned");
  return TView{reinterpret_cast<const bf16_t*>(t.data_ptr()),
               t.stride(0), t.stride(1), t.stride(2)};
}

TViewMut make_view_mut(at::Tensor& t) {
  TView v = make_view(t);
  return TViewMut{const_cast<bf16_t*>(v.p), v.bs, v.hs, v.rs};
}

// every operand is reinterpreted as bf16 by the launchers: a wider dtype
// would be misread, a narrower one read past its end
void check_bf16(const at::Tensor& t, const at::Tensor& q, const char* fn,
                const char* name) {
  TORCH_CHECK(t.scalar_type() == at::kBFloat16, fn, ": ", name,
              " must be bf16, got ", t.scalar_type());
  TORCH_CHECK(t.device() == q.device(), fn, ": ", name,
              " must be on q's device");
}

// shapes the kernels index with: q (B / q_repeat, H, Lq, 64),
// k and v (B, H, Lk, 64), bias (B / bias_repeat, H, Lq, Lk)
void check_qkv_bias(const at::Tensor& q, const at::Tensor& k,
                    const at::Tensor& v,
                    const c10::optional<at::Tensor>& bias,
                    long bias_repeat, long q_repeat, const char* fn) {
  check_bf16(q, q, fn, "q");
  check_bf16(k, q, fn, "k");
  check_bf16(v, q, fn, "v");
  TORCH_CHECK(q.dim() == 4 && k.dim() == 4 && v.dim() == 4, fn,
              ": q, k and v must be 4-D (B, h, L, 64)");
  TORCH_CHECK(q_repeat >= 1 && bias_repeat >= 1, fn,
              ": q_repeat and bias_repeat must be >= 1");
  const long B = k.size(0), H = q.size(1), Lq = q.size(2), Lk = k.size(2);
  TORCH_CHECK(q.size(0) * q_repeat == B, fn,
              ": q batch must be B / q_repeat");
  TORCH_CHECK(k.size(1) == H && v.size(0) == B && v.size(1) == H &&
              v.size(2) == Lk, fn,
              ": k and v must both be (B, h, Lk, 64) with q's head count");
  if (bias.has_value()) {
    check_bf16(*bias, q, fn, "bias");
    TORCH_CHECK(B % bias_repeat == 0, fn, ": batch ", B,
                " is not divisible by bias_repeat ", bias_repeat);
    TORCH_CHECK(bias->dim() == 4 && bias->size(0) == B / bias_repeat &&
                bias->size(1) == H && bias->size(2) == Lq &&
                bias->size(3) == Lk, fn,
                ": bias must be (B / bias_repeat, h, Lq, Lk) = (",
                B / bias_repeat, ", ", H, ", ", Lq, ", ", Lk, "), got ",
                bias->sizes());
  }
}

void check_dropout_p(double p, const char* fn) {
  TORCH_CHECK(p > 0.0 && p < 1.0, fn, ": dropout_p must satisfy 0 < p < 1, "
              "got ", p);
}

// (seed, offset) as the kernels read it: int64[2] on q's device
void check_rng_state(const at::Tensor& s, const at::Tensor& q,
                     const char* fn) {
  TORCH_CHECK(s.scalar_type() == at::kLong && s.numel() == 2 &&
              s.is_contiguous(), fn,
              ": rng_state must be a contiguous int64 tensor of 2 elements "
              "(seed, offset), got ", s.scalar_type(), " ", s.sizes());
  TORCH_CHECK(s.device() == q.device(), fn,
              ": rng_state must be on q's device");
}

}  // namespace

std::vector<at::Tensor> attn_fwd(at::Tensor q, at::Tensor k, at::Tensor v,
                                 c10::optional<at::Tensor> bias,
                                 c10::optional<at::Tensor> mask,
                                 long bias_repeat, double scale,
                                 long q_repeat, double dropout_p,
                                 c10::optional<at::Tensor> rng_state) {
  TORCH_CHECK(q.scalar_type() == at::kBFloat16, "attn_fwd: bf16 only");
  check_qkv_bias(q, k, v, bias, bias_repeat, q_repeat, "attn_fwd");
  const int B = k.size(0), H = q.size(1), Lq = q.size(2), Lk = k.size(2);
  const bool has_drop = dropout_p != 0.0;
  if (has_drop) {
    check_dropout_p(dropout_p, "attn_fwd");
    if (rng_state.has_value()) check_rng_state(*rng_state, q, "attn_fwd");
  }

  // out in (B, Lq, H, DH) memory (the layout downstream Linears want),
  // exposed as a (B, H, Lq, DH) strided view
  auto out_bnhd = at::empty({B, Lq, H, DH}, q.options());
  auto out = out_bnhd.permute({0, 2, 1, 3});
  auto lse = at::empty({B, H, Lq}, q.options().dtype(at::kFloat));

  const bool has_bias = bias.has_value();
  const bool has_mask = mask.has_value();
  at::Tensor bias_c, mask_u8;
  if (has_bias) bias_c = bias->contiguous();
  if (has_mask) {
    // the kernel indexes mask[batch * Lk + j]: a broadcast (1, Lk) mask
    // at B > 1 would read out of bounds (advisory r01)
    TORCH_CHECK(mask->dim() == 2 && mask->size(0) == B &&
                mask->size(1) == Lk,
                "attn_fwd: mask must be (B, Lk); expand broadcast masks "
                "host-side");
    mask_u8 = mask->to(at::kByte).contiguous();
  }

  dim3 grid((Lq + FBQ - 1) / FBQ, B * H);
  auto stream = at::cuda::getCurrentHIPStream();
  TView qv = make_view(q), kv = make_view(k), vv = make_view(v);
  TViewMut ov = make_view_mut(out);

#define DISPATCH(HB, HM, HD, DROP)                                            \
  hipLaunchKernelGGL((attn_fwd_kernel<HB, HM, HD>), grid, dim3(FNT), 0,       \
      stream, qv, kv, vv,                                                     \
      has_bias ? reinterpret_cast<const bf16_t*>(bias_c.data_ptr()) : nullptr,\
      has_mask ? mask_u8.data_ptr<unsigned char>() : nullptr,                 \
      ov, lse.data_ptr<float>(),                                              \
      Lq, Lk, H, (int)bias_repeat, (int)q_repeat, (float)scale, DROP)

  if (!has_drop) {
    const FwdDrop<false> nd{};
    if (has_bias && has_mask) DISPATCH(true, true, false, nd);
    else if (has_bias) DISPATCH(true, false, false, nd);
    else if (has_mask) DISPATCH(false, true, false, nd);
    else DISPATCH(false, false, false, nd);
    return {out, lse};
  }

  FwdDrop<true> dr{};
  dr.thresh = attn_drop::threshold(dropout_p);
  dr.rescale = attn_drop::rescale(dr.thresh);
  at::Tensor state;
  if (rng_state.has_value()) {
    state = *rng_state;
    dr.state_in = state.data_ptr<int64_t>();
    dr.state_out = nullptr;
  } else {
    // each 4x4 block is its own subsequence and uses one 128-bit output
    // (4 values); the PhiloxCudaState goes to the kernel by value and is
    // unpacked there, which keeps a captured graph correct on replay
    auto gen = at::get_generator_or_default<at::CUDAGeneratorImpl>(
        c10::nullopt, at::cuda::detail::getDefaultCUDAGenerator());
    {
      std::lock_guard<std::mutex> lock(gen->mutex_);
      dr.philox = gen->philox_cuda_state(4);
    }
    state = at::empty({2}, q.options().dtype(at::kLong));
    dr.state_in = nullptr;
    dr.state_out = state.data_ptr<int64_t>();
  }
  if (has_bias && has_mask) DISPATCH(true, true, true, dr);
  else if (has_bias) DISPATCH(true, false, true, dr);
  else if (has_mask) DISPATCH(false, true, true, dr);
  else DISPATCH(false, false, true, dr);
#undef DISPATCH
  return {out, lse, state};
}

at::Tensor attn_dropout_mask(at::Tensor rng_state, long B, long H, long Lq,
                             long Lk, double dropout_p) {
  check_dropout_p(dropout_p, "attn_dropout_mask");
  check_rng_state(rng_state, rng_state, "attn_dropout_mask");
  TORCH_CHECK(rng_state.is_cuda(), "attn_dropout_mask: rng_state must be on "
              "the GPU");
  TORCH_CHECK(B > 0 && H > 0 && Lq > 0 && Lk > 0,
              "attn_dropout_mask: B, H, Lq and Lk must be positive");
  auto keep = at::empty({B, H, Lq, Lk},
                        rng_state.options().dtype(at::kByte));
  const long total = keep.numel();
  const int block = 256;
  const long grid = (total + block - 1) / block;
  TORCH_CHECK(B * H <= INT_MAX && grid <= INT_MAX,
              "attn_dropout_mask: shape too large");
  hipLaunchKernelGGL(attn_dropout_mask_kernel, dim3(grid), dim3(block), 0,
                     at::cuda::getCurrentHIPStream(),
                     rng_state.data_ptr<int64_t>(),
                     keep.data_ptr<unsigned char>(), (int)Lq, (int)Lk, total,
                     attn_drop::threshold(dropout_p));
  return keep;
}

std::vector<at::Tensor> attn_bwd(at::Tensor dout, at::Tensor q, at::Tensor k,
                                 at::Tensor v, at::Tensor out, at::Tensor lse,
                                 c10::optional<at::Tensor> bias,
                                 c10::optional<at::Tensor> mask,
                                 long bias_repeat, double scale,
                                 bool need_dbias, long q_repeat,
                                 c10::optional<at::Tensor> dq_out,
                                 c10::optional<at::Tensor> dk_out,
                                 c10::optional<at::Tensor> dv_out,
                                 double dropout_p,
                                 c10::optional<at::Tensor> rng_state,
                                 c10::optional<int64_t> ds_scratch_bytes,
                                 c10::optional<at::Tensor> delta_in,
                                 c10::optional<int64_t> dq_entries_per_block) {
  check_qkv_bias(q, k, v, bias, bias_repeat, q_repeat, "attn_bwd");
  const bool has_drop = dropout_p != 0.0;
  BwdDrop<true> dr{};
  if (has_drop) {
    check_dropout_p(dropout_p, "attn_bwd");
    TORCH_CHECK(rng_state.has_value(),
                "attn_bwd: dropout_p > 0 requires the forward's rng_state");
    check_rng_state(*rng_state, q, "attn_bwd");
    dr.state = rng_state->data_ptr<int64_t>();
    dr.thresh = attn_drop::threshold(dropout_p);
    dr.rescale = attn_drop::rescale(dr.thresh);
  }
  const BwdDrop<false> nd{};
  const int B = k.size(0), H = q.size(1), Lq = q.size(2), Lk = k.size(2);
  check_bf16(dout, q, "attn_bwd", "dout");
  check_bf16(out, q, "attn_bwd", "out");
  TORCH_CHECK(dout.dim() == 4 && dout.size(0) == B && dout.size(1) == H &&
              dout.size(2) == Lq && dout.size(3) == DH &&
              out.sizes() == dout.sizes(),
              "attn_bwd: dout and out must be (B, h, Lq, 64)");
  TORCH_CHECK(lse.scalar_type() == at::kFloat && lse.is_contiguous() &&
              lse.numel() == (long)B * H * Lq && lse.device() == q.device(),
              "attn_bwd: lse must be contiguous fp32 (B, h, Lq)");
  TORCH_CHECK(!need_dbias || bias.has_value(),
              "attn_bwd: need_dbias requires a bias");
  TORCH_CHECK(dq_out.has_value() == dk_out.has_value() &&
              dq_out.has_value() == dv_out.has_value(),
              "attn_bwd: dq_out, dk_out and dv_out must be given together");
  if (dq_out.has_value()) {
    check_bf16(*dq_out, q, "attn_bwd", "dq_out");
    check_bf16(*dk_out, q, "attn_bwd", "dk_out");
    check_bf16(*dv_out, q, "attn_bwd", "dv_out");
    // dq is written per batch entry even under q_repeat (the caller
    // folds the tie group afterwards)
    TORCH_CHECK(dq_out->dim() == 4 && dq_out->size(0) == B &&
                dq_out->size(1) == H && dq_out->size(2) == Lq &&
                dq_out->size(3) == DH,
                "attn_bwd: dq_out must be (B, h, Lq, 64)");
    TORCH_CHECK(dk_out->sizes() == k.sizes() && dv_out->sizes() == v.sizes(),
                "attn_bwd: dk_out and dv_out must have k's and v's shapes");
  }
  if (dout.stride(3) != 1) dout = dout.contiguous();

  // delta = rowsum(dO * O): computed here, or handed in by a caller whose
  // own pass over dO and O already formed it (attn_gate_bwd)
  at::Tensor delta;
  if (delta_in.has_value()) {
    delta = *delta_in;
    TORCH_CHECK(delta.scalar_type() == at::kFloat && delta.is_contiguous() &&
                delta.numel() == (long)B * H * Lq &&
                delta.device() == q.device(),
                "attn_bwd: delta must be contiguous fp32 (B, h, Lq)");
  } else {
    delta = at::empty({B, H, Lq}, lse.options());
  }
  // gradients written through strided views — either caller-provided
  // slices of a packed buffer (no concatenation in autograd) or fresh
  // (B, L, H, DH) memory viewed (B, H, L, DH)
  at::Tensor dq, dk, dv;
  if (dq_out.has_value()) {
    dq = *dq_out; dk = *dk_out; dv = *dv_out;
  } else {
    dq = at::empty({B, Lq, H, DH}, q.options()).permute({0, 2, 1, 3});
    dk = at::empty({B, Lk, H, DH}, q.options()).permute({0, 2, 1, 3});
    dv = at::empty({B, Lk, H, DH}, q.options()).permute({0, 2, 1, 3});
  }
  at::Tensor dbias;
  // chunks > 1 shortens same-address atomic chains but the extra
  // zeros+sum traffic measured NET-NEGATIVE (tri bwd 4.0 -> 4.3 ms at
  // chunks=8, tools/attn_bench.py) — keep a single copy
  int dbias_chunks = 1;

  // split dV/dK passes (4/3 waves per SIMD, but prefetch-free and
  // +40% flops): measured SLOWER end-to-end than the combined kernel
  // (748 vs 699 ms/step, r02) — combined stays default;
  // AF2AMD_SPLIT_DKV=1 re-enables for tuning.
  static const bool split_dkv = [] {
    const char* e = getenv("AF2AMD_SPLIT_DKV");
    return e != nullptr && e[0] == '1';
  }();

  // dS scratch path (docs/KERNELS.md "Attention backward: stored dS"):
  // with a bias gradient wanted, the dK/dV kernel stores its bf16 dS
  // tile instead of adding it to dbias with float atomics, dQ is a
  // plain dS K product over that scratch and dbias a one-writer sum.
  // The scratch is capped in bytes — a memory budget, not a tuned
  // optimum; above the cap the three kernels run over consecutive batch
  // slices that reuse one scratch.  0 selects the atomic path.
  static const int64_t ds_scratch_default = [] {
    const char* e = getenv("AF2AMD_DS_SCRATCH_BYTES");
    if (e == nullptr || e[0] == '\0') return (int64_t)2 << 30;
    char* end = nullptr;
    const long long val = strtoll(e, &end, 10);
    TORCH_CHECK(end != e && *end == '\0' && val >= 0,
                "AF2AMD_DS_SCRATCH_BYTES must be a non-negative byte count, "
                "got '", e, "'");
    return (int64_t)val;
  }();
  const int64_t ds_cap = ds_scratch_bytes.value_or(ds_scratch_default);
  TORCH_CHECK(ds_cap >= 0, "attn_bwd: ds_scratch_bytes must be >= 0, got ",
              ds_cap);
  const bool use_ds = need_dbias && ds_cap > 0 && !split_dkv;

  // dBias out of the dQ-from-dS kernel (attn_bwd_dq_dbias_kernel):
  // batch entries of a repeat group per block, None = what fills the
  // device, 0 = the two kernels (dQ, then the sum), as
  // AF2AMD_DQ_DBIAS_FUSED=0 selects everywhere.  Automatic takes the
  // fused kernel up to four kv tiles (Lk <= 256, what was measured); an
  // explicit count takes it up to six (Lk <= 384).  Longer Lk, and slices with more dbias elements
  // than an int holds, stay on the two kernels.
  static const bool dq_dbias_fused_env = [] {
    const char* e = getenv("AF2AMD_DQ_DBIAS_FUSED");
    return !(e != nullptr && e[0] == '0');
  }();
  const int64_t epb_arg = dq_entries_per_block.value_or(-1);
  TORCH_CHECK(!dq_entries_per_block.has_value() || epb_arg >= 0,
              "attn_bwd: dq_entries_per_block must be >= 0, got ", epb_arg);

  const int n_q = (Lq + BQ - 1) / BQ, n_k = (Lk + BK - 1) / BK;
  const long ds_plane = (long)n_q * BQ * n_k * BK;  // padded to whole tiles
  int ds_slice = 0;  // batch entries per slice
  at::Tensor ds_buf;
  if (use_ds) {
    const int64_t per_entry = (int64_t)H * ds_plane * sizeof(bf16_t);
    ds_slice = (int)std::min<int64_t>(
        B, std::max<int64_t>(1, ds_cap / per_entry));
    TORCH_CHECK((long)n_q * BQ <= INT_MAX, "attn_bwd: Lq too large");
    ds_buf = at::empty({(long)ds_slice * H * ds_plane}, q.options());
    TORCH_CHECK(reinterpret_cast<uintptr_t>(ds_buf.data_ptr()) % 16 == 0,
                "attn_bwd: dS scratch must be 16-byte aligned");
    // one writer per element: no zero fill, no chunk dimension to fold
    dbias = at::empty({B / bias_repeat, H, Lq, Lk},
                      q.options().dtype(at::kFloat));
  } else if (need_dbias) {
    dbias = at::zeros({dbias_chunks, B / bias_repeat, H, Lq, Lk},
                      q.options().dtype(at::kFloat));
  }
  const bool has_bias = bias.has_value();
  const bool has_mask = mask.has_value();
  at::Tensor bias_c, mask_u8;
  if (has_bias) bias_c = bias->contiguous();
  if (has_mask) {
    TORCH_CHECK(mask->dim() == 2 && mask->size(0) == B &&
                mask->size(1) == Lk,
                "attn_bwd: mask must be (B, Lk); expand broadcast masks "
                "host-side");
    mask_u8 = mask->to(at::kByte).contiguous();
  }

  auto stream = at::cuda::getCurrentHIPStream();
  TView qv = make_view(q), kvv = make_view(k), vv = make_view(v);
  TView dov = make_view(dout), outv = make_view(out);
  TViewMut dqv = make_view_mut(dq), dkv = make_view_mut(dk),
           dvv = make_view_mut(dv);

  if (!delta_in.has_value()) {
    const long rows = (long)B * H * Lq;
    const int block = 256;
    const long grid = (rows * 8 + block - 1) / block;
    hipLaunchKernelGGL(attn_delta_kernel, dim3(grid), dim3(block), 0, stream,
                       dov, outv, delta.data_ptr<float>(), H, Lq, rows);
  }

  dim3 grid_q((Lq + BQ - 1) / BQ, B * H);
  dim3 grid_k((Lk + BK - 1) / BK, B * H);

#define DISPATCH_DQ(HB, HM)                                                   \
  if (has_drop) DISPATCH_DQ_(HB, HM, true, dr);                               \
  else DISPATCH_DQ_(HB, HM, false, nd)
#define DISPATCH_DQ_(HB, HM, HD, DROP)                                        \
  hipLaunchKernelGGL((attn_bwd_dq_kernel<HB, HM, HD>), grid_q, dim3(256), 0,  \
      stream, qv, kvv, vv,                                                    \
      has_bias ? reinterpret_cast<const bf16_t*>(bias_c.data_ptr()) : nullptr,\
      has_mask ? mask_u8.data_ptr<unsigned char>() : nullptr,                 \
      dov, lse.data_ptr<float>(), delta.data_ptr<float>(), dqv,               \
      Lq, Lk, H, (int)bias_repeat, (int)q_repeat, (float)scale, DROP)

  // the stored-dS path forms dQ after dK/dV, from the scratch
  if (!use_ds) {
    if (has_bias && has_mask) { DISPATCH_DQ(true, true); }
    else if (has_bias) { DISPATCH_DQ(true, false); }
    else if (has_mask) { DISPATCH_DQ(false, true); }
    else { DISPATCH_DQ(false, false); }
  }
#undef DISPATCH_DQ
#undef DISPATCH_DQ_

  auto check_launch = [](const char* name) {
    const hipError_t err = hipGetLastError();
    TORCH_CHECK(err == hipSuccess, "attn_bwd: ", name, " launch failed: ",
                hipGetErrorString(err));
  };

  DsView dsv{nullptr, 0, 0, 0};
#define DISPATCH_DKV(HB, HM, DB)                                              \
  if (has_drop) DISPATCH_DKV_(HB, HM, DB, true, dr);                          \
  else DISPATCH_DKV_(HB, HM, DB, false, nd)
#define DISPATCH_DKV_(HB, HM, DB, HD, DROP)                                   \
  hipLaunchKernelGGL((attn_bwd_dkv_kernel<HB, HM, DB, HD>), grid_k,           \
      dim3(256), 0, stream, qv, kvv, vv,                                      \
      has_bias ? reinterpret_cast<const bf16_t*>(bias_c.data_ptr()) : nullptr,\
      has_mask ? mask_u8.data_ptr<unsigned char>() : nullptr,                 \
      dov, lse.data_ptr<float>(), delta.data_ptr<float>(), dkv, dvv,          \
      DB == DBIAS_ATOMIC ? dbias.data_ptr<float>() : nullptr,                 \
      dbias_chunks, DB == DBIAS_ATOMIC ? dbias.stride(0) : 0L, dsv,           \
      Lq, Lk, H, (int)bias_repeat, (int)q_repeat, (float)scale, DROP)

  if (use_ds) {
    // delta -> per slice: dK/dV (stores dS) -> dQ from dS -> dBias sum,
    // all on one stream, so a slice's scratch is consumed before the
    // next slice overwrites it.  Slices need not align to repeat groups:
    // the sum adds to groups an earlier slice started.
    const int R = (int)bias_repeat;
    const long HLL = (long)H * Lq * Lk;   // dbias elements of one group
    const long groups_cap = ((long)ds_slice + R - 1) / R + 1;
    // the fused kernel's 32-bit row offsets inside a tile
    const bool fused = groups_cap * HLL <= INT_MAX &&
        (long)BK * n_q * BQ <= INT_MAX && kvv.rs > 0 &&
        (long)BK * kvv.rs <= INT_MAX &&
        (dq_entries_per_block.has_value()
             ? epb_arg != 0 && n_k <= DQ_DBIAS_MAX_NKV
             : dq_dbias_fused_env && n_k <= 4);
#define DQ_DBIAS_FOR_NKV(DO)                                                  \
  switch (n_k) {                                                              \
    case 1: DO(1); break;                                                     \
    case 2: DO(2); break;                                                     \
    case 3: DO(3); break;                                                     \
    case 4: DO(4); break;                                                     \
    case 5: DO(5); break;                                                     \
    default: DO(6); break;                                                    \
  }
    const void* fused_kernel = nullptr;
#define DQ_DBIAS_PTR(NKV)                                                     \
  fused_kernel = reinterpret_cast<const void*>(&attn_bwd_dq_dbias_kernel<NKV>)
    DQ_DBIAS_FOR_NKV(DQ_DBIAS_PTR)
#undef DQ_DBIAS_PTR
    for (int b0 = 0; b0 < B; b0 += ds_slice) {
      const int b1 = std::min(B, b0 + ds_slice);
      dsv = DsView{reinterpret_cast<bf16_t*>(ds_buf.data_ptr()), ds_plane,
                   n_q * BQ, b0 * H};
      grid_k = dim3(n_k, (b1 - b0) * H);
      if (has_mask) { DISPATCH_DKV(true, true, DBIAS_STORE); }
      else { DISPATCH_DKV(true, false, DBIAS_STORE); }
      check_launch("attn_bwd_dkv_kernel");
      if (fused) {
        const int g0 = b0 / R, g1 = (b1 - 1) / R;
        const int ng = g1 - g0 + 1;
        const int span = std::min(R, b1 - b0);  // most entries of a group
        long epb = epb_arg;
        if (epb <= 0) {
          // as many chunks per group as keep the whole grid resident at
          // once: every block then does the same share of the work
          const long resident = colsum_grid(fused_kernel, 256,
                                            COLSUM_MAX_BLOCKS);
          const long chunks = std::max(1L, resident / ((long)n_q * ng * H));
          epb = (span + chunks - 1) / chunks;
        }
        epb = std::min<long>(std::max(1L, epb), span);
        const int nchunk = (int)((span + epb - 1) / epb);
        TORCH_CHECK(nchunk <= 65535 && (long)ng * H <= 65535,
                    "attn_bwd: dQ + dBias grid too large");
        const bool direct = nchunk == 1;
        const long C = (long)ng * HLL;
        at::Tensor part;
        float* sum_out = dbias.data_ptr<float>();
        if (!direct) {
          // every block stores its whole partial: no zero fill
          part = at::empty({nchunk, C}, dbias.options());
          sum_out = part.data_ptr<float>();
        }
#define LAUNCH_DQ_DBIAS(NKV)                                                  \
  hipLaunchKernelGGL((attn_bwd_dq_dbias_kernel<NKV>),                         \
                     dim3(n_q, ng * H, nchunk), dim3(256), 0, stream, dsv,    \
                     kvv, dqv, sum_out, direct ? 0L : C, Lq, Lk, H,           \
                     (float)scale, R, b0, b1, g0, (int)epb, direct ? 1 : 0,   \
                     b0 > 0 ? 1 : 0)
        DQ_DBIAS_FOR_NKV(LAUNCH_DQ_DBIAS)
#undef LAUNCH_DQ_DBIAS
        check_launch("attn_bwd_dq_dbias_kernel");
        if (!direct) {
          // chunks in order; the slice's first group is added to where
          // an earlier slice started it
          float* dst = dbias.data_ptr<float>() + (long)g0 * HLL;
          const bool cont = b0 > 0 && (long)g0 * R < b0;
          if (cont) {
            colsum_fold_launch(sum_out, dst, nchunk, HLL, true, stream,
                               false, C);
            if (ng > 1)
              colsum_fold_launch(sum_out + HLL, dst + HLL, nchunk, C - HLL,
                                 false, stream, false, C);
          } else {
            colsum_fold_launch(sum_out, dst, nchunk, C, false, stream);
          }
          check_launch("colsum_fold (dbias)");
        }
        continue;
      }
      hipLaunchKernelGGL(attn_bwd_dq_from_ds_kernel,
                         dim3(n_q, (b1 - b0) * H), dim3(256), 0, stream, dsv,
                         kvv, dqv, Lq, Lk, H, (float)scale);
      check_launch("attn_bwd_dq_from_ds_kernel");
      const int g0 = b0 / R, g1 = (b1 - 1) / R;
      hipLaunchKernelGGL(attn_dbias_sum_kernel,
                         dim3(n_q * n_k, (g1 - g0 + 1) * H), dim3(256), 0,
                         stream, dsv, dbias.data_ptr<float>(), Lq, Lk, H, R,
                         b0, b1, g0, b0 > 0 ? 1 : 0);
      check_launch("attn_dbias_sum_kernel");
    }
#undef DQ_DBIAS_FOR_NKV
    return {dq, dk, dv, dbias};
  }

#define DISPATCH_DV(HB, HM)                                                   \
  hipLaunchKernelGGL((attn_bwd_dv_kernel<HB, HM>), grid_k, dim3(256), 0,      \
      stream, qv, kvv,                                                        \
      has_bias ? reinterpret_cast<const bf16_t*>(bias_c.data_ptr()) : nullptr,\
      has_mask ? mask_u8.data_ptr<unsigned char>() : nullptr,                 \
      dov, lse.data_ptr<float>(), dvv,                                        \
      Lq, Lk, H, (int)bias_repeat, (int)q_repeat, (float)scale)

#define DISPATCH_DK(HB, HM, DB)                                               \
  hipLaunchKernelGGL((attn_bwd_dk_kernel<HB, HM, DB>), grid_k, dim3(256), 0,  \
      stream, qv, kvv, vv,                                                    \
      has_bias ? reinterpret_cast<const bf16_t*>(bias_c.data_ptr()) : nullptr,\
      has_mask ? mask_u8.data_ptr<unsigned char>() : nullptr,                 \
      dov, lse.data_ptr<float>(), delta.data_ptr<float>(), dkv,               \
      DB ? dbias.data_ptr<float>() : nullptr,                                 \
      dbias_chunks, need_dbias ? dbias.stride(0) : 0L,                        \
      Lq, Lk, H, (int)bias_repeat, (int)q_repeat, (float)scale)

  // the split kernels do not know dropout: with it, always combined
  if (split_dkv && !has_drop) {
    if (has_bias && has_mask) DISPATCH_DV(true, true);
    else if (has_bias) DISPATCH_DV(true, false);
    else if (has_mask) DISPATCH_DV(false, true);
    else DISPATCH_DV(false, false);
    if (need_dbias) {
      if (has_mask) DISPATCH_DK(true, true, true);
      else DISPATCH_DK(true, false, true);
    } else if (has_bias && has_mask) DISPATCH_DK(true, true, false);
    else if (has_bias) DISPATCH_DK(true, false, false);
    else if (has_mask) DISPATCH_DK(false, true, false);
    else DISPATCH_DK(false, false, false);
  } else {
    if (need_dbias) {
      if (has_mask) { DISPATCH_DKV(true, true, DBIAS_ATOMIC); }
      else { DISPATCH_DKV(true, false, DBIAS_ATOMIC); }
    } else if (has_bias && has_mask) { DISPATCH_DKV(true, true, DBIAS_NONE); }
    else if (has_bias) { DISPATCH_DKV(true, false, DBIAS_NONE); }
    else if (has_mask) { DISPATCH_DKV(false, true, DBIAS_NONE); }
    else { DISPATCH_DKV(false, false, DBIAS_NONE); }
  }
#undef DISPATCH_DKV
#undef DISPATCH_DKV_
#undef DISPATCH_DV
#undef DISPATCH_DK

  std::vector<at::Tensor> ret = {dq, dk, dv};
  if (need_dbias) ret.push_back(dbias.sum(0));
  return ret;
}
