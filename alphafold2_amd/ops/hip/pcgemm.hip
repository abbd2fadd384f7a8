// Per-channel batched GEMM — gfx950 MFMA (K3 + K4 of SURVEY.md §2.17).
//
//   C[b, m, n, d] = sum_k A[b, ., ., d] * B[b, ., ., d]
//
// with the m/k (resp. n/k) axes of A (resp. B) selected by ELEMENT
// STRIDES, so one kernel covers, without any permute copies:
//   * triangle multiplicative mix, outgoing and ingoing
//     (reference alphafold2.py:313: '... i k d, ... j k d -> ... i j d')
//   * outer-product mean accumulation (reference :341-349)
//   * all four backward products of the above (dL, dR by swapping
//     operand roles/strides)
//
// The d axis is innermost/contiguous in every tensor.  Three kernels:
//
//   pcgemm_line_kernel   the default wherever D is a multiple of 64: a
//                        block owns all 64 channels of a 128-byte line
//                        and a 32x32 output tile, so every operand load
//                        and every output store moves whole lines
//                        (design at the kernel).
//   pcgemm_kernel        any D that is a multiple of 8, and what
//                        AF2AMD_PCGEMM_V1=1 selects: a block owns an
//                        8-channel d-chunk and a 64x64 output tile (8
//                        waves, one channel per wave).  Staging loads 16
//                        bytes (8 channels) per (m, k) element — per-lane
//                        strided at D*2B, the sibling d-chunks of the
//                        same cacheline served by L2 — and scatters them
//                        into per-channel [64][32] LDS planes (+8 element
//                        row padding) with 2-byte stores; the C tile
//                        reuses the staging pool and drains as 16-byte
//                        d-contiguous global writes.
//   pcgemm_wide_kernel   pcgemm_kernel with 16-byte LDS stores, hoisted B
//                        fragments and register prefetch.  Bit-equal to
//                        it and measured 2-5 % SLOWER on every class
//                        (profiles/r08_pcgemm_ab.log): the 2-byte stores
//                        were not what the kernel waits for — its
//                        16-bytes-of-a-line loads are.  Kept for A/B,
//                        never the default (variant = 2).
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "common.h"

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef __bf16 pb16;

namespace {

constexpr int TM = 64, TN = 64, TK = 32, DC = 8;
constexpr int NTHREADS = 512;               // 8 waves; one d-channel each
constexpr int PLANE_ROW = TK + 8;           // padded row, elements
constexpr int PLANE = TM * PLANE_ROW;       // elements per channel plane

__global__ __launch_bounds__(NTHREADS, 2)
void pcgemm_kernel(const pb16* __restrict__ A, const pb16* __restrict__ B,
                   pb16* __restrict__ C,
                   int M, int N, int K, int D,
                   long a_bs, long a_ms, long a_ks,
                   long b_bs, long b_ns, long b_ks,
                   int ntiles, int mtiles, int swizzle, float alpha) {
  // a/b staging planes and the C drain buffer share one pool: the
  // C round-trip begins only after the K loop has consumed a/b
  __shared__ pb16 pool[2 * DC * PLANE > TM * TN * DC
                       ? 2 * DC * PLANE : TM * TN * DC];
  pb16* a_lds = pool;
  pb16* b_lds = pool + DC * PLANE;
  pb16* c_lds = pool;

  // logical work id L enumerates (batch, tile, chunk) with the d-chunk
  // fastest; the XCD swizzle places the 8 sibling chunks of a tile
  // (which share 128-byte cachelines of A/B/C) on ONE XCD's L2 —
  // without it each sibling re-fetches the same line into a different
  // XCD L2 (8x HBM/L3 traffic; MfmaUtil measured at 3%).
  // phys = (G%8) + 8*(m + 8*(G/8)) for L = 8G + m  (bijective when the
  // grid is a multiple of 64; identity otherwise).
  long L = (long)blockIdx.y * gridDim.x + blockIdx.x;
  if (swizzle) {
    const long phys = L;
    const long c = phys & 7;
    const long t = phys >> 3;
    const long m_ = t & 7;
    const long Ghi = t >> 3;
    L = ((Ghi << 3) + c) * 8 + m_;
  }
  const int dchunks = D / DC;
  const int chunk = L % dchunks;
  const long Lt = L / dchunks;
  const int tile = Lt % ((long)mtiles * ntiles);
  const int batch = Lt / ((long)mtiles * ntiles);
  const int mtile = tile / ntiles;
  const int ntile = tile - mtile * ntiles;
  const int m0 = mtile * TM, n0 = ntile * TN;
  const int d0 = chunk * DC;

  const pb16* Ab = A + (long)batch * a_bs + d0;
  const pb16* Bb_ = B + (long)batch * b_bs + d0;

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;   // = d channel within the chunk

  f32x4_t acc[4][4];  // [mt][nt] 16x16 fragments of the 64x64 tile
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = f32x4_t{0, 0, 0, 0};

  const int m_rows = min(TM, M - m0);
  const int n_rows = min(TN, N - n0);

  for (int k0 = 0; k0 < K; k0 += TK) {
    const int k_rows = min(TK, K - k0);
    __syncthreads();
    // stage A and B tiles: 64x32 (row, k) elements each, one 16-byte
    // 8-channel load per element, scattered into the 8 LDS planes
#pragma unroll
    for (int pass = 0; pass < 4; ++pass) {
      int idx = threadIdx.x + pass * NTHREADS;  // 0..2047
      int r = idx >> 5;                         // row in tile
      int kk = idx & 31;
      bf16x8_t av = {};
      bf16x8_t bv = {};
      if (r < m_rows && kk < k_rows) {
        av = *reinterpret_cast<const bf16x8_t*>(
            Ab + (long)(m0 + r) * a_ms + (long)(k0 + kk) * a_ks);
      }
      if (r < n_rows && kk < k_rows) {
        bv = *reinterpret_cast<const bf16x8_t*>(
            Bb_ + (long)(n0 + r) * b_ns + (long)(k0 + kk) * b_ks);
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        a_lds[j * PLANE + r * PLANE_ROW + kk] = av[j];
        b_lds[j * PLANE + r * PLANE_ROW + kk] = bv[j];
      }
    }
    __syncthreads();

    // MFMA: each wave owns one d channel of the full 64x64 tile
    const pb16* ap = a_lds + wave * PLANE;
    const pb16* bp = b_lds + wave * PLANE;
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      // A fragment: row = mt*16 + (lane&15), k = (lane>>4)*8 + j
      bf16x8_t af = *reinterpret_cast<const bf16x8_t*>(
          ap + (mt * 16 + (lane & 15)) * PLANE_ROW + ((lane >> 4) << 3));
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        bf16x8_t bf = *reinterpret_cast<const bf16x8_t*>(
            bp + (nt * 16 + (lane & 15)) * PLANE_ROW + ((lane >> 4) << 3));
        acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            af, bf, acc[mt][nt], 0, 0, 0);
      }
    }
    __builtin_amdgcn_s_setprio(0);
  }

  // C tile -> LDS in [m][n][d] layout, then 16B coalesced global writes
  __syncthreads();
  const int d = wave;
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int row = mt * 16 + (lane >> 4) * 4 + reg;
        const int col = nt * 16 + (lane & 15);
        c_lds[(row * TN + col) * DC + d] =
            (pb16)(acc[mt][nt][reg] * alpha);
      }
  __syncthreads();
  // 64*64 (m,n) cells * 16B = 4096 chunks; 8 per thread
  pb16* Cb = C + (((long)batch * M) * N) * D + d0;
#pragma unroll
  for (int pass = 0; pass < 8; ++pass) {
    int idx = threadIdx.x + pass * NTHREADS;
    int r = idx >> 6;
    int cc = idx & 63;
    if (r < m_rows && cc < n_rows) {
      *reinterpret_cast<bf16x8_t*>(
          Cb + ((long)(m0 + r) * N + (n0 + cc)) * D) =
          *reinterpret_cast<const bf16x8_t*>(c_lds + (r * TN + cc) * DC);
    }
  }
}

typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));

// Wide-store kernel.  Same tile, same LDS image, same fragment reads and
// the same ascending 32-wide MFMA k-steps as pcgemm_kernel (bit-equal
// results); what changes is how the operands reach LDS and when they are
// loaded:
//   * waves 0-3 stage A, waves 4-7 stage B.  A thread owns one tile row
//     (its lane) and 8 consecutive k (k-group = wave & 3): it loads the
//     eight 16-byte 8-channel pieces, transposes the 8(k) x 8(d) block in
//     registers (16-bit packs, no cross-lane traffic) and writes ONE
//     16-byte store per channel plane — 8 LDS stores per thread and
//     k-step where the scatter kernel issues 64 two-byte ones.  Lanes of
//     a store are consecutive rows at the 80-byte padded pitch, which is
//     conflict-free for the 8-lane groups of a 16-byte store.
//   * the loads of k-step t+1 are issued after the barrier that
//     publishes step t and complete behind its fragment reads and MFMAs
//     (32 VGPRs; the kernel stays at two blocks per CU, which LDS sets).
//   * the four B fragments are read once per k-step, not once per mt.
__global__ __launch_bounds__(NTHREADS, 2)
void pcgemm_wide_kernel(const pb16* __restrict__ A, const pb16* __restrict__ B,
                        pb16* __restrict__ C,
                        int M, int N, int K, int D,
                        long a_bs, long a_ms, long a_ks,
                        long b_bs, long b_ns, long b_ks,
                        int ntiles, int mtiles, int swizzle, float alpha) {
  __shared__ __attribute__((aligned(16)))
  pb16 pool[2 * DC * PLANE > TM * TN * DC ? 2 * DC * PLANE : TM * TN * DC];
  pb16* a_lds = pool;
  pb16* b_lds = pool + DC * PLANE;
  pb16* c_lds = pool;

  // work id -> (batch, tile, chunk): as pcgemm_kernel
  long L = (long)blockIdx.y * gridDim.x + blockIdx.x;
  if (swizzle) {
    const long phys = L;
    const long c = phys & 7;
    const long t = phys >> 3;
    const long m_ = t & 7;
    const long Ghi = t >> 3;
    L = ((Ghi << 3) + c) * 8 + m_;
  }
  const int dchunks = D / DC;
  const int chunk = L % dchunks;
  const long Lt = L / dchunks;
  const int tile = Lt % ((long)mtiles * ntiles);
  const int batch = Lt / ((long)mtiles * ntiles);
  const int mtile = tile / ntiles;
  const int ntile = tile - mtile * ntiles;
  const int m0 = mtile * TM, n0 = ntile * TN;
  const int d0 = chunk * DC;

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);

  const int m_rows = min(TM, M - m0);
  const int n_rows = min(TN, N - n0);

  // staging role of this wave.  Only the tile row differs between the
  // lanes of a load: its byte offset stays in one 32-bit VGPR (the host
  // checks that it fits) and everything else is a scalar base.  Rows
  // past the edge re-read the last valid row — they only reach C rows
  // or columns that are never written; k past the edge re-reads k = K-1
  // and is zeroed before it is stored.
  const bool stage_b = wave >= 4;
  const int kg = (wave & 3) * 8;       // first k of the group in the tile
  const int s_rows = stage_b ? n_rows : m_rows;
  const long s_rs = stage_b ? b_ns : a_ms;
  const long s_ks = stage_b ? b_ks : a_ks;
  const char* sbase = reinterpret_cast<const char*>(
      stage_b ? B + (long)batch * b_bs + (long)n0 * b_ns + d0
              : A + (long)batch * a_bs + (long)m0 * a_ms + d0);
  const unsigned int voff =
      (unsigned int)min(lane, s_rows - 1) * (unsigned int)s_rs * 2u;
  pb16* dst = (stage_b ? b_lds : a_lds) + lane * PLANE_ROW + kg;

  u32x4_t st[8];   // st[i] = channels 0..7 of (row, k0 + kg + i)
  auto stage_load = [&](int k0) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int k = min(k0 + kg + i, K - 1);
      st[i] = *reinterpret_cast<const u32x4_t*>(
          sbase + (long)k * s_ks * 2 + voff);
    }
  };

  f32x4_t acc[4][4];  // [mt][nt] 16x16 fragments of the 64x64 tile
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = f32x4_t{0, 0, 0, 0};

  stage_load(0);
  for (int k0 = 0; k0 < K; k0 += TK) {
    __syncthreads();   // the previous step's fragment reads are done
    if (k0 + TK > K) {
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if (k0 + kg + i >= K) st[i] = u32x4_t{0, 0, 0, 0};
    }
    // dword c of st[i] holds channels 2c (low half) and 2c+1 (high half);
    // plane 2c takes the low halves of k = 0..7, plane 2c+1 the high ones
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      u32x4_t lo, hi;
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const unsigned int x = st[2 * p][c], y = st[2 * p + 1][c];
        lo[p] = (x & 0xffffu) | (y << 16);
        hi[p] = (x >> 16) | (y & 0xffff0000u);
      }
      *reinterpret_cast<u32x4_t*>(dst + (2 * c) * PLANE) = lo;
      *reinterpret_cast<u32x4_t*>(dst + (2 * c + 1) * PLANE) = hi;
    }
    __syncthreads();
    if (k0 + TK < K) stage_load(k0 + TK);

    // MFMA: each wave owns one d channel of the full 64x64 tile
    const pb16* ap = a_lds + wave * PLANE;
    const pb16* bp = b_lds + wave * PLANE;
    const int frag = (lane & 15) * PLANE_ROW + ((lane >> 4) << 3);
    bf16x8_t bf[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
      bf[nt] = *reinterpret_cast<const bf16x8_t*>(
          bp + nt * 16 * PLANE_ROW + frag);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      // A fragment: row = mt*16 + (lane&15), k = (lane>>4)*8 + j
      bf16x8_t af = *reinterpret_cast<const bf16x8_t*>(
          ap + mt * 16 * PLANE_ROW + frag);
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
        acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            af, bf[nt], acc[mt][nt], 0, 0, 0);
    }
    __builtin_amdgcn_s_setprio(0);
  }

  // C tile -> LDS in [m][n][d] layout, then 16B coalesced global writes
  __syncthreads();
  const int d = wave;
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int row = mt * 16 + (lane >> 4) * 4 + reg;
        const int col = nt * 16 + (lane & 15);
        c_lds[(row * TN + col) * DC + d] =
            (pb16)(acc[mt][nt][reg] * alpha);
      }
  __syncthreads();
  pb16* Cb = C + (((long)batch * M) * N) * D + d0;
#pragma unroll
  for (int pass = 0; pass < 8; ++pass) {
    int idx = threadIdx.x + pass * NTHREADS;
    int r = idx >> 6;
    int cc = idx & 63;
    if (r < m_rows && cc < n_rows) {
      *reinterpret_cast<bf16x8_t*>(
          Cb + ((long)(m0 + r) * N + (n0 + cc)) * D) =
          *reinterpret_cast<const bf16x8_t*>(c_lds + (r * TN + cc) * DC);
    }
  }
}

// ---------------------------------------------------------------------------
// Full-line kernel (D a multiple of 64).
//
// Both kernels above give a block 8 channels, so every (row, k) element
// it loads is a 16-byte piece of a 128-byte line whose other pieces
// belong to seven sibling blocks on other CUs: each line crosses the
// L2 -> L1 path eight times per pass, one request per 16 bytes.  Here a
// block owns ALL 64 channels of a line and a 32x32 output tile:
//   * 16 waves.  Per 16-wide k-step a thread loads the 8-channel pieces
//     of 8 consecutive k of one (row, chunk); the 8 lanes lane & 7 are
//     the 8 chunks of one line, so a load instruction reads 8 whole
//     lines.  The 8(k) x 8(d) block is transposed in registers and
//     written with one 16-byte store per channel plane.
//   * LDS holds 64 channel planes of [A rows 0..31 | B rows 32..63][16 k]
//     (32-byte rows, 128 KiB): planes of chunk c are skewed by 16c bytes
//     (the 8 lanes of a store group then hit 8 different 16-byte slots),
//     and the four 8-byte k quads of row r sit at quad ^ ((r >> 2) & 3)
//     (the 16 rows of a fragment read then cover all 32 banks once).
//   * wave w multiplies channels 4w..4w+3: per channel 2 + 2 fragment
//     reads of 8 bytes and 4 v_mfma_f32_16x16x16_bf16.  k ascends in
//     16-wide steps, so results differ from the 32-wide kernels in the
//     last fp32 bits of the sum (not bit-equal to them).
//   * the loads of step t+1 are in flight behind the MFMAs of step t.
//   * C leaves through LDS as [cell][64 d] with the 16-byte slots of a
//     cell rotated by the cell index, and is stored as whole lines.
// A tile is smaller than the 64x64 of the other kernels (operands are
// re-read 8 times instead of 4), but every re-read moves whole lines.
constexpr int LT = 32, LK = 16, LDCH = 64;   // tile, k-step, channels
constexpr int LTHREADS = 1024;
constexpr int LPLANE = 2 * LT * LK;          // elements per channel plane
constexpr int LPOOL = LDCH * LPLANE + 8 * 8; // + the chunk skew

typedef short s16x4_t __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2_t __attribute__((ext_vector_type(2)));

__device__ __forceinline__ unsigned int pack_bf16x2(float lo, float hi) {
  union { pb16 h[2]; unsigned int u; } v;
  v.h[0] = (pb16)lo;
  v.h[1] = (pb16)hi;
  return v.u;
}

__global__ __launch_bounds__(LTHREADS)
void pcgemm_line_kernel(const pb16* __restrict__ A, const pb16* __restrict__ B,
                        pb16* __restrict__ C,
                        int M, int N, int K, int D,
                        long a_bs, long a_ms, long a_ks,
                        long b_bs, long b_ns, long b_ks,
                        int ntiles, int mtiles, float alpha) {
  __shared__ __attribute__((aligned(16))) pb16 pool[LPOOL];

  // Blocks with id % 8 equal share an XCD's L2 (observed placement, a
  // speed matter only).  Give each of the 8 groups a contiguous range of
  // logical ids — ntile fastest, then mtile, then (batch, channel group)
  // — so that the blocks resident together on an XCD are neighbouring
  // tiles of one problem and re-read each other's operand lines from L2.
  long L;
  {
    const long nwg = gridDim.x, phys = blockIdx.x;
    const long q = nwg >> 3, r = nwg & 7, xcd = phys & 7;
    L = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (phys >> 3);
  }
  const int ntile = L % ntiles;
  const long L1 = L / ntiles;
  const int mtile = L1 % mtiles;
  const long L2 = L1 / mtiles;
  const int cgroups = D / LDCH;
  const int cgroup = L2 % cgroups;
  const int batch = L2 / cgroups;
  const int m0 = mtile * LT, n0 = ntile * LT;
  const int d0 = cgroup * LDCH;
  const int m_rows = min(LT, M - m0);
  const int n_rows = min(LT, N - n0);

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);

  // staging role: waves 0-7 stage A, 8-15 B; (wave >> 2) & 1 is the
  // 8-wide k group; a wave covers 8 tile rows x 8 chunks.  Rows past the
  // edge re-read the last valid row (they only reach C cells that are
  // never stored); k past the edge re-reads k = K-1 and is zeroed.
  const bool stage_b = wave >= 8;
  const int kg = ((wave >> 2) & 1) * 8;
  const int srow = (wave & 3) * 8 + (lane >> 3);
  const int chunk = lane & 7;
  const int s_rows = stage_b ? n_rows : m_rows;
  const long s_rs = stage_b ? b_ns : a_ms;
  const long s_ks = stage_b ? b_ks : a_ks;
  const char* sbase = reinterpret_cast<const char*>(
      stage_b ? B + (long)batch * b_bs + (long)n0 * b_ns + d0
              : A + (long)batch * a_bs + (long)m0 * a_ms + d0);
  const unsigned int voff =
      (unsigned int)min(srow, s_rows - 1) * (unsigned int)s_rs * 2u +
      (unsigned int)chunk * 16u;
  // plane 8*chunk + j, row (B rows after the 32 A rows); the four
  // 8-byte k quads of a row sit at quad ^ ((row >> 2) & 3): the 16-byte
  // half moves with bit 1 of that, its two quads swap with bit 0
  const int sw = (srow >> 2) & 3;
  const bool swap_quads = sw & 1;
  pb16* dst = pool + (8 * chunk) * LPLANE + 8 * chunk +
              ((stage_b ? LT : 0) + srow) * LK + (kg ^ ((sw >> 1) * 8));

  u32x4_t st[8];   // st[i] = channels 8*chunk.. of (row, k0 + kg + i)
  auto stage_load = [&](int k0) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int k = min(k0 + kg + i, K - 1);
      st[i] = *reinterpret_cast<const u32x4_t*>(
          sbase + (long)k * s_ks * 2 + voff);
    }
  };

  f32x4_t acc[4][2][2];   // [channel][mt][nt] 16x16 fragments
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) acc[c][mt][nt] = f32x4_t{0, 0, 0, 0};

  // fragment of 16x16x16: row = lane & 15, k = 4 * (lane >> 4) + j
  const int fr = lane & 15, fq = lane >> 4;
  const int frag = fr * LK + ((fq ^ ((fr >> 2) & 3)) << 2);

  stage_load(0);
  for (int k0 = 0; k0 < K; k0 += LK) {
    __syncthreads();   // the previous step's fragment reads are done
    if (k0 + LK > K) {
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if (k0 + kg + i >= K) st[i] = u32x4_t{0, 0, 0, 0};
    }
    // dword c of st[i] holds channels 2c (low half) and 2c+1 (high half)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      u32x4_t lo, hi;
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const unsigned int x = st[2 * p][c], y = st[2 * p + 1][c];
        lo[p] = (x & 0xffffu) | (y << 16);
        hi[p] = (x >> 16) | (y & 0xffff0000u);
      }
      if (swap_quads) {
        lo = u32x4_t{lo[2], lo[3], lo[0], lo[1]};
        hi = u32x4_t{hi[2], hi[3], hi[0], hi[1]};
      }
      *reinterpret_cast<u32x4_t*>(dst + (2 * c) * LPLANE) = lo;
      *reinterpret_cast<u32x4_t*>(dst + (2 * c + 1) * LPLANE) = hi;
    }
    __syncthreads();
    if (k0 + LK < K) stage_load(k0 + LK);

    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int p = 4 * wave + c;
      const pb16* pl = pool + p * LPLANE + 8 * (p >> 3) + frag;
      s16x4_t af[2], bf[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        af[t] = *reinterpret_cast<const s16x4_t*>(pl + t * 16 * LK);
        bf[t] = *reinterpret_cast<const s16x4_t*>(pl + (LT + t * 16) * LK);
      }
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
          acc[c][mt][nt] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(
              af[mt], bf[nt], acc[c][mt][nt], 0, 0, 0);
    }
    __builtin_amdgcn_s_setprio(0);
  }

  // C tile -> LDS as [cell = m*32 + n][64 d]; the eight 16-byte slots of
  // a cell are rotated by the cell index (a wave's 16 lanes of a store
  // are 16 consecutive cells at one channel offset)
  __syncthreads();
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int cell = (mt * 16 + fq * 4 + reg) * LT + nt * 16 + fr;
        const int slot = ((wave >> 1) + cell) & 7;
        u32x2_t v;
        v[0] = pack_bf16x2(acc[0][mt][nt][reg] * alpha,
                           acc[1][mt][nt][reg] * alpha);
        v[1] = pack_bf16x2(acc[2][mt][nt][reg] * alpha,
                           acc[3][mt][nt][reg] * alpha);
        *reinterpret_cast<u32x2_t*>(
            pool + cell * LDCH + slot * 8 + (wave & 1) * 4) = v;
      }
  __syncthreads();
  // 1024 cells x 8 chunks; the 8 lanes lane & 7 store one whole line
  pb16* Cb = C + (((long)batch * M) * N) * D + d0;
#pragma unroll
  for (int pass = 0; pass < 8; ++pass) {
    const int cell = pass * 128 + (threadIdx.x >> 3);
    const int r = cell >> 5, cc = cell & 31;
    if (r < m_rows && cc < n_rows) {
      *reinterpret_cast<u32x4_t*>(
          Cb + ((long)(m0 + r) * N + (n0 + cc)) * D + chunk * 8) =
          *reinterpret_cast<const u32x4_t*>(
              pool + cell * LDCH + ((chunk + cell) & 7) * 8);
    }
  }
}

}  // namespace

// C (Bb, M, N, D) bf16 = alpha * sum_k A*B per channel; strides in elements.
// variant: 1 = scatter-staging kernel, 2 = wide-store kernel, 3 = full-line
// kernel, 0 = the default (full-line where D % 64 == 0 unless
// AF2AMD_PCGEMM_V1=1, else scatter-staging).
at::Tensor pcgemm(at::Tensor A, at::Tensor B, long Bb, long M, long N,
                  long K, long D,
                  long a_bs, long a_ms, long a_ks,
                  long b_bs, long b_ns, long b_ks, double alpha,
                  long variant) {
  TORCH_CHECK(A.scalar_type() == at::kBFloat16 &&
              B.scalar_type() == at::kBFloat16, "pcgemm: bf16 only");
  TORCH_CHECK(Bb >= 0 && M >= 0 && N >= 0 && K >= 0 && D >= 0 &&
              M <= INT_MAX && N <= INT_MAX && K <= INT_MAX && D <= INT_MAX,
              "pcgemm: M, N, K, D must fit int, got ", M, ", ", N, ", ", K,
              ", ", D);
  TORCH_CHECK(D % DC == 0, "pcgemm: D must be a multiple of 8");
  // the kernels move 8-channel vectors as 16-byte accesses
  for (const long s : {a_bs, a_ms, a_ks, b_bs, b_ns, b_ks})
    TORCH_CHECK(s % DC == 0, "pcgemm: every stride must be a multiple of 8 "
                "elements, got ", s);
  TORCH_CHECK(reinterpret_cast<uintptr_t>(A.data_ptr()) % 16 == 0 &&
              reinterpret_cast<uintptr_t>(B.data_ptr()) % 16 == 0,
              "pcgemm: operands must be 16-byte aligned");
  static const bool force_v1 = [] {
    const char* e = getenv("AF2AMD_PCGEMM_V1");
    return e != nullptr && e[0] == '1';
  }();
  // the wide-store and full-line kernels keep a row's byte offset inside
  // its tile in 32 bits and clamp k to K - 1; what they cannot hold goes
  // to the scatter kernel
  const long max_rs = (long)(0xffffffffu / (2 * TM));
  const bool fits = a_ms >= 0 && b_ns >= 0 && a_ms <= max_rs &&
                    b_ns <= max_rs && K > 0;
  TORCH_CHECK(variant >= 0 && variant <= 3, "pcgemm: variant ", variant);
  TORCH_CHECK(variant != 3 || (D % LDCH == 0 && fits),
              "pcgemm: the full-line kernel needs D % 64 == 0");
  // default: full lines where D allows, else the scatter kernel (the
  // wide-store kernel measured no faster: docs/ROADMAP.md, round 8)
  int kind = variant;
  if (kind == 0) kind = (!force_v1 && fits && D % LDCH == 0) ? 3 : 1;
  if (kind == 2 && !fits) kind = 1;

  auto C = at::empty({Bb, M, N, D}, A.options());
  if (C.numel() == 0) return C;
  auto stream = at::cuda::getCurrentHIPStream();
  const pb16* Ap = reinterpret_cast<const pb16*>(A.data_ptr());
  const pb16* Bp = reinterpret_cast<const pb16*>(B.data_ptr());
  pb16* Cp = reinterpret_cast<pb16*>(C.data_ptr());
  if (kind == 3) {
    const int mtiles = (M + LT - 1) / LT;
    const int ntiles = (N + LT - 1) / LT;
    const long nblocks = (long)mtiles * ntiles * Bb * (D / LDCH);
    TORCH_CHECK(nblocks <= INT_MAX, "pcgemm: grid too large (", nblocks, ")");
    hipLaunchKernelGGL(pcgemm_line_kernel, dim3((unsigned int)nblocks),
                       dim3(LTHREADS), 0, stream, Ap, Bp, Cp,
                       (int)M, (int)N, (int)K, (int)D,
                       a_bs, a_ms, a_ks, b_bs, b_ns, b_ks,
                       ntiles, mtiles, (float)alpha);
  } else {
    const int mtiles = (M + TM - 1) / TM;
    const int ntiles = (N + TN - 1) / TN;
    const long nblocks = (long)mtiles * ntiles * Bb * (D / DC);
    TORCH_CHECK((long)mtiles * ntiles <= INT_MAX && Bb * (D / DC) <= 65535,
                "pcgemm: grid too large (", (long)mtiles * ntiles, " x ",
                Bb * (D / DC), ")");
    const int swizzle = (D / DC) % 8 == 0 && nblocks % 64 == 0;
    dim3 grid(mtiles * ntiles, Bb * (D / DC));
    const auto kernel = kind == 1 ? pcgemm_kernel : pcgemm_wide_kernel;
    hipLaunchKernelGGL(kernel, grid, dim3(NTHREADS), 0, stream, Ap, Bp, Cp,
                       (int)M, (int)N, (int)K, (int)D,
                       a_bs, a_ms, a_ks, b_bs, b_ns, b_ks,
                       ntiles, mtiles, swizzle, (float)alpha);
  }
  const hipError_t err = hipGetLastError();
  TORCH_CHECK(err == hipSuccess, "pcgemm: launch failed: ",
              hipGetErrorString(err));
  return C;
}
