// Split-K weight-gradient GEMM — gfx950 MFMA.
//
//   dW[m, n] = sum_k A[k, m] * B[k, n]      (A = dY, B = X activations)
//
// The Evoformer's wgrads reduce over K = b*m*n up to ~330k rows into
// tiny (M x N) outputs: the work is one pass over dY and X, so the
// kernel to beat is the HBM stream, not the MFMA rate.  Two kernels:
//
//   wgrad_stream_kernel  the default (r09).  Both operands go to LDS
//                        k-major, exactly as they lie in memory, with
//                        16-byte stores, and both MFMA operands come
//                        back through the transposing LDS read; LDS is
//                        double buffered (one barrier per 32-row K
//                        step) with two steps of global loads in
//                        flight.  A block owns one 256x256 output tile
//                        and one contiguous K slot and writes its
//                        partial whole with plain stores; a fixed-order
//                        fold sums the slots.  No atomics, no zero
//                        fill: dW is the same on every run.  The blocks
//                        of the first column tile can also form the
//                        column sum of dY (the Linear's bias gradient)
//                        with one extra MFMA per fragment and K step.
//                        Design at the kernel.
//   wgrad_kernel         r02, what AF2AMD_WGRAD_V1=1 selects: 128x128
//                        tiles transposed on the way INTO LDS with
//                        2-byte stores, two barriers per step, fp32
//                        atomic drain into a zero-filled dW.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <climits>
#include <cstdint>
#include <cstdlib>

#include "colsum.h"
#include "common.h"

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef short s16x4_t __attribute__((ext_vector_type(4)));
typedef short s16x8_t __attribute__((ext_vector_type(8)));
typedef __bf16 pb16;

namespace {

constexpr int WM = 128;        // dW rows per block (A columns)
constexpr int WN = 128;        // dW cols per block (B columns)
constexpr int KS = 64;         // k rows staged per iteration
constexpr int NT = 256;        // 4 waves; wave w owns rows [w*32, w*32+32)

// LDS tiles hold the operands TRANSPOSED: [m_or_n][k], padded rows
constexpr int PR = KS + 8;

__global__ __launch_bounds__(NT, 2)
void wgrad_kernel(const pb16* __restrict__ A, const pb16* __restrict__ B,
                  float* __restrict__ dW,
                  long K, int M, int N, long k_per_block,
                  int mtiles, int ntiles) {
  __shared__ pb16 a_lds[WM * PR];
  __shared__ pb16 b_lds[WN * PR];

  const int tile = blockIdx.x;
  const int kslot = blockIdx.y;
  const int mtile = tile / ntiles;
  const int ntile = tile - mtile * ntiles;
  const int m0 = mtile * WM;
  const int n0 = ntile * WN;
  const long k0 = (long)kslot * k_per_block;
  const long k1 = min(K, k0 + k_per_block);
  const int m_cols = min(WM, M - m0);
  const int n_cols = min(WN, N - n0);

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int wr = wave * 32;

  f32x4_t acc[2][8];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int nt = 0; nt < 8; ++nt) acc[mt][nt] = f32x4_t{0, 0, 0, 0};

  for (long ks = k0; ks < k1; ks += KS) {
    const int k_rows = min((long)KS, k1 - ks);
    __syncthreads();
    // stage 64 k-rows of A (WM cols) and B (WN cols) transposed:
    // thread loads 8 consecutive columns of one k-row (16-byte,
    // coalesced along the tensor row) and scatters them into 8 LDS
    // rows at column k.  1024 chunks per operand = 4 per thread.
#pragma unroll
    for (int pass = 0; pass < 4; ++pass) {
      const int idx = threadIdx.x + pass * NT;
      const int kk = idx >> 4;              // k row within the slab
      const int c8 = (idx & 15) << 3;       // first of 8 source columns
      bf16x8_t av = {};
      if (kk < k_rows && c8 < m_cols)
        av = *reinterpret_cast<const bf16x8_t*>(
            A + (ks + kk) * (long)M + m0 + c8);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        a_lds[(c8 + j) * PR + kk] = av[j];

      bf16x8_t bv = {};
      if (kk < k_rows && c8 < n_cols)
        bv = *reinterpret_cast<const bf16x8_t*>(
            B + (ks + kk) * (long)N + n0 + c8);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        b_lds[(c8 + j) * PR + kk] = bv[j];
    }
    __syncthreads();

    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int koff = kk * 32 + ((lane >> 4) << 3);
      bf16x8_t af0 = *reinterpret_cast<const bf16x8_t*>(
          a_lds + (wr + (lane & 15)) * PR + koff);
      bf16x8_t af1 = *reinterpret_cast<const bf16x8_t*>(
          a_lds + (wr + 16 + (lane & 15)) * PR + koff);
#pragma unroll
      for (int nt = 0; nt < 8; ++nt) {
        bf16x8_t bf = *reinterpret_cast<const bf16x8_t*>(
            b_lds + (nt * 16 + (lane & 15)) * PR + koff);
        acc[0][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            af0, bf, acc[0][nt], 0, 0, 0);
        acc[1][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            af1, bf, acc[1][nt], 0, 0, 0);
      }
    }
    __builtin_amdgcn_s_setprio(0);
  }

  // drain: fp32 atomics (one partial per k-slot); C/D frag col=lane&15,
  // row=(lane>>4)*4+reg
  const int fcol = lane & 15;
  const int frow = (lane >> 4) << 2;
  const bool single = gridDim.y == 1;
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int nt = 0; nt < 8; ++nt)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int row = wr + mt * 16 + frow + reg;
        const int col = nt * 16 + fcol;
        if (row < m_cols && col < n_cols) {
          float* addr = dW + (long)(m0 + row) * N + n0 + col;
          if (single) *addr = acc[mt][nt][reg];
          else atomicAdd(addr, acc[mt][nt][reg]);
        }
      }
}


// ---------------------------------------------------------------------------
// r09 streaming kernel.
//
// Tile.  A block owns a 256 (dW rows, dY columns) x 256 (dW columns, X
// columns) output tile and one contiguous K slot; 8 waves, wave (wm, wn)
// = (wave >> 1, wave & 1) owns 64 x 128 of it: 4 x 8 MFMA 16x16x32
// accumulators, 128 registers per lane.  K advances 32 rows per step.
// Per step a block reads 32 KB from global memory and issues 256 MFMAs
// (4096 MFMA cycles over 4 SIMDs = 1024 per SIMD) against ~3300 cycles
// of HBM time for 32 KB at 1/256 of 6 TB/s: the kernel waits on memory.
//
// LDS image.  Each operand step is a [32 k rows][256 columns] bf16 tile
// with 512-byte rows, stored as it lies in memory: thread t stores the
// 16-byte chunk (t & 31) of row (t >> 5) (+16).  Byte offset of column
// byte c of row r:
//     r * 512 + (c ^ (f(r) << 5)),   f(r) = (r & 3) | ((r >> 3) & 1) << 2
// i.e. the eight 32-byte pieces of every 256-byte half row are permuted
// by f(r); 16-byte chunks and the 8-byte pieces of the transposing read
// stay whole.  The transposing read (ds_read_b64_tr_b16) serves a
// 16-lane group 4 rows x 32 bytes; the two groups of a 32-lane half
// read rows {8g + q} and {8(g+1) + q}, q = 0..3, at ONE column piece:
// eight rows whose f(r) are the eight values 0..7, so the eight 32-byte
// pieces fall into the eight distinct 8-bank groups of the 64 banks —
// conflict-free by the bank rule (bank = (addr / 4) % 64, conflicts
// counted per 32-lane half).  The second read of a fragment is 4 rows
// further on (f(r + 4) == f(r) for these r).  The 16-byte stores of a
// wave cover two whole rows, every bank equally.
//
// MFMA roles.  D[n][m] = sum_k X[k][n] dY[k][m]: X is the A operand, dY
// the B operand, so a lane ends with 4 consecutive n of one m — one
// 16-byte store into row-major dW.  Both fragments are lane (i = lane &
// 15) = column, k = (lane >> 4) * 8 + j = tile row, which is what the
// transposing read delivers (frag_tr of attention.hip).
//
// Transposing-read rules.  The reads sit outside every divergent
// branch (EXEC all ones), every lane's address is 8-byte aligned and
// inside the 16 KB tile, and whatever the problem does not cover — k
// rows past the slot's end, columns past M or N — is stored as zeros.
// Only whole wave tiles outside M or N are skipped, by a wave-uniform
// (scalar) branch.
//
// Pipeline.  Two register stages (32 registers): step t + 2 is loaded
// right after the barrier of step t and stored to LDS two steps later,
// so two steps (64 KB per CU) of loads are in flight during the MFMAs.
// One barrier per step: the buffer a step stores was last read two
// steps ago, before the previous barrier.
//
// Column sum.  With CS, the wn == 0 waves of the first column tile add
// MFMA(ones, dY fragment): every row of that 16x16 result is the fp32
// column sum of the 32 bf16 rows.  It lands behind the M * N tile
// elements of the block's partial row and folds with them.
//
// Grid.  One dimension; consecutive block ids go round the 8 XCDs, and
// xcd_logical() gives each XCD a contiguous range of logical ids =
// slot * tiles + tile, so the tiles of one K slab share an L2 (for
// every slab when tiles divides the per-XCD share, else for all but
// those straddling two ranges).  Placement changes nothing in the result.

constexpr int TM = 256;            // dW rows (dY columns) per block
constexpr int TN = 256;            // dW columns (X columns) per block
constexpr int SK = 32;             // k rows per step
constexpr int SNT = 512;           // 8 waves
constexpr int SROWB = TM * 2;      // bytes per LDS row
constexpr int STILEB = SK * SROWB; // 16 KB per operand and step
constexpr long PART_CAP_BYTES = 64l << 20;

static_assert(TM == TN, "one staging pattern for both operands");

__device__ __forceinline__ int simg(int row, int colb) {
  return row * SROWB + (colb ^ (((row & 3) | ((row >> 1) & 4)) << 5));
}

// fragment of 16 columns from col0 of a staged tile: lane i = column,
// k = tile row (lane >> 4) * 8 + j.  EXEC must be full.
__device__ __forceinline__ bf16x8_t sfrag_tr(const char* tile, int col0) {
  typedef __attribute__((address_space(3))) s16x4_t* lds_ptr;
  const int lane = threadIdx.x & 63;
  const int i = lane & 15;
  const int row = ((lane >> 4) << 3) + (i >> 2);
  const int colb = (col0 + ((i & 3) << 2)) * 2;
  const char* p = tile + simg(row, colb);
  const s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)p);
  const s16x4_t hi =
      __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(p + 4 * SROWB));
  return __builtin_bit_cast(
      bf16x8_t,
      (s16x8_t)__builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

// bijective: physical block id -> logical id, each XCD a contiguous range
__device__ __forceinline__ long wg_xcd_logical(long phys, long nwg) {
  if (nwg < 16) return phys;
  const long q = nwg >> 3, r = nwg & 7;
  const long xcd = phys & 7, idx = phys >> 3;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

struct SStage {
  uint4 a[2], b[2];
};

template <bool CS>
__global__ __launch_bounds__(SNT)
void wgrad_stream_kernel(const pb16* __restrict__ dY,
                         const pb16* __restrict__ X,
                         float* __restrict__ part,
                         long K, int M, int N, long k_per_slot,
                         int ntiles, int tiles, long nwg, long part_stride) {
  __shared__ __attribute__((aligned(16))) char lds[2][2][STILEB];

  const long L = wg_xcd_logical((long)blockIdx.x, nwg);
  const long slot = L / tiles;
  const int tile = (int)(L - slot * tiles);
  const int mtile = tile / ntiles;
  const int ntile = tile - mtile * ntiles;
  const int m0 = mtile * TM;
  const int n0 = ntile * TN;
  const long k0 = slot * k_per_slot;
  const long k1 = min(K, k0 + k_per_slot);
  const int nsteps = (int)((k1 - k0 + SK - 1) / SK);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  // in an SGPR, so that what follows from it branches on the scalar unit
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1;
  const int wn = wave & 1;

  // does the wave tile reach into M x N (wave-uniform)
  const bool wave_on = m0 + wm * 64 < M && n0 + wn * 128 < N;
  const bool do_cs = CS && ntile == 0 && wn == 0 && wave_on;

  // staging: chunk ch of tile rows r0 and r0 + 16.  Every load is
  // issued unconditionally and nothing looks at its result before the
  // LDS store two steps later, so the wait there is for the older stage
  // alone: a chunk past M / N reads chunk 0 of its row and a row past
  // the slot's end reads the slot's last row (both inside the operand),
  // and the store masks what came to zeros.
  const int ch = tid & 31;
  const int r0 = tid >> 5;
  const unsigned a_mask = m0 + ch * 8 < M ? 0xffffffffu : 0u;
  const unsigned b_mask = n0 + ch * 8 < N ? 0xffffffffu : 0u;
  const pb16* a_src = dY + m0 + (a_mask ? ch * 8 : 0);
  const pb16* b_src = X + n0 + (b_mask ? ch * 8 : 0);
  const int st_off = simg(r0, ch * 16);   // simg(r0 + 16, .) = + 16 rows

  auto load = [&](SStage& s, int step) {
    const long kr = k0 + (long)step * SK + r0;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const long row = min(kr + p * 16, k1 - 1);
      s.a[p] = *reinterpret_cast<const uint4*>(a_src + row * M);
      s.b[p] = *reinterpret_cast<const uint4*>(b_src + row * N);
    }
  };
  auto masked = [](uint4 v, unsigned m) {
    return uint4{v.x & m, v.y & m, v.z & m, v.w & m};
  };
  auto store = [&](const SStage& s, int buf, int step) {
    const long kr = k0 + (long)step * SK + r0;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const unsigned row_mask = kr + p * 16 < k1 ? 0xffffffffu : 0u;
      *reinterpret_cast<uint4*>(lds[buf][0] + st_off + p * 16 * SROWB) =
          masked(s.a[p], a_mask & row_mask);
      *reinterpret_cast<uint4*>(lds[buf][1] + st_off + p * 16 * SROWB) =
          masked(s.b[p], b_mask & row_mask);
    }
  };

  f32x4_t acc[8][4];
#pragma unroll
  for (int nf = 0; nf < 8; ++nf)
#pragma unroll
    for (int mf = 0; mf < 4; ++mf) acc[nf][mf] = f32x4_t{0, 0, 0, 0};
  f32x4_t cs[4];
#pragma unroll
  for (int mf = 0; mf < 4; ++mf) cs[mf] = f32x4_t{0, 0, 0, 0};

  bf16x8_t ones;
#pragma unroll
  for (int j = 0; j < 8; ++j) ones[j] = (__bf16)1.0f;

  // A wave tile with nothing inside M x N is skipped whole; one that is
  // partly inside runs all its MFMAs, on the zeros LDS holds there.
  auto compute = [&](int buf) {
    if (!wave_on) return;
    const char* yl = lds[buf][0];
    const char* xl = lds[buf][1];
    bf16x8_t yf[4];
#pragma unroll
    for (int mf = 0; mf < 4; ++mf) yf[mf] = sfrag_tr(yl, wm * 64 + mf * 16);
    if (CS && do_cs) {
#pragma unroll
      for (int mf = 0; mf < 4; ++mf)
        cs[mf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            ones, yf[mf], cs[mf], 0, 0, 0);
    }
#pragma unroll
    for (int nf = 0; nf < 8; ++nf) {
      const bf16x8_t xf = sfrag_tr(xl, wn * 128 + nf * 16);
#pragma unroll
      for (int mf = 0; mf < 4; ++mf)
        acc[nf][mf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            xf, yf[mf], acc[nf][mf], 0, 0, 0);
    }
  };

  // s0 strictly before s1, as in the loop: the wait in front of a store
  // then counts the younger stage's four loads and leaves them in flight
  SStage s0, s1;
  load(s0, 0);
  __builtin_amdgcn_sched_barrier(0);
  load(s1, 1);
  __builtin_amdgcn_sched_barrier(0);
  for (int t = 0; t < nsteps; t += 2) {
    store(s0, 0, t);
    __syncthreads();
    load(s0, t + 2);
    compute(0);
    // with an odd step count the last half stages zeros: one straight
    // loop body keeps the wait counts in front of the stores exact
    store(s1, 1, t + 1);
    __syncthreads();
    load(s1, t + 3);
    compute(1);
  }

  // the block's partial, whole: lane holds n = 4 * (lane >> 4) + 0..3 of
  // m = lane & 15 in every fragment
  float* prow = part + slot * part_stride;
  const int fm = lane & 15;
  const int fn = (lane >> 4) << 2;
#pragma unroll
  for (int nf = 0; nf < 8; ++nf)
#pragma unroll
    for (int mf = 0; mf < 4; ++mf) {
      const int m = m0 + wm * 64 + mf * 16 + fm;
      const int n = n0 + wn * 128 + nf * 16 + fn;
      if (m < M && n < N)
        *reinterpret_cast<f32x4_t*>(prow + (long)m * N + n) = acc[nf][mf];
    }
  if (CS && do_cs && lane < 16) {
#pragma unroll
    for (int mf = 0; mf < 4; ++mf) {
      const int m = m0 + wm * 64 + mf * 16 + fm;
      if (m < M) prow[(long)M * N + m] = cs[mf][0];
    }
  }
}

// dW (M, N) fp32 = dY^T @ X, and with want_cs the fp32 column sum (M,) of
// dY, both views of one buffer.
std::vector<at::Tensor> wgrad_stream(const at::Tensor& dY,
                                     const at::Tensor& X, bool want_cs) {
  const long K = dY.size(0);
  const int M = dY.size(1);
  const int N = X.size(1);
  const long MN = (long)M * N;
  const long rowlen = MN + (want_cs ? M : 0);
  TORCH_CHECK(rowlen <= INT_MAX, "wgrad: M * N too large (", M, " x ", N,
              ")");
  const int mtiles = (M + TM - 1) / TM;
  const int ntiles = (N + TN - 1) / TN;
  const long tiles = (long)mtiles * ntiles;

  const void* kernel = want_cs
      ? reinterpret_cast<const void*>(&wgrad_stream_kernel<true>)
      : reinterpret_cast<const void*>(&wgrad_stream_kernel<false>);
  // what the device holds at once, split into K slots per tile; the
  // partials stay under PART_CAP_BYTES
  const long resident = colsum_grid(kernel, SNT, COLSUM_MAX_BLOCKS);
  long slots = std::max(1L, resident / tiles);
  slots = std::min(slots, (K + SK - 1) / SK);
  slots = std::min(slots, std::max(1L, PART_CAP_BYTES / (rowlen * 4)));
  // whole slabs per XCD: with slots a multiple of 8 every XCD's range of
  // logical ids is a whole number of (slot, all tiles) groups
  if (tiles > 1 && slots > 8) slots -= slots % 8;
  const long k_per_slot = ((K + slots - 1) / slots + SK - 1) / SK * SK;
  slots = (K + k_per_slot - 1) / k_per_slot;   // no empty slot
  const long nwg = slots * tiles;
  TORCH_CHECK(nwg <= INT_MAX, "wgrad: grid too large (", nwg, ")");

  const auto opts = dY.options().dtype(at::kFloat);
  auto out = at::empty({rowlen}, opts);
  auto part = slots > 1 ? at::empty({slots, rowlen}, opts) : out;
  auto stream = at::cuda::getCurrentHIPStream();
  const pb16* a = reinterpret_cast<const pb16*>(dY.data_ptr());
  const pb16* b = reinterpret_cast<const pb16*>(X.data_ptr());
  if (want_cs)
    hipLaunchKernelGGL(wgrad_stream_kernel<true>, dim3((unsigned int)nwg),
                       dim3(SNT), 0, stream, a, b, part.data_ptr<float>(),
                       K, M, N, k_per_slot, ntiles, (int)tiles, nwg, rowlen);
  else
    hipLaunchKernelGGL(wgrad_stream_kernel<false>, dim3((unsigned int)nwg),
                       dim3(SNT), 0, stream, a, b, part.data_ptr<float>(),
                       K, M, N, k_per_slot, ntiles, (int)tiles, nwg, rowlen);
  hipError_t err = hipGetLastError();
  TORCH_CHECK(err == hipSuccess, "wgrad: launch failed: ",
              hipGetErrorString(err));
  if (slots > 1) {
    colsum_fold_launch(part.data_ptr<float>(), out.data_ptr<float>(), slots,
                       rowlen, false, stream);
    err = hipGetLastError();
    TORCH_CHECK(err == hipSuccess, "wgrad: fold launch failed: ",
                hipGetErrorString(err));
  }
  std::vector<at::Tensor> ret{out.narrow(0, 0, MN).view({M, N})};
  if (want_cs) ret.push_back(out.narrow(0, MN, M));
  return ret;
}

void wgrad_check(const at::Tensor& dY, const at::Tensor& X) {
  TORCH_CHECK(dY.is_cuda() && X.is_cuda() && dY.device() == X.device(),
              "wgrad: operands must be on one GPU");
  TORCH_CHECK(dY.scalar_type() == at::kBFloat16 &&
              X.scalar_type() == at::kBFloat16, "wgrad: bf16 only");
  TORCH_CHECK(dY.is_contiguous() && X.is_contiguous(),
              "wgrad: contiguous inputs required");
  TORCH_CHECK(dY.dim() == 2 && X.dim() == 2 && dY.size(0) == X.size(0),
              "wgrad: (K, M) and (K, N) expected");
  TORCH_CHECK(dY.size(0) >= 1 && dY.size(1) >= 8 && X.size(1) >= 8,
              "wgrad: empty operand");
  TORCH_CHECK(dY.size(1) <= INT_MAX && X.size(1) <= INT_MAX,
              "wgrad: M, N must fit int");
  TORCH_CHECK(dY.size(1) % 8 == 0 && X.size(1) % 8 == 0,
              "wgrad: M, N multiples of 8");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(dY.data_ptr()) % 16 == 0 &&
              reinterpret_cast<uintptr_t>(X.data_ptr()) % 16 == 0,
              "wgrad: operands must be 16-byte aligned");
}

}  // namespace

// The r02 kernel: atomic drain into a zero-filled dW.
at::Tensor wgrad_v1(at::Tensor dY, at::Tensor X) {
  wgrad_check(dY, X);
  const long K = dY.size(0);
  const int M = dY.size(1);
  const int N = X.size(1);

  const int mtiles = (M + WM - 1) / WM;
  const int ntiles = (N + WN - 1) / WN;
  // enough k-slots to fill the chip (>= ~2048 blocks), each a multiple
  // of the 64-row stage
  long kslots = 2048 / ((long)mtiles * ntiles);
  kslots = std::max(1L, std::min(kslots, (K + KS - 1) / KS));
  long k_per_block = ((K + kslots - 1) / kslots + KS - 1) / KS * KS;
  kslots = (K + k_per_block - 1) / k_per_block;

  auto dW = kslots > 1
      ? at::zeros({M, N}, dY.options().dtype(at::kFloat))
      : at::empty({M, N}, dY.options().dtype(at::kFloat));
  dim3 grid(mtiles * ntiles, kslots);
  auto stream = at::cuda::getCurrentHIPStream();
  hipLaunchKernelGGL(wgrad_kernel, grid, dim3(NT), 0, stream,
                     reinterpret_cast<const pb16*>(dY.data_ptr()),
                     reinterpret_cast<const pb16*>(X.data_ptr()),
                     dW.data_ptr<float>(), K, M, N, k_per_block,
                     mtiles, ntiles);
  hipError_t err = hipGetLastError();
  TORCH_CHECK(err == hipSuccess, "wgrad: launch failed: ",
              hipGetErrorString(err));
  return dW;
}

// dW (M, N) fp32 = dY^T @ X with dY (K, M), X (K, N) bf16 row-major: the
// streaming kernel, or the r02 kernel under AF2AMD_WGRAD_V1=1.
at::Tensor wgrad(at::Tensor dY, at::Tensor X) {
  static const bool force_v1 = [] {
    const char* e = getenv("AF2AMD_WGRAD_V1");
    return e != nullptr && e[0] == '1';
  }();
  if (force_v1) return wgrad_v1(dY, X);
  wgrad_check(dY, X);
  return wgrad_stream(dY, X, false)[0];
}

// [dW (M, N), colsum (M,) = sum_k dY[k, :]] fp32, one pass over dY and X
// (always the streaming kernel).
std::vector<at::Tensor> wgrad_colsum(at::Tensor dY, at::Tensor X) {
  wgrad_check(dY, X);
  return wgrad_stream(dY, X, true);
}
