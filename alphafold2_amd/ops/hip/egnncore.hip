// Fused fp32 EGNN edge-message core — gfx950 (K16: the pair-sized half of
// models/equivariant.py EGNNLayer).
//
//   rel_ij = x_i - x_j              d2_ij = |rel_ij|^2
//   z1     = P_i + Q_j + w_d d2 + W_e edges_ij           s1 = silu(z1)
//   z2     = W2 s1 + b2             m_ij = silu(z2) * (mask_i & mask_j)
//   zc     = Wc1 m_ij + bc1         cw_ij = Wc2 . silu(zc) + bc2
//   m_i    = sum_j m_ij             dx_i = sum_j cw_ij rel_ij / sqrt(d2 + eps)
//
// P = W_i h + b1 and Q = W_j h are node-side library GEMMs; W_i, W_j, w_d,
// W_e are the column blocks of edge_mlp[0].weight in cat order.
//
// One block per query row (b,i), four waves, each wave owns 16 keys of a
// 64-key tile.  The three GEMMs run transposed on the f32-input MFMA
// (v_mfma_f32_16x16x4_f32, exact f32):  D^T[channel, key] = W[channel, k]
// act^T[k, key], weights as the A operand from LDS, activations as the B
// operand from registers.  The C/D map (row = 4 (lane >> 4) + reg, column
// = lane & 15) puts four consecutive channels of one key on a lane, which
// is exactly the k grouping of the next MFMA's B operand, so z1 -> z2 ->
// zc chain through registers with no LDS round trip: a k-slot is a pure
// reduction axis, and the weight fragment is read with the same
// permutation (one float4 of W[row][16 kk + 4 (lane >> 4) ..] feeds four
// MFMAs).  The same permutation lets a lane feed one float4 of
// edges[b,i,j, 16 kk + 4 (lane >> 4) ..] to four successive MFMAs, so
// edges is read once with 16-byte global loads and nothing pair-sized is
// written by the forward.
//
// Backward: the same block recomputes the chain and runs it in reverse.
// The transposed weight products read W[k][row] from the row-major LDS
// copy (scalar reads, conflict-free at the 68-float stride).  dW2 and
// dWc1 are MFMA products over the key axis; the two operands go through a
// per-wave LDS transpose ([channel][key]) first.  Every per-weight sum is
// a per-block partial folded on the host side in a fixed order; dQ and
// the j side of dx are fixed-order sums of what the row side stored: dz1
// (b,n,n,64) and drel (b,n,n,4), the gradient of rel_ij, a sixteenth of
// dz1.  (The j side of dx needs cw_ij, i.e. the whole chain, so without
// drel a column-side kernel would have to recompute the forward a second
// time.)  No float atomics.
//
// Edge dim 64, 128, 192 or 256: the whole W_e sits in LDS (64 x (E + 4)
// floats, 65 KiB at E = 256) next to W2, Wc1 and, in the backward, the
// transposes: 101.3 / 145.6 KiB per block at E = 256.  Wider edges need
// K-chunked staging of W_e and are rejected by the gate.  Keys are tiled,
// so nothing of length n lives in LDS and there is no bound on n.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <cstdint>

#include "common.h"

namespace {

constexpr int NT = 256;      // threads per block
constexpr int NW = NT / 64;  // waves per block
constexpr int M = 64;        // m_dim
constexpr int WS = M + 4;    // LDS row stride of the 64 x 64 weights
constexpr int TS = 16 + 4;   // LDS row stride of the [channel][key] transposes
constexpr int MAX_EC = 4;    // edge dim = 64 * EC, EC = 1..4
constexpr int NVEC_FWD = 5;  // P_i, w_d, b2, bc1, Wc2
constexpr int NVEC_BWD = 6;  // ... and dm_i
constexpr int NSUM = 5;      // dP, dw_d, db2, dbc1, dWc2

using f32x4 = __attribute__((ext_vector_type(4))) float;

__device__ __forceinline__ f32x4 ld4(const float* p) {
  return *reinterpret_cast<const f32x4*>(p);
}

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ float sigmoid_f(float z) {
  return 1.f / (1.f + expf(-z));
}

// sum over the 16 lanes that share lane >> 4 (the keys of a tile)
__device__ __forceinline__ float keys_reduce_sum(float v) {
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// sum over the 4 lanes that share lane & 15 (the channel groups of a key)
__device__ __forceinline__ float groups_reduce_sum(float v) {
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}

// LDS carve of both kernels (floats).  The regions addressed as smem +
// constant come first, so that their offsets fit a DS instruction's
// 16-bit immediate; W_e and the per-wave transposes are read off one
// base register each.
template <int EC>
struct Carve {
  static constexpr int E = 64 * EC;
  static constexpr int ES = E + 4;          // row stride of W_e
  static constexpr int w2 = 0;              // [M][WS]
  static constexpr int wc1 = w2 + M * WS;   // [M][WS]
  static constexpr int vec = wc1 + M * WS;  // [NVEC][M]
  static constexpr int fwd_red = vec + NVEC_FWD * M;        // [NW][M + 4]
  static constexpr int fwd_we = fwd_red + NW * (M + 4);     // [M][ES]
  static constexpr int fwd_end = fwd_we + M * ES;
  static constexpr int bwd_red = vec + NVEC_BWD * M;        // [NW][NSUM*M + 4]
  static constexpr int bwd_we = bwd_red + NW * (NSUM * M + 4);  // [M][ES]
  static constexpr int bwd_tr = bwd_we + M * ES;            // [NW][2][M][TS]
  static constexpr int bwd_end = bwd_tr + NW * 2 * M * TS;
};

// W_e (M, E), W2 / Wc1 (M, M) and the per-row vectors into LDS
template <int EC>
__device__ __forceinline__ void stage_weights(
    float* smem, float* we, const float* __restrict__ W_e,
    const float* __restrict__ W2, const float* __restrict__ Wc1) {
  using C = Carve<EC>;
  const int tid = threadIdx.x;
  for (int idx = tid * 4; idx < M * C::E; idx += NT * 4) {
    const int c = idx / C::E, k = idx - c * C::E;
    *reinterpret_cast<f32x4*>(we + c * C::ES + k) = ld4(W_e + idx);
  }
  for (int idx = tid * 4; idx < M * M; idx += NT * 4) {
    const int c = idx / M, k = idx - c * M;
    *reinterpret_cast<f32x4*>(smem + C::w2 + c * WS + k) = ld4(W2 + idx);
    *reinterpret_cast<f32x4*>(smem + C::wc1 + c * WS + k) = ld4(Wc1 + idx);
  }
}

// What one lane knows about its key of the tile.
struct Key {
  int j;          // key index (not clamped)
  long bj;        // b * n + min(j, n - 1): always a safe row
  bool valid;     // j < n
  bool pm;        // valid && mask_i && mask_j
  float r0, r1, r2, d2;
};

__device__ __forceinline__ Key load_key(
    int j, int n, long b, bool mask_i, const unsigned char* __restrict__ mask,
    const float* __restrict__ x, float xi0, float xi1, float xi2) {
  Key k;
  k.j = j;
  k.valid = j < n;
  k.bj = b * n + (k.valid ? j : n - 1);
  k.pm = k.valid && mask_i && (mask ? mask[k.bj] != 0 : true);
  k.r0 = xi0 - x[k.bj * 3];
  k.r1 = xi1 - x[k.bj * 3 + 1];
  k.r2 = xi2 - x[k.bj * 3 + 2];
  k.d2 = k.r0 * k.r0 + k.r1 * k.r1 + k.r2 * k.r2;
  return k;
}

// 64 MFMAs: z1 += W_e[:, 64 ec .. 64 ec + 63] (LDS) times the lane's four
// float4 of edges for those channels
template <int EC>
__device__ __forceinline__ void z1_step(
    f32x4 (&z1)[4], const f32x4 (&e4)[4], const float* we, int ec, int g,
    int l16) {
  using C = Carve<EC>;
  const float* wrow = we + l16 * C::ES + 64 * ec + 4 * g;
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) {
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      const f32x4 w4 = ld4(wrow + 16 * ct * C::ES + 16 * kk);
#pragma unroll
      for (int t = 0; t < 4; ++t) z1[ct] = mfma4(w4[t], e4[kk][t], z1[ct]);
    }
  }
}

// z1[ct][r]: channel 16 ct + 4 g + r of key l16, g = lane >> 4.  The
// steps over E are a real loop: unrolled, every load of the row is
// hoisted and costs more registers than there are.  With PREFETCH the
// next step's four float4 are in flight while this step's MFMAs run
// (forward); the backward has no registers to spare for that.
template <int EC, bool PREFETCH>
__device__ __forceinline__ void compute_z1(
    f32x4 (&z1)[4], const float* smem, const float* we, const Key& key,
    const float* __restrict__ Q, const float* __restrict__ erow, int g,
    int l16) {
  using C = Carve<EC>;
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) {
    const int c = 16 * ct + 4 * g;
    z1[ct] = ld4(smem + C::vec + c) + ld4(Q + key.bj * M + c)
        + ld4(smem + C::vec + M + c) * key.d2;
  }
  f32x4 e4[4];
  if constexpr (PREFETCH) {
    f32x4 nx[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) e4[kk] = ld4(erow + 16 * kk + 4 * g);
#pragma unroll 1
    for (int ec = 0; ec < EC; ++ec) {
      // the last step loads its own channels again: in bounds, unused
      const int pre = ec + 1 < EC ? ec + 1 : ec;
#pragma unroll
      for (int kk = 0; kk < 4; ++kk)
        nx[kk] = ld4(erow + 64 * pre + 16 * kk + 4 * g);
      z1_step<EC>(z1, e4, we, ec, g, l16);
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) e4[kk] = nx[kk];
    }
  } else {
#pragma unroll 1
    for (int ec = 0; ec < EC; ++ec) {
#pragma unroll
      for (int kk = 0; kk < 4; ++kk)
        e4[kk] = ld4(erow + 64 * ec + 16 * kk + 4 * g);
      z1_step<EC>(z1, e4, we, ec, g, l16);
    }
  }
}

// out = W act + bias for a 64 x 64 weight in LDS (row stride WS)
__device__ __forceinline__ void dense64(
    f32x4 (&out)[4], const f32x4 (&act)[4], const float* W, const float* bias,
    int g, int l16) {
#pragma unroll
  for (int co = 0; co < 4; ++co) {
    out[co] = ld4(bias + 16 * co + 4 * g);
#pragma unroll
    for (int ci = 0; ci < 4; ++ci) {
      const f32x4 w4 = ld4(W + (16 * co + l16) * WS + 16 * ci + 4 * g);
#pragma unroll
      for (int t = 0; t < 4; ++t) out[co] = mfma4(w4[t], act[ci][t], out[co]);
    }
  }
}

// out = init + W^T act: the A operand is W[k][row], read from the
// row-major copy (bank = 16 g + l16: conflict-free)
__device__ __forceinline__ void dense64_t(
    f32x4 (&out)[4], const f32x4 (&act)[4], const float* W, int g, int l16) {
#pragma unroll
  for (int co = 0; co < 4; ++co) {
#pragma unroll
    for (int ci = 0; ci < 4; ++ci) {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const float w = W[(16 * ci + 4 * g + t) * WS + 16 * co + l16];
        out[co] = mfma4(w, act[ci][t], out[co]);
      }
    }
  }
}

// inputs (fp32, contiguous, 16-byte aligned unless noted):
//   P, Q (b,n,M)   x (b,n,3), 4-byte aligned   edges (b,n,n,E)
//   W_e (M,E)  w_d (M)  W2 (M,M)  b2 (M)  Wc1 (M,M)  bc1 (M)  Wc2 (M)
//   bc2 (1)   mask (b,n) bytes or null
//   m_out (b,n,M)   dx_out (b,n,3): the unclamped coordinate update
template <int EC>
__global__ __launch_bounds__(NT)
void egnn_core_fwd_kernel(const float* __restrict__ P,
                          const float* __restrict__ Q,
                          const float* __restrict__ x,
                          const float* __restrict__ edges,
                          const float* __restrict__ W_e,
                          const float* __restrict__ w_d,
                          const float* __restrict__ W2,
                          const float* __restrict__ b2,
                          const float* __restrict__ Wc1,
                          const float* __restrict__ bc1,
                          const float* __restrict__ Wc2,
                          const float* __restrict__ bc2,
                          const unsigned char* __restrict__ mask,
                          float* __restrict__ m_out,
                          float* __restrict__ dx_out,
                          int n, float eps) {
  using C = Carve<EC>;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const long bi = blockIdx.x;           // b * n + i
  const long b = bi / n;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, l16 = lane & 15;

  float* we = smem + C::fwd_we;
  stage_weights<EC>(smem, we, W_e, W2, Wc1);
  if (tid < M) {
    smem[C::vec + tid] = P[bi * M + tid];
    smem[C::vec + M + tid] = w_d[tid];
    smem[C::vec + 2 * M + tid] = b2[tid];
    smem[C::vec + 3 * M + tid] = bc1[tid];
    smem[C::vec + 4 * M + tid] = Wc2[tid];
  }
  const float xi0 = x[bi * 3], xi1 = x[bi * 3 + 1], xi2 = x[bi * 3 + 2];
  const bool mask_i = mask ? mask[bi] != 0 : true;
  const float bc2v = bc2[0];
  __syncthreads();

  f32x4 macc[4];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) macc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
  float dxa0 = 0.f, dxa1 = 0.f, dxa2 = 0.f;

  for (int j0 = wave * 16; j0 < n; j0 += 16 * NW) {
    const Key key = load_key(j0 + l16, n, b, mask_i, mask, x, xi0, xi1, xi2);
    const float* erow =
        edges + (bi * n + (key.bj - b * n)) * (long)C::E;
    f32x4 z1[4], z2[4], zc[4];
    compute_z1<EC, true>(z1, smem, we, key, Q, erow, g, l16);
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
      for (int r = 0; r < 4; ++r) z1[ct][r] *= sigmoid_f(z1[ct][r]);
    dense64(z2, z1, smem + C::w2, smem + C::vec + 2 * M, g, l16);
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        z2[ct][r] = key.pm ? z2[ct][r] * sigmoid_f(z2[ct][r]) : 0.f;
      macc[ct] += z2[ct];
    }
    dense64(zc, z2, smem + C::wc1, smem + C::vec + 3 * M, g, l16);
    float cw = 0.f;
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      const f32x4 wc = ld4(smem + C::vec + 4 * M + 16 * ct + 4 * g);
#pragma unroll
      for (int r = 0; r < 4; ++r)
        cw += wc[r] * (zc[ct][r] * sigmoid_f(zc[ct][r]));
    }
    cw = groups_reduce_sum(cw) + bc2v;
    if (key.valid && g == 0) {
      // j == i has rel == 0 and contributes nothing
      const float s = cw / sqrtf(key.d2 + eps);
      dxa0 += s * key.r0;
      dxa1 += s * key.r1;
      dxa2 += s * key.r2;
    }
  }

  // ---- fold: 16 keys of a lane group, then the waves in order ---------
  float* red = smem + C::fwd_red + wave * (M + 4);
#pragma unroll
  for (int ct = 0; ct < 4; ++ct)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float v = keys_reduce_sum(macc[ct][r]);
      if (l16 == 0) red[16 * ct + 4 * g + r] = v;
    }
  dxa0 = wave_reduce_sum(dxa0);
  dxa1 = wave_reduce_sum(dxa1);
  dxa2 = wave_reduce_sum(dxa2);
  if (lane == 0) {
    red[M] = dxa0;
    red[M + 1] = dxa1;
    red[M + 2] = dxa2;
  }
  __syncthreads();
  if (tid < M + 3) {
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) t += smem[C::fwd_red + w * (M + 4) + tid];
    if (tid < M) m_out[bi * M + tid] = t;
    else dx_out[bi * 3 + (tid - M)] = t;
  }
}

// d silu(z) / dz given sg = sigmoid(z)
__device__ __forceinline__ float dsilu(float z, float sg) {
  return sg * (1.f + z * (1.f - sg));
}

// sums[channel 16 ct + 4 g + r] += the 16 keys' sum of v; sums is a
// wave-private LDS row
__device__ __forceinline__ void add_channel_sum(
    float* sums, float v, int ct, int r, int g, int l16) {
  v = keys_reduce_sum(v);
  if (l16 == 0) sums[16 * ct + 4 * g + r] += v;
}

// Writes act[ct][r] (channel 16 ct + 4 g + r, key l16) into a per-wave
// [channel][key] LDS image with row stride TS.
__device__ __forceinline__ void store_transposed(
    float* dst, const f32x4 (&act)[4], int g, int l16) {
#pragma unroll
  for (int ct = 0; ct < 4; ++ct)
#pragma unroll
    for (int r = 0; r < 4; ++r)
      dst[(16 * ct + 4 * g + r) * TS + l16] = act[ct][r];
}

// acc[ro][co] += rows^T-image x cols^T-image over the 16 keys of the tile:
// acc tile (ro, co) holds dW[16 ro + 4 g + reg][16 co + l16]
__device__ __forceinline__ void outer_over_keys(
    f32x4 (&acc)[4][4], const float* rows, const float* cols, int g,
    int l16) {
  f32x4 a4[4], b4[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    a4[q] = ld4(rows + (16 * q + l16) * TS + 4 * g);
    b4[q] = ld4(cols + (16 * q + l16) * TS + 4 * g);
  }
#pragma unroll
  for (int ro = 0; ro < 4; ++ro)
#pragma unroll
    for (int co = 0; co < 4; ++co)
#pragma unroll
      for (int t = 0; t < 4; ++t)
        acc[ro][co] = mfma4(a4[ro][t], b4[co][t], acc[ro][co]);
}

// Folds the four waves' 64 x 64 accumulators through `buf` ([M][WS], LDS)
// in wave order and writes the block's partial to dst (M, M).
__device__ __forceinline__ void fold_weight_partial(
    const f32x4 (&acc)[4][4], float* buf, float* __restrict__ dst, int wave,
    int g, int l16) {
  for (int w = 0; w < NW; ++w) {
    if (wave == w) {
#pragma unroll
      for (int ro = 0; ro < 4; ++ro)
#pragma unroll
        for (int co = 0; co < 4; ++co)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float* p = buf + (16 * ro + 4 * g + r) * WS + 16 * co + l16;
            *p = w == 0 ? acc[ro][co][r] : *p + acc[ro][co][r];
          }
    }
    __syncthreads();
  }
  for (int idx = threadIdx.x * 4; idx < M * M; idx += NT * 4) {
    const int c = idx / M, k = idx - c * M;
    *reinterpret_cast<f32x4*>(dst + idx) = ld4(buf + c * WS + k);
  }
}

// ---- backward: one block per (b, i) ----------------------------------
//   dm (b,n,M), ddx (b,n,3): incoming gradients of m_i and of the
//   unclamped dx.  Writes
//     dz1 (b,n,n,M)      gradient of z1, the pair-sized intermediate
//     drel (b,n,n,4)     d loss / d rel_ij in .xyz (dx_j = -sum_i of it)
//     dP (b,n,M)         = sum_j dz1
//     dx_row (b,n,3)     = sum_j drel, the i side of dx
//     vec_part (b*n, 4, M)  partials of dw_d, db2, dbc1, dWc2
//     dbc2_part (b*n)
//     dW2_part, dWc1_part (b*n, M, M)
template <int EC>
__global__ __launch_bounds__(NT)
void egnn_core_bwd_kernel(const float* __restrict__ dm,
                          const float* __restrict__ ddx,
                          const float* __restrict__ P,
                          const float* __restrict__ Q,
                          const float* __restrict__ x,
                          const float* __restrict__ edges,
                          const float* __restrict__ W_e,
                          const float* __restrict__ w_d,
                          const float* __restrict__ W2,
                          const float* __restrict__ b2,
                          const float* __restrict__ Wc1,
                          const float* __restrict__ bc1,
                          const float* __restrict__ Wc2,
                          const float* __restrict__ bc2,
                          const unsigned char* __restrict__ mask,
                          float* __restrict__ dz1_out,
                          float* __restrict__ drel_out,
                          float* __restrict__ dP,
                          float* __restrict__ dx_row,
                          float* __restrict__ vec_part,
                          float* __restrict__ dbc2_part,
                          float* __restrict__ dW2_part,
                          float* __restrict__ dWc1_part,
                          int n, float eps) {
  using C = Carve<EC>;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const long bi = blockIdx.x;           // b * n + i
  const long b = bi / n;
  const int i = bi - b * n;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, l16 = lane & 15;

  float* we = smem + C::bwd_we;
  stage_weights<EC>(smem, we, W_e, W2, Wc1);
  if (tid < M) {
    smem[C::vec + tid] = P[bi * M + tid];
    smem[C::vec + M + tid] = w_d[tid];
    smem[C::vec + 2 * M + tid] = b2[tid];
    smem[C::vec + 3 * M + tid] = bc1[tid];
    smem[C::vec + 4 * M + tid] = Wc2[tid];
    smem[C::vec + 5 * M + tid] = dm[bi * M + tid];
  }
  const float xi0 = x[bi * 3], xi1 = x[bi * 3 + 1], xi2 = x[bi * 3 + 2];
  const float g0 = ddx[bi * 3], g1 = ddx[bi * 3 + 1], g2 = ddx[bi * 3 + 2];
  const bool mask_i = mask ? mask[bi] != 0 : true;
  const float bc2v = bc2[0];
  float* trA = smem + C::bwd_tr + wave * 2 * M * TS;
  float* trB = trA + M * TS;
  // per-channel sums of this wave (dP, dw_d, db2, dbc1, dWc2) live in its
  // own LDS rows: each tile adds its 16 keys' sum, always from the same
  // lane, so the order is fixed and no barrier is needed
  float* red = smem + C::bwd_red + wave * (NSUM * M + 4);
  for (int idx = lane; idx < NSUM * M + 4; idx += 64) red[idx] = 0.f;
  __syncthreads();

  f32x4 dW2a[4][4], dWc1a[4][4];
#pragma unroll
  for (int ro = 0; ro < 4; ++ro)
#pragma unroll
    for (int co = 0; co < 4; ++co) {
      dW2a[ro][co] = f32x4{0.f, 0.f, 0.f, 0.f};
      dWc1a[ro][co] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  float sBc2 = 0.f, dxa0 = 0.f, dxa1 = 0.f, dxa2 = 0.f;

  // every wave runs every tile (the loop holds block barriers); a wave
  // past the end works on clamped keys and contributes zeros
  for (int t0 = 0; t0 < n; t0 += 16 * NW) {
    const Key key = load_key(t0 + wave * 16 + l16, n, b, mask_i, mask, x,
                             xi0, xi1, xi2);
    const long pair = bi * n + (key.bj - b * n);
    f32x4 z1[4], s1[4], z2[4], mij[4], zc[4], dzc[4], dmm[4], dz2[4],
        dz1[4];
    compute_z1<EC, false>(z1, smem, we, key, Q,
                           edges + pair * (long)C::E, g, l16);
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        s1[ct][r] = z1[ct][r] * sigmoid_f(z1[ct][r]);
    dense64(z2, s1, smem + C::w2, smem + C::vec + 2 * M, g, l16);
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        mij[ct][r] = key.pm ? z2[ct][r] * sigmoid_f(z2[ct][r]) : 0.f;
    dense64(zc, mij, smem + C::wc1, smem + C::vec + 3 * M, g, l16);

    // ---- coordinate head: cw, its gradient, dzc -----------------------
    const float inv = 1.f / sqrtf(key.d2 + eps);
    // rel_ii == 0, so the diagonal has dcw == 0 without a test
    const float dcw = key.valid
        ? (key.r0 * g0 + key.r1 * g1 + key.r2 * g2) * inv : 0.f;
    float cw = 0.f;
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      const f32x4 wc = ld4(smem + C::vec + 4 * M + 16 * ct + 4 * g);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float z = zc[ct][r];
        const float sg = sigmoid_f(z);
        const float sz = z * sg;
        cw += wc[r] * sz;
        const float d = dcw * wc[r] * dsilu(z, sg);
        dzc[ct][r] = d;
        add_channel_sum(red + 4 * M, dcw * sz, ct, r, g, l16);
        add_channel_sum(red + 3 * M, d, ct, r, g, l16);
      }
    }
    cw = groups_reduce_sum(cw) + bc2v;
    if (g == 0) sBc2 += dcw;

    // ---- dm_ij = dm_i + Wc1^T dzc, then dWc1 += dzc m^T over the keys
    // of the tile (the operands leave the registers as early as possible)
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
      dmm[ct] = ld4(smem + C::vec + 5 * M + 16 * ct + 4 * g);
    dense64_t(dmm, dzc, smem + C::wc1, g, l16);
    __syncthreads();
    store_transposed(trA, dzc, g, l16);
    store_transposed(trB, mij, g, l16);
    __syncthreads();
    outer_over_keys(dWc1a, trA, trB, g, l16);

    // ---- dz2, then dW2 += dz2 s1^T --------------------------------------
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float z = z2[ct][r];
        dz2[ct][r] = key.pm ? dmm[ct][r] * dsilu(z, sigmoid_f(z)) : 0.f;
        add_channel_sum(red + 2 * M, dz2[ct][r], ct, r, g, l16);
      }
    }
    __syncthreads();
    store_transposed(trA, dz2, g, l16);
    store_transposed(trB, s1, g, l16);
    __syncthreads();
    outer_over_keys(dW2a, trA, trB, g, l16);

    // ---- ds1 = W2^T dz2, dz1 ---------------------------------------------
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) dz1[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    dense64_t(dz1, dz2, smem + C::w2, g, l16);
    float dd2 = 0.f;
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      const f32x4 wd = ld4(smem + C::vec + M + 16 * ct + 4 * g);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float z = z1[ct][r];
        const float d = dz1[ct][r] * dsilu(z, sigmoid_f(z));
        dz1[ct][r] = d;
        dd2 += d * wd[r];
        add_channel_sum(red, d, ct, r, g, l16);
        add_channel_sum(red + M, d * key.d2, ct, r, g, l16);
      }
      if (key.valid)
        *reinterpret_cast<f32x4*>(dz1_out + pair * M + 16 * ct + 4 * g) =
            dz1[ct];
    }
    dd2 = groups_reduce_sum(dd2);

    // ---- d loss / d rel_ij ---------------------------------------------
    if (key.valid && g == 0) {
      float d0 = 2.f * dd2 * key.r0, d1 = 2.f * dd2 * key.r1,
            d2 = 2.f * dd2 * key.r2;
      // rel_norm path: u / s - rel (rel.u) / s^3 with u = cw ddx_i.  The
      // diagonal cancels against the j side analytically and is skipped.
      if (key.j != i) {
        const float u0 = cw * g0, u1 = cw * g1, u2 = cw * g2;
        const float ru = (key.r0 * u0 + key.r1 * u1 + key.r2 * u2)
            * inv * inv * inv;
        d0 += u0 * inv - key.r0 * ru;
        d1 += u1 * inv - key.r1 * ru;
        d2 += u2 * inv - key.r2 * ru;
      }
      dxa0 += d0;
      dxa1 += d1;
      dxa2 += d2;
      *reinterpret_cast<f32x4*>(drel_out + pair * 4) = f32x4{d0, d1, d2, 0.f};
    }
  }

  // ---- fold the waves' sums in wave order -----------------------------
  sBc2 = wave_reduce_sum(sBc2);
  dxa0 = wave_reduce_sum(dxa0);
  dxa1 = wave_reduce_sum(dxa1);
  dxa2 = wave_reduce_sum(dxa2);
  if (lane == 0) {
    red[NSUM * M] = sBc2;
    red[NSUM * M + 1] = dxa0;
    red[NSUM * M + 2] = dxa1;
    red[NSUM * M + 3] = dxa2;
  }
  __syncthreads();          // also: every wave is done with W2 / Wc1
  for (int idx = tid; idx < NSUM * M + 4; idx += NT) {
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w)
      t += smem[C::bwd_red + w * (NSUM * M + 4) + idx];
    if (idx < M) dP[bi * M + idx] = t;
    else if (idx < NSUM * M) vec_part[bi * (4 * M) + (idx - M)] = t;
    else if (idx == NSUM * M) dbc2_part[bi] = t;
    else dx_row[bi * 3 + (idx - NSUM * M - 1)] = t;
  }

  fold_weight_partial(dW2a, smem + C::w2, dW2_part + bi * (M * M), wave, g,
                      l16);
  fold_weight_partial(dWc1a, smem + C::wc1, dWc1_part + bi * (M * M), wave,
                      g, l16);
}

// ---- host side --------------------------------------------------------

long fwd_lds_bytes(long EC) {
  return (M * (64 * EC + 4) + 2 * M * WS + NVEC_FWD * M + NW * (M + 4))
      * (long)sizeof(float);
}
long bwd_lds_bytes(long EC) {
  return (M * (64 * EC + 4) + 2 * M * WS + NVEC_BWD * M
          + NW * (NSUM * M + 4) + NW * 2 * M * TS) * (long)sizeof(float);
}
// LDS one workgroup may use on the current device, opt-in included
long device_lds_limit() {
  int dev = 0, base = 0, optin = 0;
  TORCH_CHECK(hipGetDevice(&dev) == hipSuccess, "egnn_core: hipGetDevice");
  TORCH_CHECK(hipDeviceGetAttribute(
                  &base, hipDeviceAttributeMaxSharedMemoryPerBlock, dev)
              == hipSuccess, "egnn_core: LDS size query failed");
  if (hipDeviceGetAttribute(&optin, hipDeviceAttributeSharedMemPerBlockOptin,
                            dev) != hipSuccess) {
    (void)hipGetLastError();
    optin = 0;
  }
  return base > optin ? base : optin;
}

template <typename K>
void prepare_launch(K kernel, long smem, const char* name) {
  TORCH_CHECK(smem <= device_lds_limit(), name, ": needs ", smem,
              " B of LDS per block, the device allows ", device_lds_limit());
  if (smem > 64 * 1024) {
    TORCH_CHECK(hipFuncSetAttribute(
                    reinterpret_cast<const void*>(kernel),
                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem)
                == hipSuccess, name, ": LDS opt-in failed");
  }
}

void check_launch(const char* name) {
  const hipError_t err = hipGetLastError();
  TORCH_CHECK(err == hipSuccess, name, ": launch failed: ",
              hipGetErrorString(err));
}

void check_f32(const at::Tensor& t, const char* what, int align = 16) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kFloat
              && t.is_contiguous(), what,
              ": fp32 contiguous device tensors required");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % align == 0, what,
              ": tensors must be 16-byte aligned (x: 4-byte)");
}

struct Dims { int b, n, EC; };

Dims check_dims(const at::Tensor& P, const at::Tensor& Q,
                const at::Tensor& x, const at::Tensor& edges,
                const at::Tensor& W_e, const at::Tensor& w_d,
                const at::Tensor& W2, const at::Tensor& b2,
                const at::Tensor& Wc1, const at::Tensor& bc1,
                const at::Tensor& Wc2, const at::Tensor& bc2,
                const c10::optional<at::Tensor>& mask, const char* what) {
  for (const at::Tensor* t :
       {&P, &Q, &edges, &W_e, &w_d, &W2, &b2, &Wc1, &bc1, &Wc2, &bc2})
    check_f32(*t, what);
  check_f32(x, what, 4);                // read as scalars
  TORCH_CHECK(P.dim() == 3 && edges.dim() == 4, what, ": bad ranks");
  const long b = P.size(0), n = P.size(1), E = edges.size(3);
  TORCH_CHECK(P.size(2) == M, what, ": m_dim must be 64");
  TORCH_CHECK(E % 64 == 0 && E >= 64 && E <= 64 * MAX_EC, what,
              ": edge dim must be a multiple of 64 up to 256");
  TORCH_CHECK(b * n > 0 && b * n < (1L << 31) && b * n * n < (1L << 40),
              what, ": bad batch / length");
  auto is = [](const at::Tensor& t, at::IntArrayRef s) {
    return t.sizes() == s;
  };
  TORCH_CHECK(is(P, {b, n, M}) && is(Q, {b, n, M}) && is(x, {b, n, 3})
              && is(edges, {b, n, n, E}) && is(W_e, {M, E}) && is(w_d, {M})
              && is(W2, {M, M}) && is(b2, {M}) && is(Wc1, {M, M})
              && is(bc1, {M}) && Wc2.numel() == M && bc2.numel() == 1,
              what, ": shapes do not match");
  if (mask.has_value()) {
    TORCH_CHECK(mask->is_cuda() && mask->scalar_type() == at::kBool
                && mask->is_contiguous() && is(*mask, {b, n}),
                what, ": mask must be a contiguous (b, n) bool tensor");
  }
  return {(int)b, (int)n, (int)(E / 64)};
}

const unsigned char* mask_ptr(const c10::optional<at::Tensor>& mask) {
  return mask.has_value()
      ? reinterpret_cast<const unsigned char*>(mask->data_ptr<bool>())
      : nullptr;
}

#define EGNN_DISPATCH_EC(EC_RT, ...)                                   \
  switch (EC_RT) {                                                     \
    case 1: { constexpr int EC = 1; __VA_ARGS__; break; }              \
    case 2: { constexpr int EC = 2; __VA_ARGS__; break; }              \
    case 3: { constexpr int EC = 3; __VA_ARGS__; break; }              \
    case 4: { constexpr int EC = 4; __VA_ARGS__; break; }              \
    default: TORCH_CHECK(false, "egnn_core: edge dim must be 64..256"); \
  }

}  // namespace

// Largest edge dim (a multiple of 64) whose forward AND backward fit the
// device's LDS per block and have a kernel; 0 when none does.  The design
// has no bound on n: keys are tiled, nothing of length n lives in LDS.
long egnn_core_max_edge_dim() {
  const long limit = device_lds_limit();
  long best = 0;
  for (long ec = 1; ec <= MAX_EC; ++ec)
    if (bwd_lds_bytes(ec) <= limit && fwd_lds_bytes(ec) <= limit)
      best = 64 * ec;
  return best;
}

// Returns {m_i (b,n,M), dx (b,n,3)}; dx is the unclamped coordinate update.
std::vector<at::Tensor> egnn_core_fwd(
    at::Tensor P, at::Tensor Q, at::Tensor x, at::Tensor edges,
    at::Tensor W_e, at::Tensor w_d, at::Tensor W2, at::Tensor b2,
    at::Tensor Wc1, at::Tensor bc1, at::Tensor Wc2, at::Tensor bc2,
    double eps, c10::optional<at::Tensor> mask) {
  const Dims d = check_dims(P, Q, x, edges, W_e, w_d, W2, b2, Wc1, bc1, Wc2,
                            bc2, mask, "egnn_core_fwd");
  auto m_out = at::empty_like(P);
  auto dx = at::empty({d.b, d.n, 3}, P.options());
  const long smem = fwd_lds_bytes(d.EC);
  auto stream = at::cuda::getCurrentHIPStream();
  EGNN_DISPATCH_EC(d.EC, {
    static_assert(Carve<EC>::fwd_end == M * (64 * EC + 4) + 2 * M * WS
                  + NVEC_FWD * M + NW * (M + 4), "fwd_lds_bytes mirrors Carve");
    static_assert(Carve<EC>::fwd_we * sizeof(float) < 65536, "DS immediates");
    prepare_launch(egnn_core_fwd_kernel<EC>, smem, "egnn_core_fwd");
    hipLaunchKernelGGL(egnn_core_fwd_kernel<EC>, dim3((long)d.b * d.n),
                       dim3(NT), smem, stream,
                       P.data_ptr<float>(), Q.data_ptr<float>(),
                       x.data_ptr<float>(), edges.data_ptr<float>(),
                       W_e.data_ptr<float>(), w_d.data_ptr<float>(),
                       W2.data_ptr<float>(), b2.data_ptr<float>(),
                       Wc1.data_ptr<float>(), bc1.data_ptr<float>(),
                       Wc2.data_ptr<float>(), bc2.data_ptr<float>(),
                       mask_ptr(mask), m_out.data_ptr<float>(),
                       dx.data_ptr<float>(), d.n, (float)eps);
  });
  check_launch("egnn_core_fwd");
  return {m_out, dx};
}

// Returns {dP, dQ, dx, dz1, dw_d, dW2, db2, dWc1, dbc1, dWc2, dbc2}.  dz1
// (b,n,n,M) is the gradient of the first Linear's output: the caller
// takes dedges = dz1 W_e and dW_e = dz1^T edges from it.
std::vector<at::Tensor> egnn_core_bwd(
    at::Tensor dm, at::Tensor ddx, at::Tensor P, at::Tensor Q, at::Tensor x,
    at::Tensor edges, at::Tensor W_e, at::Tensor w_d, at::Tensor W2,
    at::Tensor b2, at::Tensor Wc1, at::Tensor bc1, at::Tensor Wc2,
    at::Tensor bc2, double eps, c10::optional<at::Tensor> mask) {
  const Dims d = check_dims(P, Q, x, edges, W_e, w_d, W2, b2, Wc1, bc1, Wc2,
                            bc2, mask, "egnn_core_bwd");
  check_f32(dm, "egnn_core_bwd");
  check_f32(ddx, "egnn_core_bwd", 4);
  TORCH_CHECK(dm.sizes() == P.sizes() && ddx.sizes() == x.sizes(),
              "egnn_core_bwd: dm / ddx shapes do not match");

  auto opt = P.options();
  const long rows = (long)d.b * d.n;
  auto dz1 = at::empty({d.b, d.n, d.n, M}, opt);
  auto drel = at::empty({d.b, d.n, d.n, 4}, opt);
  auto dP = at::empty_like(P);
  auto dx_row = at::empty({d.b, d.n, 3}, opt);
  auto vec_part = at::empty({rows, 4, M}, opt);
  auto dbc2_part = at::empty({rows}, opt);
  auto dW2_part = at::empty({rows, M, M}, opt);
  auto dWc1_part = at::empty({rows, M, M}, opt);

  const long smem = bwd_lds_bytes(d.EC);
  auto stream = at::cuda::getCurrentHIPStream();
  EGNN_DISPATCH_EC(d.EC, {
    static_assert(Carve<EC>::bwd_end == M * (64 * EC + 4) + 2 * M * WS
                  + NVEC_BWD * M + NW * (NSUM * M + 4) + NW * 2 * M * TS,
                  "bwd_lds_bytes mirrors Carve");
    static_assert(Carve<EC>::bwd_we * sizeof(float) < 65536, "DS immediates");
    prepare_launch(egnn_core_bwd_kernel<EC>, smem, "egnn_core_bwd");
    hipLaunchKernelGGL(egnn_core_bwd_kernel<EC>, dim3(rows), dim3(NT), smem,
                       stream,
                       dm.data_ptr<float>(), ddx.data_ptr<float>(),
                       P.data_ptr<float>(), Q.data_ptr<float>(),
                       x.data_ptr<float>(), edges.data_ptr<float>(),
                       W_e.data_ptr<float>(), w_d.data_ptr<float>(),
                       W2.data_ptr<float>(), b2.data_ptr<float>(),
                       Wc1.data_ptr<float>(), bc1.data_ptr<float>(),
                       Wc2.data_ptr<float>(), bc2.data_ptr<float>(),
                       mask_ptr(mask), dz1.data_ptr<float>(),
                       drel.data_ptr<float>(), dP.data_ptr<float>(),
                       dx_row.data_ptr<float>(), vec_part.data_ptr<float>(),
                       dbc2_part.data_ptr<float>(),
                       dW2_part.data_ptr<float>(),
                       dWc1_part.data_ptr<float>(), d.n, (float)eps);
  });
  check_launch("egnn_core_bwd");

  // column side and the per-block partials: fixed-order sums
  auto dQ = dz1.sum(1);                                   // over i
  auto dx = dx_row - drel.sum(1).narrow(-1, 0, 3);        // i side - j side
  auto vec = vec_part.sum(0);                             // (4, M)
  auto dW2 = dW2_part.sum(0);
  auto dWc1 = dWc1_part.sum(0);
  auto dbc2 = dbc2_part.sum(0).reshape(bc2.sizes());
  return {dP, dQ, dx, dz1, vec.select(0, 0), dW2, vec.select(0, 1), dWc1,
          vec.select(0, 2), vec.select(0, 3).reshape(Wc2.sizes()), dbc2};
}
