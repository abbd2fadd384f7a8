// Fused fp32 Invariant-Point-Attention core — gfx950 (K7 of SURVEY.md
// §2.17, reference alphafold2.py:873-891 + external IPABlock).
//
// Forward: logits (scalar QK + pair bias - point-distance term, with
// the optional padding mask), per-head softmax, and the three value
// aggregations + local-frame rotation + point norms in ONE VALU kernel
// (the structure module is fp32-pinned and gfx950 has no fp32 MFMA; the
// win is fusion, not matrix cores).  Heads 1..8 (template), pair dim any
// multiple of 64 up to 512 (runtime), scalar dims 16/16, points 4/4.
//
// Backward: two deterministic kernels, no float atomics.
//   row side    one block per (b,i): dA, delta, dL; owns dq_s, dq_pg,
//               dbias (= s_b * dL), dpair, dR, dt and a per-block partial
//               of dpoint_w (folded by a sum afterwards)
//   column side one block per (b,j): reads the A and dbias columns; owns
//               dk_s, dk_pg, dv_s, dv_pg
// The forward saves the probabilities A (b,H,n,n) and the aggregated
// global points when gradients are required; nothing of size b*h*n*n*p
// is ever materialised.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <cfloat>
#include <cstdint>

#include "common.h"

namespace {

constexpr int DS = 16;      // scalar qk dim
constexpr int DV = 16;      // scalar value dim
constexpr int P = 4;        // points (key == value count here)
constexpr int P3 = P * 3;
constexpr int NT = 256;     // threads per block
constexpr int NW = NT / 64; // waves per block
constexpr int MAX_H = 8;
constexpr int MAX_DP = 512; // pairwise repr dim: multiple of 64, <= 512

// per-i output row layout (matches models/ipa.py `pieces` concat):
//   [ h*DV scalar | h*DP pair | h*P*3 local points | h*P norms ]

// Block-wide sum of H per-thread values; the totals come back in v[] on
// every thread.  `red` holds NW * H floats.
template <int H>
__device__ __forceinline__ void block_reduce_heads(float (&v)[H],
                                                   float* red) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
#pragma unroll
  for (int h = 0; h < H; ++h) {
    v[h] = wave_reduce_sum(v[h]);
    if (lane == 0) red[wave * H + h] = v[h];
  }
  __syncthreads();
#pragma unroll
  for (int h = 0; h < H; ++h) {
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) t += red[w * H + h];
    v[h] = t;
  }
  __syncthreads();
}

// inputs (all fp32, contiguous):
//   q_s, k_s: (b, n, H, DS)      v_s: (b, n, H, DV)
//   q_pg, k_pg, v_pg: (b, n, H, P, 3)   (already in GLOBAL frame)
//   bias: (b, H, n, n)   pair: (b, n, n, DP)
//   rot: (b, n, 3, 3)  trans: (b, n, 3)
//   point_w: (H,) softplus-ed weights
//   mask: (b, n) bytes or null; logits with !(mask[i] & mask[j]) become
//         -FLT_MAX, so a padded query row gets the uniform 1/n softmax
//   attn_save (b, H, n, n) / gpts_save (b, n, H*P*3): null when no
//         gradient is required
template <int H>
__global__ __launch_bounds__(NT, 4)
void ipa_core_kernel(const float* __restrict__ q_s,
                     const float* __restrict__ k_s,
                     const float* __restrict__ v_s,
                     const float* __restrict__ q_pg,
                     const float* __restrict__ k_pg,
                     const float* __restrict__ v_pg,
                     const float* __restrict__ bias,
                     const float* __restrict__ pair,
                     const float* __restrict__ rot,
                     const float* __restrict__ trans,
                     const float* __restrict__ point_w,
                     const unsigned char* __restrict__ mask,
                     float* __restrict__ out,
                     float* __restrict__ attn_save,
                     float* __restrict__ gpts_save,
                     int n, int DP, float scale_s, float scale_b,
                     float scale_p, float eps) {
  extern __shared__ float smem[];
  float* logits = smem;                 // [H][n]
  float* qrow = logits + H * n;         // q_s[i]: [H][DS]
  float* qpts = qrow + H * DS;          // q_pg[i]: [H][P][3]
  float* red = qpts + H * P3;           // [H][NW] reduction scratch
  float* gpts = red + H * NW;           // aggregated global points [H*P*3]

  constexpr int OUT_SCALAR = H * DV;
  constexpr int OUT_PTS = H * P3;
  const int OUT_PAIR = H * DP;
  const int DOUT = OUT_SCALAR + OUT_PAIR + OUT_PTS + H * P;

  const long bi = blockIdx.x;           // b * n + i
  const long b = bi / n;
  const int i = bi - b * n;
  const int tid = threadIdx.x;

  // stage the query row
  for (int c = tid; c < H * DS; c += NT) qrow[c] = q_s[bi * H * DS + c];
  for (int c = tid; c < H * P3; c += NT)
    qpts[c] = q_pg[bi * (long)H * P3 + c];
  __syncthreads();

  const bool mi = mask ? mask[bi] != 0 : true;

  // ---- pass 1: logits[h][j], thread owns column j -------------------
  for (int j = tid; j < n; j += NT) {
    const float* krow = k_s + (b * (long)n + j) * H * DS;
    const float* kpts = k_pg + (b * (long)n + j) * (long)H * P3;
    const float* brow = bias + ((b * H) * (long)n + i) * n + j;  // [h] stride n*n
    const bool valid = mi && (mask ? mask[b * n + j] != 0 : true);
#pragma unroll
    for (int h = 0; h < H; ++h) {
      float dot = 0.f;
#pragma unroll
      for (int d = 0; d < DS; ++d)
        dot += qrow[h * DS + d] * krow[h * DS + d];
      float d2 = 0.f;
#pragma unroll
      for (int p = 0; p < P; ++p) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float dd = qpts[(h * P + p) * 3 + c]
              - kpts[(h * P + p) * 3 + c];
          d2 += dd * dd;
        }
      }
      const float bia = brow[(long)h * n * n];
      const float lg = dot * scale_s + bia * scale_b
          - 0.5f * point_w[h] * scale_p * d2;
      logits[h * n + j] = valid ? lg : -FLT_MAX;
    }
  }
  __syncthreads();

  // ---- pass 2: per-head softmax over j ------------------------------
  const int lane = tid & 63;
  const int wave = tid >> 6;
  for (int h = 0; h < H; ++h) {
    // -FLT_MAX, not a larger sentinel: a fully masked row must reduce to
    // m == -FLT_MAX so that exp(logit - m) == 1 on every column
    float m = -FLT_MAX;
    for (int j = tid; j < n; j += NT) m = fmaxf(m, logits[h * n + j]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
      m = fmaxf(m, __shfl_down(m, off, 64));
    if (lane == 0) red[h * NW + wave] = m;
    __syncthreads();
    m = red[h * NW + 0];
    for (int w = 1; w < NW; ++w) m = fmaxf(m, red[h * NW + w]);

    float s = 0.f;
    for (int j = tid; j < n; j += NT) {
      const float e = __expf(logits[h * n + j] - m);
      logits[h * n + j] = e;
      s += e;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    __syncthreads();          // red[] reuse
    if (lane == 0) red[h * NW + wave] = s;
    __syncthreads();
    s = 0.f;
    for (int w = 0; w < NW; ++w) s += red[h * NW + w];
    const float inv = 1.f / s;
    for (int j = tid; j < n; j += NT) logits[h * n + j] *= inv;
    __syncthreads();
  }

  if (attn_save) {
    for (int h = 0; h < H; ++h) {
      float* arow = attn_save + ((b * H + h) * (long)n + i) * n;
      for (int j = tid; j < n; j += NT) arow[j] = logits[h * n + j];
    }
  }

  // ---- pass 3: aggregations, thread owns one output channel ---------
  float* orow = out + bi * (long)DOUT;

  // 3a. pair: thread owns channel c; all H heads accumulated
  for (int c = tid; c < DP; c += NT) {
    float acc[H];
#pragma unroll
    for (int h = 0; h < H; ++h) acc[h] = 0.f;
    const float* prow = pair + (b * (long)n + i) * (long)n * DP;
    for (int j = 0; j < n; ++j) {
      const float pv = prow[(long)j * DP + c];   // coalesced across tid
#pragma unroll
      for (int h = 0; h < H; ++h) acc[h] += logits[h * n + j] * pv;
    }
#pragma unroll
    for (int h = 0; h < H; ++h)
      orow[OUT_SCALAR + h * DP + c] = acc[h];
  }

  // 3b. scalar values: channels (h, d) for tid < H*DV
  if (tid < OUT_SCALAR) {
    const int h = tid / DV, d = tid - (tid / DV) * DV;
    float acc = 0.f;
    for (int j = 0; j < n; ++j)
      acc += logits[h * n + j] * v_s[(b * (long)n + j) * H * DV + h * DV + d];
    orow[tid] = acc;
  }

  // 3c. points: aggregate global components (one channel per thread),
  // then rotate to the local frame; norms from the local vector
  if (tid < OUT_PTS) {
    const int h = tid / P3;
    float g = 0.f;
    for (int j = 0; j < n; ++j)
      g += logits[h * n + j] * v_pg[(b * (long)n + j) * (long)H * P3 + tid];
    gpts[tid] = g;
    if (gpts_save) gpts_save[bi * (long)OUT_PTS + tid] = g;
  }
  __syncthreads();
  if (tid < OUT_PTS) {
    const int h = tid / P3;
    const int pc = tid - h * P3;
    const int p = pc / 3, c = pc - p * 3;
    // local = (global - t) . R^T  -> l_c = sum_d (g_d - t_d) * R[c][d]
    const float* R = rot + (b * (long)n + i) * 9;
    const float* T = trans + (b * (long)n + i) * 3;
    float l = 0.f;
#pragma unroll
    for (int d = 0; d < 3; ++d)
      l += (gpts[(h * P + p) * 3 + d] - T[d]) * R[c * 3 + d];
    orow[OUT_SCALAR + OUT_PAIR + tid] = l;
    // norms: the c==0 thread recomputes all 3 local components (cheap,
    // avoids another barrier)
    if (c == 0) {
      float nrm = 0.f;
#pragma unroll
      for (int cc = 0; cc < 3; ++cc) {
        float lc = 0.f;
#pragma unroll
        for (int d = 0; d < 3; ++d)
          lc += (gpts[(h * P + p) * 3 + d] - T[d]) * R[cc * 3 + d];
        nrm += lc * lc;
      }
      orow[OUT_SCALAR + OUT_PAIR + OUT_PTS + h * P + p] =
          sqrtf(nrm + eps);
    }
  }
}

// ---- backward, row side: one block per (b, i) ------------------------
//   dout: (b, n, DOUT) incoming gradient, attn: saved A, gsave: saved
//   aggregated global points.  Writes
//   dq_s (b,n,H,DS), dq_pg (b,n,H,P,3), dbias (b,H,n,n) = s_b * dL,
//   dg (b,n,H*P*3) for the column kernel, dpw_part (b*n, H) = sum_j dL*d2,
//   dtrans (b,n,3), and when non-null dpair (b,n,n,DP) and drot (b,n,3,3).
template <int H>
__global__ __launch_bounds__(NT)
void ipa_core_bwd_row_kernel(const float* __restrict__ dout,
                             const float* __restrict__ attn,
                             const float* __restrict__ gsave,
                             const float* __restrict__ q_pg,
                             const float* __restrict__ k_s,
                             const float* __restrict__ v_s,
                             const float* __restrict__ k_pg,
                             const float* __restrict__ v_pg,
                             const float* __restrict__ pair,
                             const float* __restrict__ rot,
                             const float* __restrict__ trans,
                             const float* __restrict__ point_w,
                             const unsigned char* __restrict__ mask,
                             float* __restrict__ dq_s,
                             float* __restrict__ dq_pg,
                             float* __restrict__ dbias,
                             float* __restrict__ dg_out,
                             float* __restrict__ dpw_part,
                             float* __restrict__ dtrans,
                             float* __restrict__ dpair,
                             float* __restrict__ drot,
                             int n, int DP, float scale_s, float scale_b,
                             float scale_p, float eps) {
  extern __shared__ float smem[];
  float* dop = smem;                    // do_pair[i]: [H][DP], 16-B aligned
  float* A = dop + H * DP;              // [H][n]
  float* dL = A + H * n;                // [H][n]: dA, then dL in place
  float* qpts = dL + H * n;             // q_pg[i]: [H*P*3]
  float* dos = qpts + H * P3;           // do_s[i]: [H*DV]
  float* dg = dos + H * DV;             // [H*P*3] grad of global points
  float* dl = dg + H * P3;              // [H*P*3] grad of local points
  float* grel = dl + H * P3;            // [H*P*3] g - t
  float* red = grel + H * P3;           // [NW][H]

  constexpr int OUT_SCALAR = H * DV;
  constexpr int OUT_PTS = H * P3;
  const int OUT_PAIR = H * DP;
  const int DOUT = OUT_SCALAR + OUT_PAIR + OUT_PTS + H * P;

  const long bi = blockIdx.x;           // b * n + i
  const long b = bi / n;
  const int i = bi - b * n;
  const int tid = threadIdx.x;
  const float* dorow = dout + bi * (long)DOUT;

  // ---- stage the row -------------------------------------------------
  for (int c = tid; c < H * DP; c += NT) dop[c] = dorow[OUT_SCALAR + c];
  for (int c = tid; c < H * DV; c += NT) dos[c] = dorow[c];
  for (int c = tid; c < H * P3; c += NT)
    qpts[c] = q_pg[bi * (long)H * P3 + c];
  for (int h = 0; h < H; ++h) {
    const float* arow = attn + ((b * H + h) * (long)n + i) * n;
    for (int j = tid; j < n; j += NT) A[h * n + j] = arow[j];
  }
  // output-side frame transform: l = (g - t) R^T, nrm = sqrt(|l|^2 + eps)
  if (tid < H * P) {
    const float* R = rot + bi * 9;
    const float* T = trans + bi * 3;
    const float* dop_pts = dorow + OUT_SCALAR + OUT_PAIR;
    float rel[3], l[3], dlc[3];
    float nrm = 0.f;
#pragma unroll
    for (int d = 0; d < 3; ++d)
      rel[d] = gsave[bi * (long)OUT_PTS + tid * 3 + d] - T[d];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      l[c] = rel[0] * R[c * 3] + rel[1] * R[c * 3 + 1] + rel[2] * R[c * 3 + 2];
      nrm += l[c] * l[c];
    }
    nrm = sqrtf(nrm + eps);
    const float don = dop_pts[OUT_PTS + tid] / nrm;
#pragma unroll
    for (int c = 0; c < 3; ++c) dlc[c] = dop_pts[tid * 3 + c] + don * l[c];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const float v = dlc[0] * R[d] + dlc[1] * R[3 + d] + dlc[2] * R[6 + d];
      dg[tid * 3 + d] = v;
      dg_out[bi * (long)OUT_PTS + tid * 3 + d] = v;
      dl[tid * 3 + d] = dlc[d];
      grel[tid * 3 + d] = rel[d];
    }
  }
  __syncthreads();

  // dR[c][d] = sum_{h,p} dl_c (g_d - t_d);  dt_d = -sum_{h,p} dg_d
  if (tid < 9) {
    if (drot) {
      const int c = tid / 3, d = tid - c * 3;
      float acc = 0.f;
      for (int hp = 0; hp < H * P; ++hp)
        acc += dl[hp * 3 + c] * grel[hp * 3 + d];
      drot[bi * 9 + tid] = acc;
    }
  } else if (tid < 12) {
    const int d = tid - 9;
    float acc = 0.f;
    for (int hp = 0; hp < H * P; ++hp) acc += dg[hp * 3 + d];
    dtrans[bi * 3 + d] = -acc;
  }

  // ---- dA, value part: thread owns column j --------------------------
  for (int j = tid; j < n; j += NT) {
    const float* vrow = v_s + (b * (long)n + j) * H * DV;
    const float* vpts = v_pg + (b * (long)n + j) * (long)H * P3;
#pragma unroll
    for (int h = 0; h < H; ++h) {
      float acc = 0.f;
#pragma unroll
      for (int d = 0; d < DV; ++d) acc += dos[h * DV + d] * vrow[h * DV + d];
#pragma unroll
      for (int d = 0; d < P3; ++d) acc += dg[h * P3 + d] * vpts[h * P3 + d];
      dL[h * n + j] = acc;
    }
  }
  __syncthreads();

  // ---- dA, pair part: 16 lanes own column j, float4 over channels ----
  {
    const int grp = tid >> 4, l16 = tid & 15;
    const float* prow = pair + bi * (long)n * DP;
    for (int j0 = 0; j0 < n; j0 += NT / 16) {
      const int j = j0 + grp;
      const bool valid = j < n;
      float acc[H];
#pragma unroll
      for (int h = 0; h < H; ++h) acc[h] = 0.f;
      for (int c = l16 * 4; c < DP; c += 64) {
        float4 pv = make_float4(0.f, 0.f, 0.f, 0.f);
        if (valid)
          pv = *reinterpret_cast<const float4*>(prow + (long)j * DP + c);
#pragma unroll
        for (int h = 0; h < H; ++h) {
          const float4 dv = *reinterpret_cast<const float4*>(dop + h * DP + c);
          acc[h] += pv.x * dv.x + pv.y * dv.y + pv.z * dv.z + pv.w * dv.w;
        }
      }
#pragma unroll
      for (int h = 0; h < H; ++h) {
#pragma unroll
        for (int off = 8; off > 0; off >>= 1)
          acc[h] += __shfl_xor(acc[h], off, 64);
      }
      if (valid && l16 == 0) {
#pragma unroll
        for (int h = 0; h < H; ++h) dL[h * n + j] += acc[h];
      }
    }
  }
  __syncthreads();

  // ---- delta_h = sum_j A dA -------------------------------------------
  float delta[H];
#pragma unroll
  for (int h = 0; h < H; ++h) {
    delta[h] = 0.f;
    for (int j = tid; j < n; j += NT) delta[h] += A[h * n + j] * dL[h * n + j];
  }
  block_reduce_heads<H>(delta, red);

  // ---- dL = A (dA - delta), zero where masked; dbias; dpoint_w part --
  const bool mi = mask ? mask[bi] != 0 : true;
  float pw[H];
#pragma unroll
  for (int h = 0; h < H; ++h) pw[h] = 0.f;
  for (int j = tid; j < n; j += NT) {
    const float* kpts = k_pg + (b * (long)n + j) * (long)H * P3;
    const bool valid = mi && (mask ? mask[b * n + j] != 0 : true);
#pragma unroll
    for (int h = 0; h < H; ++h) {
      float d2 = 0.f;
#pragma unroll
      for (int d = 0; d < P3; ++d) {
        const float dd = qpts[h * P3 + d] - kpts[h * P3 + d];
        d2 += dd * dd;
      }
      const float v = valid ? A[h * n + j] * (dL[h * n + j] - delta[h]) : 0.f;
      dL[h * n + j] = v;
      pw[h] += v * d2;
      dbias[((b * H + h) * (long)n + i) * n + j] = v * scale_b;
    }
  }
  block_reduce_heads<H>(pw, red);     // also orders the dL writes
  if (tid == 0) {
#pragma unroll
    for (int h = 0; h < H; ++h) dpw_part[bi * H + h] = pw[h];
  }

  // ---- dq_s, dq_pg: thread owns one channel, loops over j ------------
  if (tid < H * DS) {
    const int h = tid / DS;
    float acc = 0.f;
    for (int j = 0; j < n; ++j)
      acc += dL[h * n + j] * k_s[(b * (long)n + j) * H * DS + tid];
    dq_s[bi * H * DS + tid] = acc * scale_s;
  } else if (tid < H * DS + H * P3) {
    const int r = tid - H * DS;
    const int h = r / P3;
    const float qv = qpts[r];
    float acc = 0.f;
    for (int j = 0; j < n; ++j)
      acc += dL[h * n + j] * (qv - k_pg[(b * (long)n + j) * (long)H * P3 + r]);
    dq_pg[bi * (long)H * P3 + r] = -point_w[h] * scale_p * acc;
  }

  // ---- dpair[i,j,c] = sum_h A[h,j] do_pair[h,c] -----------------------
  if (dpair) {
    float* drow = dpair + bi * (long)n * DP;
    const int total4 = n * (DP / 4);
    for (int idx = tid; idx < total4; idx += NT) {
      const int e = idx * 4;
      const int j = e / DP, c = e - j * DP;
      float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int h = 0; h < H; ++h) {
        const float a = A[h * n + j];
        const float4 dv = *reinterpret_cast<const float4*>(dop + h * DP + c);
        o.x += a * dv.x; o.y += a * dv.y; o.z += a * dv.z; o.w += a * dv.w;
      }
      *reinterpret_cast<float4*>(drow + e) = o;
    }
  }
}

// ---- backward, column side: one block per (b, j) ---------------------
//   dk_s[j]  = (s_s/s_b) sum_i dbias[i,j] q_s[i]
//   dk_pg[j] = (w s_p/s_b) sum_i dbias[i,j] (q_pg[i] - k_pg[j])
//   dv_s[j]  = sum_i A[i,j] do_s[i]      dv_pg[j] = sum_i A[i,j] dg[i]
template <int H>
__global__ __launch_bounds__(NT)
void ipa_core_bwd_col_kernel(const float* __restrict__ dout,
                             const float* __restrict__ attn,
                             const float* __restrict__ dbias,
                             const float* __restrict__ dg,
                             const float* __restrict__ q_s,
                             const float* __restrict__ q_pg,
                             const float* __restrict__ k_pg,
                             const float* __restrict__ point_w,
                             float* __restrict__ dk_s,
                             float* __restrict__ dk_pg,
                             float* __restrict__ dv_s,
                             float* __restrict__ dv_pg,
                             int n, int DP, float ks_scale, float kp_scale) {
  extern __shared__ float smem[];
  float* colA = smem;                   // A[h][i] for this column
  float* colL = colA + H * n;           // dbias[h][i] for this column

  const int DOUT = H * (DV + DP + P3 + P);
  const long bj = blockIdx.x;           // b * n + j
  const long b = bj / n;
  const int j = bj - b * n;
  const int tid = threadIdx.x;

  for (int idx = tid; idx < H * n; idx += NT) {
    const int h = idx / n, i = idx - h * n;
    const long off = ((b * H + h) * (long)n + i) * n + j;
    colA[idx] = attn[off];
    colL[idx] = dbias[off];
  }
  __syncthreads();

  constexpr int R0 = H * DS;            // dk_s roles
  constexpr int R1 = R0 + H * P3;       // dk_pg
  constexpr int R2 = R1 + H * DV;       // dv_s
  constexpr int R3 = R2 + H * P3;       // dv_pg
  for (int r = tid; r < R3; r += NT) {
    float acc = 0.f;
    if (r < R0) {
      const int h = r / DS;
      for (int i = 0; i < n; ++i)
        acc += colL[h * n + i] * q_s[(b * (long)n + i) * H * DS + r];
      dk_s[bj * H * DS + r] = acc * ks_scale;
    } else if (r < R1) {
      const int c = r - R0;
      const int h = c / P3;
      const float kv = k_pg[bj * (long)H * P3 + c];
      for (int i = 0; i < n; ++i)
        acc += colL[h * n + i]
            * (q_pg[(b * (long)n + i) * (long)H * P3 + c] - kv);
      dk_pg[bj * (long)H * P3 + c] = acc * point_w[h] * kp_scale;
    } else if (r < R2) {
      const int c = r - R1;
      const int h = c / DV;
      for (int i = 0; i < n; ++i)
        acc += colA[h * n + i] * dout[(b * (long)n + i) * DOUT + c];
      dv_s[bj * H * DV + c] = acc;
    } else {
      const int c = r - R2;
      const int h = c / P3;
      for (int i = 0; i < n; ++i)
        acc += colA[h * n + i] * dg[(b * (long)n + i) * (long)H * P3 + c];
      dv_pg[bj * (long)H * P3 + c] = acc;
    }
  }
}

// ---- host side --------------------------------------------------------

// dynamic LDS (bytes) of the three kernels
long fwd_lds_bytes(int H, int n) {
  return (long)(H * (long)n + H * DS + H * P3 + H * NW + H * P3)
      * sizeof(float);
}
long bwd_row_lds_bytes(int H, int n, int DP) {
  return (long)(H * DP + 2L * H * n + 4 * H * P3 + H * DV + NW * H)
      * sizeof(float);
}
long bwd_col_lds_bytes(int H, int n) {
  return 2L * H * n * sizeof(float);
}

// LDS one workgroup may use on the current device, opt-in included
long device_lds_limit() {
  int dev = 0, base = 0, optin = 0;
  TORCH_CHECK(hipGetDevice(&dev) == hipSuccess, "ipa_core: hipGetDevice");
  TORCH_CHECK(hipDeviceGetAttribute(
                  &base, hipDeviceAttributeMaxSharedMemoryPerBlock, dev)
              == hipSuccess, "ipa_core: LDS size query failed");
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
              " B of LDS per block, the device allows ", device_lds_limit(),
              " (n is above ipa_core_max_n)");
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

void check_f32(const at::Tensor& t, const char* what) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kFloat
              && t.is_contiguous(), what,
              ": fp32 contiguous device tensors required");
}

struct Dims { int b, n, H, DP; };

Dims check_dims(const at::Tensor& q_s, const at::Tensor& k_s,
                const at::Tensor& v_s, const at::Tensor& q_pg,
                const at::Tensor& k_pg, const at::Tensor& v_pg,
                const at::Tensor& bias, const at::Tensor& pair,
                const at::Tensor& rot, const at::Tensor& trans,
                const at::Tensor& point_w,
                const c10::optional<at::Tensor>& mask, const char* what) {
  for (const at::Tensor* t : {&q_s, &k_s, &v_s, &q_pg, &k_pg, &v_pg, &bias,
                              &pair, &rot, &trans, &point_w})
    check_f32(*t, what);
  TORCH_CHECK(q_s.dim() == 4 && pair.dim() == 4, what, ": bad ranks");
  const long b = q_s.size(0), n = q_s.size(1), H = q_s.size(2);
  const long DP = pair.size(3);
  TORCH_CHECK(H >= 1 && H <= MAX_H, what, ": heads must be 1..8");
  TORCH_CHECK(DP % 64 == 0 && DP >= 64 && DP <= MAX_DP, what,
              ": pair dim must be a multiple of 64 up to 512");
  TORCH_CHECK(b * n > 0 && b * n < (1L << 31) && b * H * n * n < (1L << 40),
              what, ": bad batch / length");
  auto is = [](const at::Tensor& t, at::IntArrayRef s) {
    return t.sizes() == s;
  };
  TORCH_CHECK(is(q_s, {b, n, H, DS}) && is(k_s, {b, n, H, DS})
              && is(v_s, {b, n, H, DV}) && is(q_pg, {b, n, H, P, 3})
              && is(k_pg, {b, n, H, P, 3}) && is(v_pg, {b, n, H, P, 3})
              && is(bias, {b, H, n, n}) && is(pair, {b, n, n, DP})
              && is(rot, {b, n, 3, 3}) && is(trans, {b, n, 3})
              && is(point_w, {H}),
              what, ": shapes do not match (scalar 16/16, points 4/4)");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(pair.data_ptr()) % 16 == 0, what,
              ": pair must be 16-byte aligned");
  if (mask.has_value()) {
    TORCH_CHECK(mask->is_cuda() && mask->scalar_type() == at::kBool
                && mask->is_contiguous() && is(*mask, {b, n}),
                what, ": mask must be a contiguous (b, n) bool tensor");
  }
  return {(int)b, (int)n, (int)H, (int)DP};
}

const unsigned char* mask_ptr(const c10::optional<at::Tensor>& mask) {
  return mask.has_value()
      ? reinterpret_cast<const unsigned char*>(mask->data_ptr<bool>())
      : nullptr;
}

#define IPA_DISPATCH_HEADS(H_RT, ...)                                  \
  switch (H_RT) {                                                      \
    case 1: { constexpr int H = 1; __VA_ARGS__; break; }               \
    case 2: { constexpr int H = 2; __VA_ARGS__; break; }               \
    case 3: { constexpr int H = 3; __VA_ARGS__; break; }               \
    case 4: { constexpr int H = 4; __VA_ARGS__; break; }               \
    case 5: { constexpr int H = 5; __VA_ARGS__; break; }               \
    case 6: { constexpr int H = 6; __VA_ARGS__; break; }               \
    case 7: { constexpr int H = 7; __VA_ARGS__; break; }               \
    case 8: { constexpr int H = 8; __VA_ARGS__; break; }               \
    default: TORCH_CHECK(false, "ipa_core: heads must be 1..8");       \
  }

}  // namespace

// Largest n for which forward AND backward fit the device's LDS at this
// head count (the row-side backward is the largest user).
long ipa_core_max_n(long heads, long pair_dim) {
  TORCH_CHECK(heads >= 1 && heads <= MAX_H, "ipa_core_max_n: heads 1..8");
  TORCH_CHECK(pair_dim >= 64 && pair_dim <= MAX_DP,
              "ipa_core_max_n: pair dim 64..512");
  const long fixed = bwd_row_lds_bytes(heads, 0, pair_dim);
  const long n = (device_lds_limit() - fixed)
      / (2L * heads * (long)sizeof(float));
  return n > 0 ? n : 0;
}

// Returns {out (b,n,DOUT), attn (b,H,n,n), gpts (b,n,H*P*3)}; the last
// two are empty unless save_stats.
std::vector<at::Tensor> ipa_core_fwd(
    at::Tensor q_s, at::Tensor k_s, at::Tensor v_s, at::Tensor q_pg,
    at::Tensor k_pg, at::Tensor v_pg, at::Tensor bias, at::Tensor pair,
    at::Tensor rot, at::Tensor trans, at::Tensor point_w, double scale_s,
    double scale_b, double scale_p, double eps,
    c10::optional<at::Tensor> mask, bool save_stats) {
  const Dims d = check_dims(q_s, k_s, v_s, q_pg, k_pg, v_pg, bias, pair,
                            rot, trans, point_w, mask, "ipa_core_fwd");
  const long dout = (long)d.H * (DV + d.DP + P3 + P);
  auto out = at::empty({d.b, d.n, dout}, q_s.options());
  auto attn = save_stats ? at::empty({d.b, d.H, d.n, d.n}, q_s.options())
                         : at::empty({0}, q_s.options());
  auto gpts = save_stats ? at::empty({d.b, d.n, (long)d.H * P3},
                                     q_s.options())
                         : at::empty({0}, q_s.options());
  const long smem = fwd_lds_bytes(d.H, d.n);
  auto stream = at::cuda::getCurrentHIPStream();
  IPA_DISPATCH_HEADS(d.H, {
    prepare_launch(ipa_core_kernel<H>, smem, "ipa_core_fwd");
    hipLaunchKernelGGL(ipa_core_kernel<H>, dim3((long)d.b * d.n), dim3(NT),
                       smem, stream,
                       q_s.data_ptr<float>(), k_s.data_ptr<float>(),
                       v_s.data_ptr<float>(), q_pg.data_ptr<float>(),
                       k_pg.data_ptr<float>(), v_pg.data_ptr<float>(),
                       bias.data_ptr<float>(), pair.data_ptr<float>(),
                       rot.data_ptr<float>(), trans.data_ptr<float>(),
                       point_w.data_ptr<float>(), mask_ptr(mask),
                       out.data_ptr<float>(),
                       save_stats ? attn.data_ptr<float>() : nullptr,
                       save_stats ? gpts.data_ptr<float>() : nullptr,
                       d.n, d.DP, (float)scale_s, (float)scale_b,
                       (float)scale_p, (float)eps);
  });
  check_launch("ipa_core_fwd");
  return {out, attn, gpts};
}

// Gradients of the eleven core inputs, in input order:
//   {dq_s, dk_s, dv_s, dq_pg, dk_pg, dv_pg, dbias, dpair, drot, dtrans,
//    dpoint_w}; dpair / drot are empty tensors when not requested.
std::vector<at::Tensor> ipa_core_bwd(
    at::Tensor dout, at::Tensor attn, at::Tensor gpts, at::Tensor q_s,
    at::Tensor k_s, at::Tensor v_s, at::Tensor q_pg, at::Tensor k_pg,
    at::Tensor v_pg, at::Tensor bias, at::Tensor pair, at::Tensor rot,
    at::Tensor trans, at::Tensor point_w, double scale_s, double scale_b,
    double scale_p, double eps, c10::optional<at::Tensor> mask,
    bool need_dpair, bool need_drot) {
  const Dims d = check_dims(q_s, k_s, v_s, q_pg, k_pg, v_pg, bias, pair,
                            rot, trans, point_w, mask, "ipa_core_bwd");
  const long DOUT = (long)d.H * (DV + d.DP + P3 + P);
  check_f32(dout, "ipa_core_bwd");
  check_f32(attn, "ipa_core_bwd");
  check_f32(gpts, "ipa_core_bwd");
  TORCH_CHECK(dout.sizes() == at::IntArrayRef({d.b, d.n, DOUT})
              && attn.sizes() == bias.sizes()
              && gpts.sizes() == at::IntArrayRef({d.b, d.n, (long)d.H * P3}),
              "ipa_core_bwd: dout / saved statistics shapes do not match");

  auto opt = q_s.options();
  auto dq_s = at::empty_like(q_s), dk_s = at::empty_like(k_s);
  auto dv_s = at::empty_like(v_s), dq_pg = at::empty_like(q_pg);
  auto dk_pg = at::empty_like(k_pg), dv_pg = at::empty_like(v_pg);
  auto dbias = at::empty_like(bias);
  auto dpair = need_dpair ? at::empty_like(pair) : at::empty({0}, opt);
  auto drot = need_drot ? at::empty_like(rot) : at::empty({0}, opt);
  auto dtrans = at::empty_like(trans);
  auto dg = at::empty_like(gpts);
  auto dpw_part = at::empty({(long)d.b * d.n, (long)d.H}, opt);

  const long smem_row = bwd_row_lds_bytes(d.H, d.n, d.DP);
  const long smem_col = bwd_col_lds_bytes(d.H, d.n);
  auto stream = at::cuda::getCurrentHIPStream();
  IPA_DISPATCH_HEADS(d.H, {
    prepare_launch(ipa_core_bwd_row_kernel<H>, smem_row, "ipa_core_bwd");
    hipLaunchKernelGGL(ipa_core_bwd_row_kernel<H>, dim3((long)d.b * d.n),
                       dim3(NT), smem_row, stream,
                       dout.data_ptr<float>(), attn.data_ptr<float>(),
                       gpts.data_ptr<float>(), q_pg.data_ptr<float>(),
                       k_s.data_ptr<float>(), v_s.data_ptr<float>(),
                       k_pg.data_ptr<float>(), v_pg.data_ptr<float>(),
                       pair.data_ptr<float>(), rot.data_ptr<float>(),
                       trans.data_ptr<float>(), point_w.data_ptr<float>(),
                       mask_ptr(mask), dq_s.data_ptr<float>(),
                       dq_pg.data_ptr<float>(), dbias.data_ptr<float>(),
                       dg.data_ptr<float>(), dpw_part.data_ptr<float>(),
                       dtrans.data_ptr<float>(),
                       need_dpair ? dpair.data_ptr<float>() : nullptr,
                       need_drot ? drot.data_ptr<float>() : nullptr,
                       d.n, d.DP, (float)scale_s, (float)scale_b,
                       (float)scale_p, (float)eps);
    check_launch("ipa_core_bwd (row side)");
    prepare_launch(ipa_core_bwd_col_kernel<H>, smem_col, "ipa_core_bwd");
    hipLaunchKernelGGL(ipa_core_bwd_col_kernel<H>, dim3((long)d.b * d.n),
                       dim3(NT), smem_col, stream,
                       dout.data_ptr<float>(), attn.data_ptr<float>(),
                       dbias.data_ptr<float>(), dg.data_ptr<float>(),
                       q_s.data_ptr<float>(), q_pg.data_ptr<float>(),
                       k_pg.data_ptr<float>(), point_w.data_ptr<float>(),
                       dk_s.data_ptr<float>(), dk_pg.data_ptr<float>(),
                       dv_s.data_ptr<float>(), dv_pg.data_ptr<float>(),
                       d.n, d.DP, (float)(scale_s / scale_b),
                       (float)(scale_p / scale_b));
    check_launch("ipa_core_bwd (column side)");
  });
  // fold the per-row partials: dpoint_w[h] = -0.5 s_p sum_{b,i,j} dL d2
  auto dpoint_w = dpw_part.sum(0).mul_(-0.5 * scale_p);
  return {dq_s, dk_s, dv_s, dq_pg, dk_pg, dv_pg, dbias, dpair, drot,
          dtrans, dpoint_w};
}
