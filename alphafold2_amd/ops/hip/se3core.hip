// Fused fp32 SE(3) refiner attention core — gfx950 (K15: the attention
// half of models/equivariant.py SE3RefinerLayer).
//
//   rel_ij   = x_i - x_j            d2_ij = |rel_ij|^2
//   L[h,i,j] = scale q_ih.k_jh + sum_c w_e[h,c] edges[i,j,c]
//              + w_e[h,E] d2_ij + b_e[h]        (-FLT_MAX where !mask[j])
//   A        = softmax_j L
//   out_ih   = sum_j A[h,i,j] v_jh
//   dxh_ih   = sum_j A[h,i,j] rel_ij / sqrt(d2_ij + eps)
//
// Forward: one block per query row (b,i) with the H*n logits in LDS; the
// pair-bias Linear is folded in by streaming edges[b,i,:,:] once (float4
// per lane, lanes span channels, shuffle reduction to the H sums), so
// neither cat([edges, dist2]) nor rel / rel_norm / bias / logits exist in
// memory.  fp32 VALU: one row against n keys is not a matrix-core tile.
// Heads 1..8 (template), dim_head any multiple of 4 up to 64 and edge dim
// any multiple of 64 up to 512 (both runtime).
//
// Backward: two deterministic kernels, no float atomics.
//   row side    one block per (b,i): dA, delta, dL; owns dq, dedges, the
//               i-side of dx, dL (b,H,n,n) for the column side and the
//               per-block partials of dw_e / db_e (folded by a sum)
//   column side one block per (b,j): stages the A and dL columns; owns
//               dk, dv and the j-side of dx, and writes dx = both sides
// The rel_norm path of dx skips j == i: rel_ii == 0 makes that term
// cancel analytically, while adding and subtracting u / sqrt(eps) in two
// separate reductions would leave 1e4-scaled rounding noise behind.
// The forward saves the probabilities A (b,H,n,n) when a gradient is
// required; nothing else of pair size is kept.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <cfloat>
#include <cstdint>

#include "common.h"

namespace {

constexpr int NT = 256;     // threads per block
constexpr int NW = NT / 64; // waves per block
constexpr int MAX_H = 8;
constexpr int MAX_DH = 64;  // dim_head: multiple of 4, <= 64
constexpr int MAX_E = 512;  // edge dim: multiple of 64, <= 512

// rows of the [H][n] LDS arrays are padded to a multiple of 4 floats so
// that every carve offset stays 16-byte aligned
__host__ __device__ constexpr int pad4(int n) { return (n + 3) & ~3; }

// Block-wide sum of N per-thread values; the totals come back in v[] on
// every thread.  `red` holds NW * N floats.
template <int N>
__device__ __forceinline__ void block_reduce_vals(float (&v)[N], float* red) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    v[k] = wave_reduce_sum(v[k]);
    if (lane == 0) red[wave * N + k] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < N; ++k) {
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) t += red[w * N + k];
    v[k] = t;
  }
  __syncthreads();
}

// dst[c] = alpha * sum_j W[(c / dh) * np + j] * mat[j * C + c] for the
// C = H * dh channels of one row.  W is an [H][np] LDS array, mat a
// (n, C) global matrix.  When C <= NT the NT / C thread groups split j
// and fold through `part` (NT floats); the group order is fixed, so the
// sum is deterministic.  Every thread of the block must call this.
__device__ __forceinline__ void heads_row_matvec(
    const float* W, int np, int n, const float* __restrict__ mat, int C,
    int dh, float alpha, float* __restrict__ dst, float* part) {
  const int tid = threadIdx.x;
  if (C <= NT) {
    const int G = NT / C;
    const int g = tid / C, c = tid - g * C;
    float acc = 0.f;
    if (g < G) {
      const float* w = W + (c / dh) * np;
      for (int j = g; j < n; j += G) acc += w[j] * mat[(long)j * C + c];
    }
    part[tid] = acc;
    __syncthreads();
    if (tid < C) {
      float t = 0.f;
      for (int gg = 0; gg < G; ++gg) t += part[gg * C + tid];
      dst[tid] = alpha * t;
    }
    __syncthreads();
  } else {
    for (int c = tid; c < C; c += NT) {
      const float* w = W + (c / dh) * np;
      float acc = 0.f;
      for (int j = 0; j < n; ++j) acc += w[j] * mat[(long)j * C + c];
      dst[c] = alpha * acc;
    }
  }
}

// inputs (all fp32, contiguous):
//   q, k, v: (b, n, H*dh) as the Linears produce them (head h owns
//            channels [h*dh, (h+1)*dh))
//   x: (b, n, 3)   edges: (b, n, n, E)   w_e: (H, E+1)   b_e: (H)
//   mask: (b, n) bytes or null; logits of key j with !mask[j] become
//         -FLT_MAX, so a row whose keys are all masked gets the uniform
//         1/n softmax
//   out: (b, n, H*dh)   dxh: (b, n, H, 3)
//   attn_save (b, H, n, n): null when no gradient is required
template <int H>
__global__ __launch_bounds__(NT)
void se3_core_fwd_kernel(const float* __restrict__ q,
                         const float* __restrict__ k,
                         const float* __restrict__ v,
                         const float* __restrict__ x,
                         const float* __restrict__ edges,
                         const float* __restrict__ w_e,
                         const float* __restrict__ b_e,
                         const unsigned char* __restrict__ mask,
                         float* __restrict__ out,
                         float* __restrict__ dxh,
                         float* __restrict__ attn_save,
                         int n, int dh, int E, float scale, float eps) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int np = pad4(n);
  const int C = H * dh;
  float* we = smem;                     // w_e[:, :E]: [H][E]
  float* qrow = we + H * E;             // q[i]: [C]
  float* logits = qrow + C;             // [H][np]
  float* part = logits + H * np;        // [NT]
  float* red = part + NT;               // [NW][3H]

  const long bi = blockIdx.x;           // b * n + i
  const long b = bi / n;
  const int i = bi - b * n;
  const int tid = threadIdx.x;

  for (int idx = tid; idx < H * E; idx += NT) {
    const int h = idx / E, c = idx - h * E;
    we[idx] = w_e[h * (E + 1) + c];
  }
  for (int c = tid; c < C; c += NT) qrow[c] = q[bi * C + c];
  float wd[H], be[H];
#pragma unroll
  for (int h = 0; h < H; ++h) {
    wd[h] = w_e[h * (E + 1) + E];
    be[h] = b_e[h];
  }
  const float xi0 = x[bi * 3], xi1 = x[bi * 3 + 1], xi2 = x[bi * 3 + 2];
  __syncthreads();

  // ---- pass 1a: scalar qk + distance term, thread owns column j -------
  for (int j = tid; j < n; j += NT) {
    const long bj = b * n + j;
    const float* krow = k + bj * C;
    const float r0 = xi0 - x[bj * 3], r1 = xi1 - x[bj * 3 + 1],
                r2 = xi2 - x[bj * 3 + 2];
    const float d2 = r0 * r0 + r1 * r1 + r2 * r2;
#pragma unroll
    for (int h = 0; h < H; ++h) {
      float dot = 0.f;
      for (int d = 0; d < dh; d += 4) {
        const float4 kk = *reinterpret_cast<const float4*>(krow + h * dh + d);
        const float4 qq = *reinterpret_cast<const float4*>(qrow + h * dh + d);
        dot += qq.x * kk.x + qq.y * kk.y + qq.z * kk.z + qq.w * kk.w;
      }
      logits[h * np + j] = dot * scale + wd[h] * d2 + be[h];
    }
  }
  __syncthreads();

  // ---- pass 1b: edge bias; 16 lanes own column j, float4 over channels
  {
    const int grp = tid >> 4, l16 = tid & 15;
    const float* erow = edges + bi * (long)n * E;
    for (int j0 = 0; j0 < n; j0 += NT / 16) {
      const int j = j0 + grp;
      const bool inb = j < n;
      float acc[H];
#pragma unroll
      for (int h = 0; h < H; ++h) acc[h] = 0.f;
      for (int c = l16 * 4; c < E; c += 64) {
        float4 pv = make_float4(0.f, 0.f, 0.f, 0.f);
        if (inb)
          pv = *reinterpret_cast<const float4*>(erow + (long)j * E + c);
#pragma unroll
        for (int h = 0; h < H; ++h) {
          const float4 wv = *reinterpret_cast<const float4*>(we + h * E + c);
          acc[h] += pv.x * wv.x + pv.y * wv.y + pv.z * wv.z + pv.w * wv.w;
        }
      }
#pragma unroll
      for (int h = 0; h < H; ++h) {
#pragma unroll
        for (int off = 8; off > 0; off >>= 1)
          acc[h] += __shfl_xor(acc[h], off, 64);
      }
      if (inb && l16 == 0) {
        const bool keep = mask ? mask[b * n + j] != 0 : true;
#pragma unroll
        for (int h = 0; h < H; ++h)
          logits[h * np + j] = keep ? logits[h * np + j] + acc[h] : -FLT_MAX;
      }
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
    for (int j = tid; j < n; j += NT) m = fmaxf(m, logits[h * np + j]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
      m = fmaxf(m, __shfl_down(m, off, 64));
    if (lane == 0) red[wave] = m;
    __syncthreads();
    m = red[0];
    for (int w = 1; w < NW; ++w) m = fmaxf(m, red[w]);
    __syncthreads();          // red[] reuse

    float s = 0.f;
    for (int j = tid; j < n; j += NT) {
      const float e = __expf(logits[h * np + j] - m);
      logits[h * np + j] = e;
      s += e;
    }
    s = wave_reduce_sum(s);
    if (lane == 0) red[wave] = s;
    __syncthreads();
    s = 0.f;
    for (int w = 0; w < NW; ++w) s += red[w];
    const float inv = 1.f / s;
    for (int j = tid; j < n; j += NT) logits[h * np + j] *= inv;
    __syncthreads();
  }

  if (attn_save) {
    for (int h = 0; h < H; ++h) {
      float* arow = attn_save + ((b * H + h) * (long)n + i) * n;
      for (int j = tid; j < n; j += NT) arow[j] = logits[h * np + j];
    }
  }

  // ---- pass 3: value aggregation and attention-weighted displacements
  heads_row_matvec(logits, np, n, v + b * (long)n * C, C, dh, 1.f,
                   out + bi * C, part);

  float dacc[3 * H];
#pragma unroll
  for (int t = 0; t < 3 * H; ++t) dacc[t] = 0.f;
  for (int j = tid; j < n; j += NT) {
    const long bj = b * n + j;
    const float r0 = xi0 - x[bj * 3], r1 = xi1 - x[bj * 3 + 1],
                r2 = xi2 - x[bj * 3 + 2];
    const float inv = 1.f / sqrtf(r0 * r0 + r1 * r1 + r2 * r2 + eps);
#pragma unroll
    for (int h = 0; h < H; ++h) {
      const float a = logits[h * np + j] * inv;
      dacc[h * 3] += a * r0;
      dacc[h * 3 + 1] += a * r1;
      dacc[h * 3 + 2] += a * r2;
    }
  }
  block_reduce_vals<3 * H>(dacc, red);
  if (tid == 0) {
#pragma unroll
    for (int t = 0; t < 3 * H; ++t) dxh[bi * 3 * H + t] = dacc[t];
  }
}

// ---- backward, row side: one block per (b, i) ------------------------
//   dout (b,n,H*dh), ddxh (b,n,H,3): incoming gradients; attn: saved A.
//   Writes dq (b,n,H*dh), dL (b,H,n,n), dx_row (b,n,3) = the i-side of
//   dx, dwe_part (b*n, H, E), dwd_part / dbe_part (b*n, H), and when
//   non-null dedges (b,n,n,E).
template <int H>
__global__ __launch_bounds__(NT)
void se3_core_bwd_row_kernel(const float* __restrict__ dout,
                             const float* __restrict__ ddxh,
                             const float* __restrict__ attn,
                             const float* __restrict__ k,
                             const float* __restrict__ v,
                             const float* __restrict__ x,
                             const float* __restrict__ edges,
                             const float* __restrict__ w_e,
                             const unsigned char* __restrict__ mask,
                             float* __restrict__ dq,
                             float* __restrict__ dL_out,
                             float* __restrict__ dx_row,
                             float* __restrict__ dwe_part,
                             float* __restrict__ dwd_part,
                             float* __restrict__ dbe_part,
                             float* __restrict__ dedges,
                             int n, int dh, int E, float scale, float eps) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int np = pad4(n);
  const int C = H * dh;
  float* dwl = smem;                    // dw_e partial of this row: [H][E]
  float* dorow = dwl + H * E;           // dout[i]: [C]
  float* A = dorow + C;                 // [H][np]
  float* dL = A + H * np;               // [H][np]: dA, then dL in place
  float* part = dL + H * np;            // [NT]
  float* red = part + NT;               // [NW][3H]
  float* ddx = red + NW * 3 * H;        // ddxh[i]: [3H]

  const long bi = blockIdx.x;           // b * n + i
  const long b = bi / n;
  const int i = bi - b * n;
  const int tid = threadIdx.x;

  // ---- stage the row -------------------------------------------------
  for (int c = tid; c < C; c += NT) dorow[c] = dout[bi * C + c];
  if (tid < 3 * H) ddx[tid] = ddxh[bi * 3 * H + tid];
  for (int h = 0; h < H; ++h) {
    const float* arow = attn + ((b * H + h) * (long)n + i) * n;
    for (int j = tid; j < n; j += NT) A[h * np + j] = arow[j];
  }
  float wd[H];
#pragma unroll
  for (int h = 0; h < H; ++h) wd[h] = w_e[h * (E + 1) + E];
  const float xi0 = x[bi * 3], xi1 = x[bi * 3 + 1], xi2 = x[bi * 3 + 2];
  __syncthreads();

  // ---- dA[h,j] = dout_ih.v_jh + ddxh_ih.rel_norm_ij; thread owns j ----
  for (int j = tid; j < n; j += NT) {
    const long bj = b * n + j;
    const float* vrow = v + bj * C;
    const float r0 = xi0 - x[bj * 3], r1 = xi1 - x[bj * 3 + 1],
                r2 = xi2 - x[bj * 3 + 2];
    const float inv = 1.f / sqrtf(r0 * r0 + r1 * r1 + r2 * r2 + eps);
#pragma unroll
    for (int h = 0; h < H; ++h) {
      float acc = 0.f;
      for (int d = 0; d < dh; d += 4) {
        const float4 vv = *reinterpret_cast<const float4*>(vrow + h * dh + d);
        const float4 dd = *reinterpret_cast<const float4*>(dorow + h * dh + d);
        acc += dd.x * vv.x + dd.y * vv.y + dd.z * vv.z + dd.w * vv.w;
      }
      acc += (ddx[h * 3] * r0 + ddx[h * 3 + 1] * r1 + ddx[h * 3 + 2] * r2)
          * inv;
      dL[h * np + j] = acc;
    }
  }
  __syncthreads();

  // ---- delta_h = sum_j A dA -------------------------------------------
  float delta[H];
#pragma unroll
  for (int h = 0; h < H; ++h) {
    delta[h] = 0.f;
    for (int j = tid; j < n; j += NT) delta[h] += A[h * np + j] * dL[h * np + j];
  }
  block_reduce_vals<H>(delta, red);

  // ---- dL = A (dA - delta), zero where masked; db_e / dist2-weight
  // partials; the i-side of dx -------------------------------------------
  float sb[H], sd[H], dxi[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int h = 0; h < H; ++h) sb[h] = sd[h] = 0.f;
  for (int j = tid; j < n; j += NT) {
    const long bj = b * n + j;
    const float r0 = xi0 - x[bj * 3], r1 = xi1 - x[bj * 3 + 1],
                r2 = xi2 - x[bj * 3 + 2];
    const float d2 = r0 * r0 + r1 * r1 + r2 * r2;
    const float inv = 1.f / sqrtf(d2 + eps);
    const bool keep = mask ? mask[bj] != 0 : true;
    float g = 0.f, u0 = 0.f, u1 = 0.f, u2 = 0.f;
#pragma unroll
    for (int h = 0; h < H; ++h) {
      const float a = A[h * np + j];
      const float l = keep ? a * (dL[h * np + j] - delta[h]) : 0.f;
      dL[h * np + j] = l;
      dL_out[((b * H + h) * (long)n + i) * n + j] = l;
      sb[h] += l;
      sd[h] += l * d2;
      g += l * wd[h];
      u0 += a * ddx[h * 3];
      u1 += a * ddx[h * 3 + 1];
      u2 += a * ddx[h * 3 + 2];
    }
    // dist2 path
    dxi[0] += 2.f * g * r0;
    dxi[1] += 2.f * g * r1;
    dxi[2] += 2.f * g * r2;
    // rel_norm path: drel = u/s - rel (rel.u)/s^3, without the diagonal
    if (j != i) {
      const float ru = (r0 * u0 + r1 * u1 + r2 * u2) * inv * inv * inv;
      dxi[0] += u0 * inv - r0 * ru;
      dxi[1] += u1 * inv - r1 * ru;
      dxi[2] += u2 * inv - r2 * ru;
    }
  }
  block_reduce_vals<H>(sb, red);        // also orders the dL writes
  block_reduce_vals<H>(sd, red);
  block_reduce_vals<3>(dxi, red);
  if (tid == 0) {
#pragma unroll
    for (int h = 0; h < H; ++h) {
      dbe_part[bi * H + h] = sb[h];
      dwd_part[bi * H + h] = sd[h];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) dx_row[bi * 3 + c] = dxi[c];
  }

  // ---- dq_i = scale sum_j dL k_j --------------------------------------
  heads_row_matvec(dL, np, n, k + b * (long)n * C, C, dh, scale,
                   dq + bi * C, part);

  // ---- one pass over edges[b,i,:,:]: E/4 lanes own a row j (float4 over
  // channels), NT / (E/4) rows in flight.  Each thread keeps its channels'
  // dw_e partial in registers and writes dedges[i,j,c] = sum_h dL w_e ----
  {
    const int tpr = E / 4;              // threads per row: 16..128
    const int R = NT / tpr;             // rows per sweep
    const int jg = tid / tpr;
    const int c = (tid - jg * tpr) * 4;
    const bool active = jg < R;
    float4 acc[H], wv[H];
#pragma unroll
    for (int h = 0; h < H; ++h) {
      acc[h] = make_float4(0.f, 0.f, 0.f, 0.f);
      wv[h] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (active) {
      if (dedges) {
#pragma unroll
        for (int h = 0; h < H; ++h) {
          const float* w = w_e + h * (E + 1) + c;   // rows are not 16-B aligned
          wv[h] = make_float4(w[0], w[1], w[2], w[3]);
        }
      }
      const float* erow = edges + bi * (long)n * E + c;
      float* drow = dedges ? dedges + bi * (long)n * E + c : nullptr;
      for (int j = jg; j < n; j += R) {
        const float4 pv = *reinterpret_cast<const float4*>(erow + (long)j * E);
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int h = 0; h < H; ++h) {
          const float l = dL[h * np + j];
          acc[h].x += l * pv.x; acc[h].y += l * pv.y;
          acc[h].z += l * pv.z; acc[h].w += l * pv.w;
          o.x += l * wv[h].x; o.y += l * wv[h].y;
          o.z += l * wv[h].z; o.w += l * wv[h].w;
        }
        if (drow) *reinterpret_cast<float4*>(drow + (long)j * E) = o;
      }
    }
    // fold the R row groups in a fixed order
    for (int r = 0; r < R; ++r) {
      if (active && jg == r) {
#pragma unroll
        for (int h = 0; h < H; ++h) {
          float4* p = reinterpret_cast<float4*>(dwl + h * E + c);
          float4 t = acc[h];
          if (r > 0) {
            const float4 s = *p;
            t.x += s.x; t.y += s.y; t.z += s.z; t.w += s.w;
          }
          *p = t;
        }
      }
      __syncthreads();
    }
    float* dst = dwe_part + bi * (long)H * E;
    for (int idx = tid * 4; idx < H * E; idx += NT * 4)
      *reinterpret_cast<float4*>(dst + idx) =
          *reinterpret_cast<const float4*>(dwl + idx);
  }
}

// ---- backward, column side: one block per (b, j) ---------------------
//   dk_j = scale sum_i dL[i,j] q_i       dv_j = sum_i A[i,j] dout_i
//   dx_j = dx_row_j - sum_i (2 g_ij rel_ij + drel_ij)
template <int H>
__global__ __launch_bounds__(NT)
void se3_core_bwd_col_kernel(const float* __restrict__ dout,
                             const float* __restrict__ ddxh,
                             const float* __restrict__ attn,
                             const float* __restrict__ dL,
                             const float* __restrict__ q,
                             const float* __restrict__ x,
                             const float* __restrict__ w_e,
                             const float* __restrict__ dx_row,
                             float* __restrict__ dk,
                             float* __restrict__ dv,
                             float* __restrict__ dx,
                             int n, int dh, int E, float scale, float eps) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int np = pad4(n);
  const int C = H * dh;
  float* colA = smem;                   // A[h][i] for this column
  float* colL = colA + H * np;          // dL[h][i] for this column
  float* part = colL + H * np;          // [NT]
  float* red = part + NT;               // [NW][3]

  const long bj = blockIdx.x;           // b * n + j
  const long b = bj / n;
  const int j = bj - b * n;
  const int tid = threadIdx.x;

  for (int h = 0; h < H; ++h) {
    for (int i = tid; i < n; i += NT) {
      const long off = ((b * H + h) * (long)n + i) * n + j;
      colA[h * np + i] = attn[off];
      colL[h * np + i] = dL[off];
    }
  }
  float wd[H];
#pragma unroll
  for (int h = 0; h < H; ++h) wd[h] = w_e[h * (E + 1) + E];
  const float xj0 = x[bj * 3], xj1 = x[bj * 3 + 1], xj2 = x[bj * 3 + 2];
  __syncthreads();

  heads_row_matvec(colL, np, n, q + b * (long)n * C, C, dh, scale,
                   dk + bj * C, part);
  heads_row_matvec(colA, np, n, dout + b * (long)n * C, C, dh, 1.f,
                   dv + bj * C, part);

  // ---- the j-side of dx: thread owns query i --------------------------
  float dxj[3] = {0.f, 0.f, 0.f};
  for (int i = tid; i < n; i += NT) {
    const long bi = b * n + i;
    const float r0 = x[bi * 3] - xj0, r1 = x[bi * 3 + 1] - xj1,
                r2 = x[bi * 3 + 2] - xj2;
    const float d2 = r0 * r0 + r1 * r1 + r2 * r2;
    const float inv = 1.f / sqrtf(d2 + eps);
    const float* dd = ddxh + bi * 3 * H;
    float g = 0.f, u0 = 0.f, u1 = 0.f, u2 = 0.f;
#pragma unroll
    for (int h = 0; h < H; ++h) {
      const float a = colA[h * np + i];
      g += colL[h * np + i] * wd[h];
      u0 += a * dd[h * 3];
      u1 += a * dd[h * 3 + 1];
      u2 += a * dd[h * 3 + 2];
    }
    dxj[0] -= 2.f * g * r0;
    dxj[1] -= 2.f * g * r1;
    dxj[2] -= 2.f * g * r2;
    if (i != j) {
      const float ru = (r0 * u0 + r1 * u1 + r2 * u2) * inv * inv * inv;
      dxj[0] -= u0 * inv - r0 * ru;
      dxj[1] -= u1 * inv - r1 * ru;
      dxj[2] -= u2 * inv - r2 * ru;
    }
  }
  block_reduce_vals<3>(dxj, red);
  if (tid == 0) {
#pragma unroll
    for (int c = 0; c < 3; ++c) dx[bj * 3 + c] = dx_row[bj * 3 + c] + dxj[c];
  }
}

// ---- host side --------------------------------------------------------

// dynamic LDS (bytes) of the three kernels; mirrors the carves above
long fwd_lds_bytes(long H, long n, long dh, long E) {
  return (H * E + H * dh + H * pad4(n) + NT + NW * 3 * H)
      * (long)sizeof(float);
}
long bwd_row_lds_bytes(long H, long n, long dh, long E) {
  return (H * E + H * dh + 2 * H * pad4(n) + NT + NW * 3 * H + 4 * H)
      * (long)sizeof(float);
}
long bwd_col_lds_bytes(long H, long n) {
  return (2 * H * pad4(n) + NT + NW * 3) * (long)sizeof(float);
}

// LDS one workgroup may use on the current device, opt-in included
long device_lds_limit() {
  int dev = 0, base = 0, optin = 0;
  TORCH_CHECK(hipGetDevice(&dev) == hipSuccess, "se3_core: hipGetDevice");
  TORCH_CHECK(hipDeviceGetAttribute(
                  &base, hipDeviceAttributeMaxSharedMemoryPerBlock, dev)
              == hipSuccess, "se3_core: LDS size query failed");
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
              " (n is above se3_core_max_n)");
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
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, what,
              ": tensors must be 16-byte aligned");
}

struct Dims { int b, n, H, dh, E; };

Dims check_dims(const at::Tensor& q, const at::Tensor& k,
                const at::Tensor& v, const at::Tensor& x,
                const at::Tensor& edges, const at::Tensor& w_e,
                const at::Tensor& b_e,
                const c10::optional<at::Tensor>& mask, const char* what) {
  for (const at::Tensor* t : {&q, &k, &v, &x, &edges, &w_e, &b_e})
    check_f32(*t, what);
  TORCH_CHECK(q.dim() == 3 && edges.dim() == 4 && w_e.dim() == 2, what,
              ": bad ranks");
  const long b = q.size(0), n = q.size(1), C = q.size(2);
  const long H = w_e.size(0), E = edges.size(3);
  TORCH_CHECK(H >= 1 && H <= MAX_H, what, ": heads must be 1..8");
  TORCH_CHECK(C % H == 0, what, ": q width is not heads * dim_head");
  const long dh = C / H;
  TORCH_CHECK(dh % 4 == 0 && dh >= 4 && dh <= MAX_DH, what,
              ": dim_head must be a multiple of 4 up to 64");
  TORCH_CHECK(E % 64 == 0 && E >= 64 && E <= MAX_E, what,
              ": edge dim must be a multiple of 64 up to 512");
  TORCH_CHECK(b * n > 0 && b * n < (1L << 31) && b * H * n * n < (1L << 40),
              what, ": bad batch / length");
  auto is = [](const at::Tensor& t, at::IntArrayRef s) {
    return t.sizes() == s;
  };
  TORCH_CHECK(is(q, {b, n, C}) && is(k, {b, n, C}) && is(v, {b, n, C})
              && is(x, {b, n, 3}) && is(edges, {b, n, n, E})
              && is(w_e, {H, E + 1}) && is(b_e, {H}),
              what, ": shapes do not match");
  if (mask.has_value()) {
    TORCH_CHECK(mask->is_cuda() && mask->scalar_type() == at::kBool
                && mask->is_contiguous() && is(*mask, {b, n}),
                what, ": mask must be a contiguous (b, n) bool tensor");
  }
  return {(int)b, (int)n, (int)H, (int)dh, (int)E};
}

const unsigned char* mask_ptr(const c10::optional<at::Tensor>& mask) {
  return mask.has_value()
      ? reinterpret_cast<const unsigned char*>(mask->data_ptr<bool>())
      : nullptr;
}

#define SE3_DISPATCH_HEADS(H_RT, ...)                                  \
  switch (H_RT) {                                                      \
    case 1: { constexpr int H = 1; __VA_ARGS__; break; }               \
    case 2: { constexpr int H = 2; __VA_ARGS__; break; }               \
    case 3: { constexpr int H = 3; __VA_ARGS__; break; }               \
    case 4: { constexpr int H = 4; __VA_ARGS__; break; }               \
    case 5: { constexpr int H = 5; __VA_ARGS__; break; }               \
    case 6: { constexpr int H = 6; __VA_ARGS__; break; }               \
    case 7: { constexpr int H = 7; __VA_ARGS__; break; }               \
    case 8: { constexpr int H = 8; __VA_ARGS__; break; }               \
    default: TORCH_CHECK(false, "se3_core: heads must be 1..8");       \
  }

}  // namespace

// Largest n for which forward AND backward fit the device's LDS (the
// row-side backward is the largest user).
long se3_core_max_n(long heads, long dim_head, long edge_dim) {
  TORCH_CHECK(heads >= 1 && heads <= MAX_H, "se3_core_max_n: heads 1..8");
  TORCH_CHECK(dim_head >= 4 && dim_head <= MAX_DH,
              "se3_core_max_n: dim_head 4..64");
  TORCH_CHECK(edge_dim >= 64 && edge_dim <= MAX_E,
              "se3_core_max_n: edge dim 64..512");
  const long fixed = bwd_row_lds_bytes(heads, 0, dim_head, edge_dim);
  long n = (device_lds_limit() - fixed) / (2L * heads * (long)sizeof(float));
  n &= ~3L;                             // rows are padded to 4 floats
  return n > 0 ? n : 0;
}

// Returns {out (b,n,H*dh), dxh (b,n,H,3), attn (b,H,n,n)}; attn is empty
// unless save_attn.
std::vector<at::Tensor> se3_core_fwd(
    at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor x,
    at::Tensor edges, at::Tensor w_e, at::Tensor b_e, double scale,
    double eps, c10::optional<at::Tensor> mask, bool save_attn) {
  const Dims d = check_dims(q, k, v, x, edges, w_e, b_e, mask,
                            "se3_core_fwd");
  auto opt = q.options();
  auto out = at::empty_like(q);
  auto dxh = at::empty({d.b, d.n, d.H, 3}, opt);
  auto attn = save_attn ? at::empty({d.b, d.H, d.n, d.n}, opt)
                        : at::empty({0}, opt);
  const long smem = fwd_lds_bytes(d.H, d.n, d.dh, d.E);
  auto stream = at::cuda::getCurrentHIPStream();
  SE3_DISPATCH_HEADS(d.H, {
    prepare_launch(se3_core_fwd_kernel<H>, smem, "se3_core_fwd");
    hipLaunchKernelGGL(se3_core_fwd_kernel<H>, dim3((long)d.b * d.n),
                       dim3(NT), smem, stream,
                       q.data_ptr<float>(), k.data_ptr<float>(),
                       v.data_ptr<float>(), x.data_ptr<float>(),
                       edges.data_ptr<float>(), w_e.data_ptr<float>(),
                       b_e.data_ptr<float>(), mask_ptr(mask),
                       out.data_ptr<float>(), dxh.data_ptr<float>(),
                       save_attn ? attn.data_ptr<float>() : nullptr,
                       d.n, d.dh, d.E, (float)scale, (float)eps);
  });
  check_launch("se3_core_fwd");
  return {out, dxh, attn};
}

// Gradients of the seven core inputs, in input order:
//   {dq, dk, dv, dx, dedges, dw_e, db_e}; dedges is an empty tensor when
//   not requested.
std::vector<at::Tensor> se3_core_bwd(
    at::Tensor dout, at::Tensor ddxh, at::Tensor attn, at::Tensor q,
    at::Tensor k, at::Tensor v, at::Tensor x, at::Tensor edges,
    at::Tensor w_e, at::Tensor b_e, double scale, double eps,
    c10::optional<at::Tensor> mask, bool need_dedges) {
  const Dims d = check_dims(q, k, v, x, edges, w_e, b_e, mask,
                            "se3_core_bwd");
  check_f32(dout, "se3_core_bwd");
  check_f32(ddxh, "se3_core_bwd");
  check_f32(attn, "se3_core_bwd");
  TORCH_CHECK(dout.sizes() == q.sizes()
              && ddxh.sizes() == at::IntArrayRef({d.b, d.n, d.H, 3})
              && attn.sizes() == at::IntArrayRef({d.b, d.H, d.n, d.n}),
              "se3_core_bwd: dout / ddxh / saved attn shapes do not match");

  auto opt = q.options();
  const long rows = (long)d.b * d.n;
  auto dq = at::empty_like(q), dk = at::empty_like(k), dv = at::empty_like(v);
  auto dx = at::empty_like(x), dx_row = at::empty_like(x);
  auto dL = at::empty_like(attn);
  auto dedges = need_dedges ? at::empty_like(edges) : at::empty({0}, opt);
  auto dwe_part = at::empty({rows, (long)d.H, (long)d.E}, opt);
  auto dwd_part = at::empty({rows, (long)d.H}, opt);
  auto dbe_part = at::empty({rows, (long)d.H}, opt);

  const long smem_row = bwd_row_lds_bytes(d.H, d.n, d.dh, d.E);
  const long smem_col = bwd_col_lds_bytes(d.H, d.n);
  auto stream = at::cuda::getCurrentHIPStream();
  SE3_DISPATCH_HEADS(d.H, {
    prepare_launch(se3_core_bwd_row_kernel<H>, smem_row, "se3_core_bwd");
    hipLaunchKernelGGL(se3_core_bwd_row_kernel<H>, dim3(rows), dim3(NT),
                       smem_row, stream,
                       dout.data_ptr<float>(), ddxh.data_ptr<float>(),
                       attn.data_ptr<float>(), k.data_ptr<float>(),
                       v.data_ptr<float>(), x.data_ptr<float>(),
                       edges.data_ptr<float>(), w_e.data_ptr<float>(),
                       mask_ptr(mask), dq.data_ptr<float>(),
                       dL.data_ptr<float>(), dx_row.data_ptr<float>(),
                       dwe_part.data_ptr<float>(),
                       dwd_part.data_ptr<float>(),
                       dbe_part.data_ptr<float>(),
                       need_dedges ? dedges.data_ptr<float>() : nullptr,
                       d.n, d.dh, d.E, (float)scale, (float)eps);
    check_launch("se3_core_bwd (row side)");
    prepare_launch(se3_core_bwd_col_kernel<H>, smem_col, "se3_core_bwd");
    hipLaunchKernelGGL(se3_core_bwd_col_kernel<H>, dim3(rows), dim3(NT),
                       smem_col, stream,
                       dout.data_ptr<float>(), ddxh.data_ptr<float>(),
                       attn.data_ptr<float>(), dL.data_ptr<float>(),
                       q.data_ptr<float>(), x.data_ptr<float>(),
                       w_e.data_ptr<float>(), dx_row.data_ptr<float>(),
                       dk.data_ptr<float>(), dv.data_ptr<float>(),
                       dx.data_ptr<float>(),
                       d.n, d.dh, d.E, (float)scale, (float)eps);
    check_launch("se3_core_bwd (column side)");
  });
  // fold the per-row partials: dw_e = [sum dL edges | sum dL d2]
  // the two sums write straight into their column ranges of dw_e, so no
  // concatenation copy follows them
  auto dw_e = at::empty_like(w_e);
  auto dw_edges = dw_e.narrow(1, 0, d.E), dw_dist = dw_e.select(1, d.E);
  at::sum_out(dw_edges, dwe_part, {0});
  at::sum_out(dw_dist, dwd_part, {0});
  auto db_e = dbe_part.sum(0);
  return {dq, dk, dv, dx, dedges, dw_e, db_e};
}
