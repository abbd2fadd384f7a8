// Fused pair-representation build — gfx950 (K13 of SURVEY.md §2.17,
// reference alphafold2.py:715-726):
//
//   out[b, i, j, :] = left[b, i, :] + right[b, j, :] + emb[rel[b, i, j], :]
//
// The eager composition materializes the broadcast outer sum AND the
// gathered positional embedding before adding them (3 full (b,n,n,d)
// passes); this kernel writes the sum once.  One block per (b, i) row:
// the left row is staged in LDS, right rows and embedding rows stream
// through L2 (both are tiny and hot).
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "colsum.h"
#include "common.h"

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef __bf16 pb16;

namespace {

template <typename T>
__global__ void pairrep_fwd_kernel(const T* __restrict__ left,
                                   const T* __restrict__ right,
                                   const T* __restrict__ emb,
                                   const long* __restrict__ rel,
                                   T* __restrict__ out,
                                   int n, int d) {
  extern __shared__ char smem[];
  T* lrow = reinterpret_cast<T*>(smem);
  const long bi = blockIdx.x;          // b * n + i
  const long b = bi / n;
  const T* lg = left + bi * (long)d;
  for (int c = threadIdx.x; c < d; c += blockDim.x) lrow[c] = lg[c];
  __syncthreads();

  const T* rb = right + b * (long)n * d;
  const long* relrow = rel + bi * (long)n;
  T* og = out + bi * (long)n * d;
  // thread t owns 8-wide chunk (t % chunks) of row j = t / chunks.
  // When chunks does not divide blockDim the trailing threads duplicate
  // a row (identical values written twice — benign).
  const int chunks = d / 8;
  const int c8 = (threadIdx.x % chunks) * 8;
  const int j0 = threadIdx.x / chunks;
  const int jstep = blockDim.x / chunks;
  for (int j = j0; j < n; j += jstep) {
    const long e = relrow[j];
    T rv[8], ev[8], ov[8];
    vload<T, 8>(rb + (long)j * d + c8, rv);
    vload<T, 8>(emb + e * (long)d + c8, ev);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      ov[k] = from_f32<T>(to_f32(lrow[c8 + k]) + to_f32(rv[k]) +
                          to_f32(ev[k]));
    }
    vstore<T, 8>(og + (long)j * d + c8, ov);
  }
}

// ---------------------------------------------------------------------------
// backward: dleft[b,i] = sum_j dy[b,i,j], dright[b,j] = sum_i dy[b,i,j],
// demb[v] = sum over rel[b,i,j] == v of dy[b,i,j] -- all three from ONE
// read of dy, no float atomics, nothing of dy's size written.
//
// A block owns a 32 x 32 tile of (i, j) of one batch entry; a thread owns
// two adjacent columns of d (one dword of bf16), so a wave reads 256
// contiguous bytes and the 32 loads of a tile row are independent.  The
// thread walks the tile row by row and keeps, per column, one running
// sum for the row (its part of dleft[i]), 32 for the tile's columns (its
// parts of dright[j]) and adds into its own two columns of a V x d fp32
// table in LDS: columns are never shared, so the table needs neither
// atomics nor barriers.  Consecutive elements with the same index are
// summed in a register first (the model's clamp(i - j) is constant over
// most tiles).  The block stores its three partials whole and
// colsum_fold_launch adds them in a fixed order:
//   part_lr (T, 2, b, n, d): [t][0] the dleft parts of the tiles with
//                            tj == t, [t][1] the dright parts of ti == t
//   part_emb (tiles, V, d)
// An index outside [0, V) adds to nothing.
constexpr int PB_TILE = 32;
constexpr int PB_MAX_THREADS = 512;   // d <= 1024: 256 VGPRs per thread

__device__ __forceinline__ float2 load2f(const float* p) {
  return *reinterpret_cast<const float2*>(p);
}
__device__ __forceinline__ float2 load2f(const __hip_bfloat16* p) {
  const unsigned int raw = *reinterpret_cast<const unsigned int*>(p);
  return float2{__uint_as_float(raw << 16),
                __uint_as_float(raw & 0xffff0000u)};
}
__device__ __forceinline__ float2 load2f(const __half* p) {
  const __half2 h = *reinterpret_cast<const __half2*>(p);
  return float2{__low2float(h), __high2float(h)};
}

template <typename T>
__global__ __launch_bounds__(PB_MAX_THREADS)
void pairrep_bwd_kernel(const T* __restrict__ dy,
                        const long* __restrict__ rel,
                        float* __restrict__ part_lr,
                        float* __restrict__ part_emb,
                        int n, int d, int V, long bnd) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* tab = reinterpret_cast<float*>(smem);                 // [V][d]
  int* rel_l = reinterpret_cast<int*>(smem + (long)V * d * 4);  // [32][32]

  const int tj = blockIdx.x, ti = blockIdx.y, bz = blockIdx.z;
  const int i0 = ti * PB_TILE, j0 = tj * PB_TILE;
  const int ni = min(PB_TILE, n - i0), nj = min(PB_TILE, n - j0);
  const int c2 = threadIdx.x * 2;
  const bool active = c2 < d;

  for (int idx = threadIdx.x; idx < PB_TILE * PB_TILE; idx += blockDim.x) {
    const int ii = idx >> 5, jj = idx & 31;
    int e = -1;
    if (ii < ni && jj < nj) {
      const long v = rel[((long)bz * n + i0 + ii) * n + j0 + jj];
      if (v >= 0 && v < V) e = (int)v;
    }
    rel_l[idx] = e;
  }
  if (active)
    for (int e = 0; e < V; ++e)
      *reinterpret_cast<float2*>(tab + (long)e * d + c2) = float2{0.f, 0.f};
  __syncthreads();
  if (!active) return;

  float2 dr[PB_TILE];
#pragma unroll
  for (int jj = 0; jj < PB_TILE; ++jj) dr[jj] = float2{0.f, 0.f};
  int cur = -1;
  float2 eacc = {0.f, 0.f};

  const T* base = dy + (((long)bz * n + i0) * n + j0) * d + c2;
  float2 nxt[PB_TILE];
#pragma unroll
  for (int jj = 0; jj < PB_TILE; ++jj)
    nxt[jj] = jj < nj ? load2f(base + (long)jj * d) : float2{0.f, 0.f};

  float* pl = part_lr + (long)tj * 2 * bnd + ((long)bz * n + i0) * d + c2;
  for (int ii = 0; ii < ni; ++ii) {
    float2 w[PB_TILE];
#pragma unroll
    for (int jj = 0; jj < PB_TILE; ++jj) w[jj] = nxt[jj];
    if (ii + 1 < ni) {
      const T* row = base + (long)(ii + 1) * n * d;
#pragma unroll
      for (int jj = 0; jj < PB_TILE; ++jj)
        if (jj < nj) nxt[jj] = load2f(row + (long)jj * d);
    }
    float2 dl = {0.f, 0.f};
    const int* rrow = rel_l + ii * PB_TILE;
#pragma unroll
    for (int jj = 0; jj < PB_TILE; ++jj) {
      if (jj < nj) {
        const float2 f = w[jj];
        dl.x += f.x; dl.y += f.y;
        dr[jj].x += f.x; dr[jj].y += f.y;
        const int e = rrow[jj];
        if (e != cur) {
          if (cur >= 0) {
            float2* t = reinterpret_cast<float2*>(tab + (long)cur * d + c2);
            const float2 o = *t;
            *t = float2{o.x + eacc.x, o.y + eacc.y};
          }
          cur = e;
          eacc = float2{0.f, 0.f};
        }
        if (e >= 0) { eacc.x += f.x; eacc.y += f.y; }
      }
    }
    *reinterpret_cast<float2*>(pl + (long)ii * d) = dl;
  }
  if (cur >= 0) {
    float2* t = reinterpret_cast<float2*>(tab + (long)cur * d + c2);
    const float2 o = *t;
    *t = float2{o.x + eacc.x, o.y + eacc.y};
  }

  float* pr = part_lr + (long)ti * 2 * bnd + bnd + ((long)bz * n + j0) * d
      + c2;
#pragma unroll
  for (int jj = 0; jj < PB_TILE; ++jj)
    if (jj < nj) *reinterpret_cast<float2*>(pr + (long)jj * d) = dr[jj];

  const long blk = ((long)bz * gridDim.y + ti) * gridDim.x + tj;
  float* pe = part_emb + blk * V * d + c2;
  for (int e = 0; e < V; ++e)
    *reinterpret_cast<float2*>(pe + (long)e * d) =
        *reinterpret_cast<const float2*>(tab + (long)e * d + c2);
}

// LDS one block may use on the current device, opt-in included
long pairrep_lds_limit() {
  int dev = 0, base = 0, optin = 0;
  C10_HIP_CHECK(hipGetDevice(&dev));
  C10_HIP_CHECK(hipDeviceGetAttribute(
      &base, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
  if (hipDeviceGetAttribute(&optin, hipDeviceAttributeSharedMemPerBlockOptin,
                            dev) != hipSuccess) {
    (void)hipGetLastError();
    optin = 0;
  }
  return base > optin ? base : optin;
}

long pairrep_bwd_lds_bytes(long V, long d) {
  return V * d * 4 + PB_TILE * PB_TILE * 4;
}

}  // namespace

// what pairrep_bwd covers; anything else is the caller's composition
bool pairrep_bwd_covers(at::Tensor dy, long emb_rows) {
  if (dy.dim() != 4 || !dy.is_cuda() || !dy.is_contiguous()) return false;
  const auto st = dy.scalar_type();
  if (st != at::kBFloat16 && st != at::kFloat && st != at::kHalf)
    return false;
  const long b = dy.size(0), n = dy.size(1), d = dy.size(3);
  if (b < 1 || n < 1 || d < 8 || emb_rows < 1 || dy.size(2) != n)
    return false;
  if (d % 8 != 0 || d > 2 * PB_MAX_THREADS || b > 65535) return false;
  if ((n + PB_TILE - 1) / PB_TILE > 65535) return false;
  if (2 * b * n * d > INT_MAX || emb_rows * d > INT_MAX) return false;
  return pairrep_bwd_lds_bytes(emb_rows, d) <= pairrep_lds_limit();
}

// dy (b, n, n, d), rel (b, n, n) long -> [dleft (b, n, d), dright (b, n, d),
// demb (emb_rows, d)], fp32 sums rounded once to dy's dtype
std::vector<at::Tensor> pairrep_bwd(at::Tensor dy, at::Tensor rel,
                                    long emb_rows) {
  TORCH_CHECK(pairrep_bwd_covers(dy, emb_rows),
              "pairrep_bwd: shape, dtype or layout not covered (contiguous "
              "(b, n, n, d) bf16/fp16/fp32, d % 8 == 0, d <= ",
              2 * PB_MAX_THREADS, ", the emb_rows x d fp32 table within the "
              "LDS of a block)");
  TORCH_CHECK(rel.scalar_type() == at::kLong && rel.is_contiguous() &&
              rel.is_cuda() && rel.device() == dy.device() &&
              rel.dim() == 3 && rel.size(0) == dy.size(0) &&
              rel.size(1) == dy.size(1) && rel.size(2) == dy.size(2),
              "pairrep_bwd: rel must be contiguous long (b, n, n)");
  const int b = dy.size(0), n = dy.size(1), d = dy.size(3);
  const int V = (int)emb_rows;
  const int T = (n + PB_TILE - 1) / PB_TILE;
  const long bnd = (long)b * n * d, Vd = (long)V * d;
  const long tiles = (long)b * T * T;
  const auto fopt = dy.options().dtype(at::kFloat);
  // every element of both partial sets is written by exactly one block
  auto part_lr = at::empty({T, 2 * bnd}, fopt);
  auto part_emb = at::empty({tiles, Vd}, fopt);
  auto out = at::empty({2 * bnd + Vd}, fopt);
  const int threads = (d / 2 + 63) / 64 * 64;
  const long smem = pairrep_bwd_lds_bytes(V, d);
  auto stream = at::cuda::getCurrentHIPStream();

#define LAUNCH(T_)                                                          \
  do {                                                                      \
    if (smem > 64 * 1024)                                                   \
      C10_HIP_CHECK(hipFuncSetAttribute(                                    \
          reinterpret_cast<const void*>(&pairrep_bwd_kernel<T_>),           \
          hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));          \
    hipLaunchKernelGGL((pairrep_bwd_kernel<T_>), dim3(T, T, b),             \
                       dim3(threads), smem, stream,                         \
                       reinterpret_cast<const T_*>(dy.data_ptr()),          \
                       rel.data_ptr<long>(), part_lr.data_ptr<float>(),     \
                       part_emb.data_ptr<float>(), n, d, V, bnd);           \
  } while (0)
  if (dy.scalar_type() == at::kBFloat16) LAUNCH(__hip_bfloat16);
  else if (dy.scalar_type() == at::kFloat) LAUNCH(float);
  else LAUNCH(__half);
#undef LAUNCH
  hipError_t err = hipGetLastError();
  TORCH_CHECK(err == hipSuccess, "pairrep_bwd: launch failed: ",
              hipGetErrorString(err));
  float* o = out.data_ptr<float>();
  colsum_fold_launch(part_lr.data_ptr<float>(), o, T, 2 * bnd, false, stream);
  colsum_fold_launch(part_emb.data_ptr<float>(), o + 2 * bnd, tiles, Vd,
                     false, stream);
  err = hipGetLastError();
  TORCH_CHECK(err == hipSuccess, "pairrep_bwd: fold launch failed: ",
              hipGetErrorString(err));
  auto r = out.to(dy.scalar_type());
  return {r.narrow(0, 0, bnd).view({b, n, d}),
          r.narrow(0, bnd, bnd).view({b, n, d}),
          r.narrow(0, 2 * bnd, Vd).view({V, d})};
}

// left/right (b, n, d); emb (V, d); rel (b, n, n) long -> out (b, n, n, d)
at::Tensor pairrep_fwd(at::Tensor left, at::Tensor right, at::Tensor emb,
                       at::Tensor rel) {
  TORCH_CHECK(left.is_contiguous() && right.is_contiguous() &&
              emb.is_contiguous() && rel.is_contiguous(),
              "pairrep_fwd: contiguous inputs required");
  TORCH_CHECK(rel.scalar_type() == at::kLong, "pairrep_fwd: rel must be long");
  const int b = left.size(0), n = left.size(1), d = left.size(2);
  TORCH_CHECK(d % 8 == 0, "pairrep_fwd: d must be a multiple of 8");
  TORCH_CHECK(d <= 2048, "pairrep_fwd: d > 2048 not covered (one block "
              "row owns d/8 chunks across 256 threads)");
  TORCH_CHECK(emb.size(1) == d && right.size(2) == d, "pairrep_fwd: dim");
  auto out = at::empty({b, n, n, d}, left.options());
  const int block = 256;
  const int smem = d * left.element_size();
  auto stream = at::cuda::getCurrentHIPStream();

#define LAUNCH(T)                                                         \
  hipLaunchKernelGGL((pairrep_fwd_kernel<T>), dim3((long)b * n),          \
                     dim3(block), smem, stream,                           \
                     reinterpret_cast<const T*>(left.data_ptr()),         \
                     reinterpret_cast<const T*>(right.data_ptr()),        \
                     reinterpret_cast<const T*>(emb.data_ptr()),          \
                     rel.data_ptr<long>(),                                \
                     reinterpret_cast<T*>(out.data_ptr()), n, d)
  if (left.scalar_type() == at::kBFloat16) LAUNCH(__hip_bfloat16);
  else if (left.scalar_type() == at::kFloat) LAUNCH(float);
  else if (left.scalar_type() == at::kHalf) LAUNCH(__half);
  else TORCH_CHECK(false, "pairrep_fwd: unsupported dtype");
#undef LAUNCH
  return out;
}
