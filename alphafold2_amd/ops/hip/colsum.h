// Deterministic column sums riding on an elementwise kernel — gfx950.
//
// A kernel that also wants the column sum of what it writes keeps fp32
// running sums per thread (every thread keeps its columns from row to
// row), reduces them over its row groups in LDS and stores ONE (C,)
// partial row per block; colsum_fold_launch folds the (nb, C) partials
// into (C,).  One writer per element and a fixed order, so the result is
// the same on every run — no float atomics.
#pragma once

#include <cstdint>
#include <cstdlib>
#include <map>
#include <mutex>
#include <utility>

#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>

// cap of a producing grid (bounds the partials: COLSUM_MAX_BLOCKS x C)
constexpr int COLSUM_MAX_BLOCKS = 2048;

// Grid of a producer whose blocks loop over the rows: every block does
// the same share of the work, so a grid that is no whole number of
// resident rounds leaves the machine nearly idle in its last round
// (geglu_bwd_colsum on the pair rep: 807 us at 2048 blocks with 7
// resident per CU, 729 us at 1792).  The grid is what the device holds
// at once, or fewer.  Host-side queries only, cached per kernel and
// device: safe under graph capture.
inline long colsum_grid(const void* kernel, int block, long blocks_needed) {
  static std::mutex mu;
  static std::map<std::pair<const void*, int>, long> cache;
  int dev = 0;
  C10_HIP_CHECK(hipGetDevice(&dev));
  long resident;
  {
    std::lock_guard<std::mutex> lock(mu);
    const auto key = std::make_pair(kernel, dev);
    auto it = cache.find(key);
    if (it == cache.end()) {
      int per_cu = 0;
      C10_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(
          &per_cu, kernel, block, 0));
      const long cus = at::cuda::getDeviceProperties(dev)->multiProcessorCount;
      it = cache.emplace(key, (per_cu > 0 ? per_cu : 1) * cus).first;
    }
    resident = it->second;
  }
  long grid = blocks_needed < resident ? blocks_needed : resident;
  if (grid > COLSUM_MAX_BLOCKS) grid = COLSUM_MAX_BLOCKS;
  return grid < 1 ? 1 : grid;
}

// (nb, C) partial rows -> (C,), the scalar body (r05): what
// AF2AMD_COLSUM_FOLD_V1=1 selects, and the path of a C that is no
// multiple of 4 or of rows that are not 16-byte aligned.  1024 threads =
// 64 row lanes x 16 columns: row lane r adds rows r, r + 64, ... in
// order, then lane 0 of each column adds the 64 lane sums in order.
// (C + 15) / 16 blocks.  ACC adds the sum to what out holds.
constexpr int COLSUM_FOLD_THREADS = 1024;

template <bool ACC>
static __global__ __launch_bounds__(COLSUM_FOLD_THREADS)
void colsum_fold_kernel(const float* __restrict__ part,
                        float* __restrict__ out, int nb, int C, long ld) {
  __shared__ float sh[64][17];
  const int cl = threadIdx.x & 15;
  const int r = threadIdx.x >> 4;
  const int c = blockIdx.x * 16 + cl;
  float s = 0.f;
  if (c < C)
    for (int i = r; i < nb; i += 64) s += part[(long)i * ld + c];
  sh[r][cl] = s;
  __syncthreads();
  if (r == 0 && c < C) {
    float t = 0.f;
#pragma unroll 8
    for (int j = 0; j < 64; ++j) t += sh[j][cl];
    out[c] = ACC ? out[c] + t : t;
  }
}

// The same fold on whole cache lines (r10).  A thread owns one 16-byte
// column quad; CQ quads side by side make a block CQ * 4 columns wide,
// so a wave's load is 64 / CQ row pieces of CQ * 16 contiguous bytes
// (256 B at CQ = 16, 128 B at CQ = 8) where the scalar body touched
// four rows and half a line of each.  Row lane r of RL adds rows r,
// r + RL, ... in order, eight independent loads at a time; the RL lane
// sums then meet in a fixed binary tree in LDS.  Needs C % 4 == 0,
// ld % 4 == 0 and 16-byte aligned part and out.  (C / 4 + CQ - 1) / CQ blocks of
// CQ * RL threads.
template <int CQ, int RL, bool ACC>
static __global__ __launch_bounds__(CQ * RL)
void colsum_fold_vec_kernel(const float* __restrict__ part,
                            float* __restrict__ out, int nb, int C,
                            long ld) {
  __shared__ float4 sh[RL][CQ];
  const int cl = threadIdx.x % CQ;
  const int r = threadIdx.x / CQ;
  const int q = blockIdx.x * CQ + cl;          // column quad
  const bool ok = q < (C >> 2);
  float4 s = {0.f, 0.f, 0.f, 0.f};
  if (ok) {
    const float* p = part + (long)q * 4;
    int i = r;
    for (; i + 7 * RL < nb; i += 8 * RL) {
      float4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u)
        v[u] = *reinterpret_cast<const float4*>(p + (long)(i + u * RL) * ld);
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        s.x += v[u].x; s.y += v[u].y; s.z += v[u].z; s.w += v[u].w;
      }
    }
    for (; i < nb; i += RL) {
      const float4 v = *reinterpret_cast<const float4*>(p + (long)i * ld);
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
  }
  sh[r][cl] = s;
  __syncthreads();
#pragma unroll
  for (int h = RL / 2; h > 0; h >>= 1) {
    if (r < h) {
      const float4 a = sh[r][cl], b = sh[r + h][cl];
      sh[r][cl] = float4{a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w};
    }
    __syncthreads();
  }
  if (r == 0 && ok) {
    float4 t = sh[0][cl];
    float4* o = reinterpret_cast<float4*>(out) + q;
    if (ACC) {
      const float4 w = *o;
      t = float4{w.x + t.x, w.y + t.y, w.z + t.z, w.w + t.w};
    }
    *o = t;
  }
}

// AF2AMD_COLSUM_FOLD_V1=1 keeps every fold on the scalar body
inline bool colsum_fold_force_v1() {
  static const bool v1 = [] {
    const char* e = getenv("AF2AMD_COLSUM_FOLD_V1");
    return e != nullptr && e[0] == '1';
  }();
  return v1;
}

// Fold nb fp32 partial rows of C columns, ld floats apart (0: C, the
// rows are contiguous), into out (C,); with accumulate, add them to what
// out holds.  part and out do not overlap.  Launch only: safe under
// graph capture.  The caller checks the launch.
inline void colsum_fold_launch(const float* part, float* out, long nb,
                               long C, bool accumulate, hipStream_t stream,
                               bool force_v1 = false, long ld = 0) {
  if (ld == 0) ld = C;
  const bool vec = !force_v1 && !colsum_fold_force_v1() && C % 4 == 0 &&
      ld % 4 == 0 &&
      reinterpret_cast<uintptr_t>(part) % 16 == 0 &&
      reinterpret_cast<uintptr_t>(out) % 16 == 0;
#define COLSUM_FOLD_GO(GRID, THREADS, ...)                                  \
  do {                                                                      \
    if (accumulate)                                                         \
      hipLaunchKernelGGL((__VA_ARGS__ true>), dim3((unsigned int)(GRID)),   \
                         dim3(THREADS), 0, stream, part, out, (int)nb,      \
                         (int)C, ld);                                       \
    else                                                                    \
      hipLaunchKernelGGL((__VA_ARGS__ false>), dim3((unsigned int)(GRID)),  \
                         dim3(THREADS), 0, stream, part, out, (int)nb,      \
                         (int)C, ld);                                       \
  } while (0)
  if (!vec) {
    COLSUM_FOLD_GO((C + 15) / 16, COLSUM_FOLD_THREADS, colsum_fold_kernel<);
    return;
  }
  // wide blocks with few row lanes where the columns alone fill the
  // device; narrow blocks with many row lanes where they do not
  const long quads = C / 4;
  if (quads >= 16 * 512) {
    COLSUM_FOLD_GO((quads + 15) / 16, 16 * 16, colsum_fold_vec_kernel<16, 16,);
  } else {
    COLSUM_FOLD_GO((quads + 7) / 8, 8 * 128, colsum_fold_vec_kernel<8, 128,);
  }
#undef COLSUM_FOLD_GO
}
