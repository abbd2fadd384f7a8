// Deterministic column sums riding on an elementwise kernel — gfx950.
//
// A kernel that also wants the column sum of what it writes keeps fp32
// running sums per thread (every thread keeps its columns from row to
// row), reduces them over its row groups in LDS and stores ONE (C,)
// partial row per block; colsum_fold_kernel folds the (nb, C) partials
// into (C,).  One writer per element and a fixed order, so the result is
// the same on every run — no float atomics.
#pragma once

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

// (nb, C) partial rows -> (C,).  1024 threads = 64 row lanes x 16
// columns: row lane r adds rows r, r + 64, ... in order, then lane 0 of
// each column adds the 64 lane sums in order.  (C + 15) / 16 blocks.
constexpr int COLSUM_FOLD_THREADS = 1024;

static __global__ __launch_bounds__(COLSUM_FOLD_THREADS)
void colsum_fold_kernel(const float* __restrict__ part,
                               float* __restrict__ out, int nb, int C) {
  __shared__ float sh[64][17];
  const int cl = threadIdx.x & 15;
  const int r = threadIdx.x >> 4;
  const int c = blockIdx.x * 16 + cl;
  float s = 0.f;
  if (c < C)
    for (int i = r; i < nb; i += 64) s += part[(long)i * C + c];
  sh[r][cl] = s;
  __syncthreads();
  if (r == 0 && c < C) {
    float t = 0.f;
#pragma unroll 8
    for (int j = 0; j < 64; ++j) t += sh[j][cl];
    out[c] = t;
  }
}
