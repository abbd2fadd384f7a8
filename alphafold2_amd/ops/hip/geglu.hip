// Fused GEGLU activation — gfx950.
//
// FeedForward transition (reference alphafold2.py:69-94): the Linear
// produces (..., 2H); GEGLU keeps a = x[..., :H], gates = x[..., H:],
// out = a * gelu(gates).  Fusing the chunk + gelu + multiply saves two
// full tensor read/writes on a memory-bound op (K6 epilogue of
// SURVEY.md §2.17).  Vectorized 8-wide loads (guide G13).
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "common.h"
#include "colsum.h"

namespace {

// row-outer loop with multi-row packing: when H/VEC < blockDim the
// block covers several rows per iteration (shift-based row split for
// power-of-2 H — a runtime `idx / H` in the hot loop serializes on the
// integer-div unit).  row_shift = log2(H / VEC); 0 disables packing.
template <typename T, int VEC>
__global__ void geglu_fwd_kernel(const T* __restrict__ x, T* __restrict__ y,
                                 long rows, int H, int row_shift) {
  const int sub = row_shift ? (threadIdx.x >> row_shift) : 0;
  const int rows_per_iter = row_shift ? (blockDim.x >> row_shift) : 1;
  const int col0 = row_shift
      ? (threadIdx.x & ((1 << row_shift) - 1)) * VEC : threadIdx.x * VEC;
  const int cstep = row_shift ? H : blockDim.x * VEC;
  for (long row = (long)blockIdx.x * rows_per_iter + sub; row < rows;
       row += (long)gridDim.x * rows_per_iter) {
    const T* xr = x + row * (2L * H);
    T* yr = y + row * (long)H;
    for (int col = col0; col < H; col += cstep) {
      T av[VEC], gv[VEC], yv[VEC];
      vload<T, VEC>(xr + col, av);
      vload<T, VEC>(xr + H + col, gv);
#pragma unroll
      for (int k = 0; k < VEC; ++k)
        yv[k] = from_f32<T>(to_f32(av[k]) * gelu_f(to_f32(gv[k])));
      vstore<T, VEC>(yr + col, yv);
    }
  }
}

// CS: the block also stores one fp32 (2H,) partial row — the column sums
// of the ROUNDED dx it wrote (the bias gradient of the Linear in front);
// colsum_fold_kernel folds the rows.  Needs every thread to keep its
// columns from row to row, i.e. H <= blockDim.x * VEC (one column step).
// The running sums live in LDS slots the thread owns, not in registers:
// the kernel is VALU-bound on erf + exp, and 2 * VEC more live registers
// cost it waves (100 vs 74 VGPRs, 4 vs 6 waves/SIMD, when tried).
template <typename T, int VEC, bool CS>
__device__ __forceinline__ void geglu_bwd_body(const T* __restrict__ dy,
                                               const T* __restrict__ x,
                                               T* __restrict__ dx, long rows,
                                               int H, int row_shift,
                                               float* __restrict__ partials) {
  const int sub = row_shift ? (threadIdx.x >> row_shift) : 0;
  const int rows_per_iter = row_shift ? (blockDim.x >> row_shift) : 1;
  const int col0 = row_shift
      ? (threadIdx.x & ((1 << row_shift) - 1)) * VEC : threadIdx.x * VEC;
  const int cstep = row_shift ? H : blockDim.x * VEC;
  // [row group][2H], (row groups) * H <= blockDim.x * VEC = 256 * VEC
  __shared__ float red[CS ? 2 * 256 * VEC : 1];
  float4* my_a = nullptr;
  float4* my_g = nullptr;
  if constexpr (CS) {
    static_assert(!CS || VEC % 4 == 0, "column sums move float4");
    if (col0 < H) {
      my_a = reinterpret_cast<float4*>(red + sub * 2 * H + col0);
      my_g = reinterpret_cast<float4*>(red + sub * 2 * H + H + col0);
#pragma unroll
      for (int k = 0; k < VEC / 4; ++k)
        my_a[k] = my_g[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  for (long row = (long)blockIdx.x * rows_per_iter + sub; row < rows;
       row += (long)gridDim.x * rows_per_iter) {
    const T* dyr = dy + row * (long)H;
    const T* xr = x + row * (2L * H);
    T* dxr = dx + row * (2L * H);
    for (int col = col0; col < H; col += cstep) {
      T av[VEC], gv[VEC], dov[VEC], dav[VEC], dgv[VEC];
      vload<T, VEC>(xr + col, av);
      vload<T, VEC>(xr + H + col, gv);
      vload<T, VEC>(dyr + col, dov);
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        float go = to_f32(dov[k]);
        float g = to_f32(gv[k]);
        dav[k] = from_f32<T>(go * gelu_f(g));
        dgv[k] = from_f32<T>(go * to_f32(av[k]) * gelu_grad_f(g));
      }
      vstore<T, VEC>(dxr + col, dav);
      vstore<T, VEC>(dxr + H + col, dgv);
      if constexpr (CS) {
        // one column step (host-checked): col == col0, my_* are set.
        // The barrier keeps the compiler from promoting the LDS sums
        // back into registers across the row loop.
        __asm__ volatile("" ::: "memory");
#pragma unroll
        for (int k = 0; k < VEC / 4; ++k) {
          float4 sa = my_a[k], sg = my_g[k];
          sa.x += to_f32(dav[4 * k]);     sg.x += to_f32(dgv[4 * k]);
          sa.y += to_f32(dav[4 * k + 1]); sg.y += to_f32(dgv[4 * k + 1]);
          sa.z += to_f32(dav[4 * k + 2]); sg.z += to_f32(dgv[4 * k + 2]);
          sa.w += to_f32(dav[4 * k + 3]); sg.w += to_f32(dgv[4 * k + 3]);
          my_a[k] = sa;
          my_g[k] = sg;
        }
      }
    }
  }
  if constexpr (CS) {
    __syncthreads();
    for (int c = threadIdx.x; c < 2 * H; c += blockDim.x) {
      float t = 0.f;
      for (int r = 0; r < rows_per_iter; ++r) t += red[r * 2 * H + c];
      partials[(long)blockIdx.x * 2 * H + c] = t;
    }
  }
}

template <typename T, int VEC>
__global__ void geglu_bwd_kernel(const T* __restrict__ dy,
                                 const T* __restrict__ x,
                                 T* __restrict__ dx, long rows, int H,
                                 int row_shift) {
  geglu_bwd_body<T, VEC, false>(dy, x, dx, rows, H, row_shift, nullptr);
}

// 6 waves/SIMD is what geglu_bwd_kernel<bf16, 8> runs at: hold the
// column-sum variant to the same register budget
__global__ __launch_bounds__(256, 6)
void geglu_bwd_colsum_kernel(const __hip_bfloat16* __restrict__ dy,
                             const __hip_bfloat16* __restrict__ x,
                             __hip_bfloat16* __restrict__ dx, long rows,
                             int H, int row_shift,
                             float* __restrict__ partials) {
  geglu_bwd_body<__hip_bfloat16, 8, true>(dy, x, dx, rows, H, row_shift,
                                          partials);
}

}  // namespace

at::Tensor geglu_fwd(at::Tensor x) {
  TORCH_CHECK(x.is_contiguous(), "geglu_fwd: x must be contiguous");
  const int H2 = x.size(-1);
  TORCH_CHECK(H2 % 2 == 0, "geglu_fwd: last dim must be even");
  const int H = H2 / 2;
  const long rows = x.numel() / H2;

  auto sizes = x.sizes().vec();
  sizes.back() = H;
  auto y = at::empty(sizes, x.options());

  const int block = 256;
  const long total = rows * (long)H;
  auto stream = at::cuda::getCurrentHIPStream();

#define LAUNCH(T, VEC)                                                   \
  do {                                                                   \
    int colt = H / VEC;                                                  \
    int row_shift = 0;                                                   \
    if (colt < block && colt > 0 && (colt & (colt - 1)) == 0)            \
      row_shift = __builtin_ctz(colt);                                   \
    const int rpi = row_shift ? block >> row_shift : 1;                  \
    long grid = (rows + rpi - 1) / rpi;                                  \
    if (grid > 65536) grid = 65536;                                        \
    if (grid < 1) grid = 1;                                              \
    hipLaunchKernelGGL((geglu_fwd_kernel<T, VEC>), dim3(grid),           \
                       dim3(block), 0, stream,                           \
                       reinterpret_cast<const T*>(x.data_ptr()),         \
                       reinterpret_cast<T*>(y.data_ptr()), rows, H,      \
                       row_shift);                                       \
  } while (0)

  // multi-row packing keeps all lanes busy at any H; prefer 16B lanes
  const bool vec8 = (H % 8) == 0;
  const bool vec4 = (H % 4) == 0;
  if (x.scalar_type() == at::kBFloat16) {
    if (vec8) LAUNCH(__hip_bfloat16, 8);
    else if (vec4) LAUNCH(__hip_bfloat16, 4);
    else LAUNCH(__hip_bfloat16, 1);
  } else if (x.scalar_type() == at::kFloat) {
    if (vec4) LAUNCH(float, 4); else LAUNCH(float, 1);
  } else if (x.scalar_type() == at::kHalf) {
    if (vec8) LAUNCH(__half, 8);
    else if (vec4) LAUNCH(__half, 4);
    else LAUNCH(__half, 1);
  } else {
    TORCH_CHECK(false, "geglu_fwd: unsupported dtype");
  }
#undef LAUNCH
  return y;
}

at::Tensor geglu_bwd(at::Tensor dy, at::Tensor x) {
  TORCH_CHECK(dy.is_contiguous() && x.is_contiguous(),
              "geglu_bwd: inputs must be contiguous");
  const int H2 = x.size(-1);
  const int H = H2 / 2;
  const long rows = x.numel() / H2;
  auto dx = at::empty_like(x);

  const int block = 256;
  const long total = rows * (long)H;
  auto stream = at::cuda::getCurrentHIPStream();

#define LAUNCH(T, VEC)                                                   \
  do {                                                                   \
    int colt = H / VEC;                                                  \
    int row_shift = 0;                                                   \
    if (colt < block && colt > 0 && (colt & (colt - 1)) == 0)            \
      row_shift = __builtin_ctz(colt);                                   \
    const int rpi = row_shift ? block >> row_shift : 1;                  \
    long grid = (rows + rpi - 1) / rpi;                                  \
    if (grid > 65536) grid = 65536;                                        \
    if (grid < 1) grid = 1;                                              \
    hipLaunchKernelGGL((geglu_bwd_kernel<T, VEC>), dim3(grid),           \
                       dim3(block), 0, stream,                           \
                       reinterpret_cast<const T*>(dy.data_ptr()),        \
                       reinterpret_cast<const T*>(x.data_ptr()),         \
                       reinterpret_cast<T*>(dx.data_ptr()), rows, H,     \
                       row_shift);                                       \
  } while (0)

  // multi-row packing keeps all lanes busy at any H; prefer 16B lanes
  const bool vec8 = (H % 8) == 0;
  const bool vec4 = (H % 4) == 0;
  if (x.scalar_type() == at::kBFloat16) {
    if (vec8) LAUNCH(__hip_bfloat16, 8);
    else if (vec4) LAUNCH(__hip_bfloat16, 4);
    else LAUNCH(__hip_bfloat16, 1);
  } else if (x.scalar_type() == at::kFloat) {
    if (vec4) LAUNCH(float, 4); else LAUNCH(float, 1);
  } else if (x.scalar_type() == at::kHalf) {
    if (vec8) LAUNCH(__half, 8);
    else if (vec4) LAUNCH(__half, 4);
    else LAUNCH(__half, 1);
  } else {
    TORCH_CHECK(false, "geglu_bwd: unsupported dtype");
  }
#undef LAUNCH
  return dx;
}

// geglu_bwd that also returns the fp32 column sum (2H,) of the rounded
// dx over all rows — the bias gradient of the Linear that produced x.
// bf16, H a multiple of 8 and at most 2048 (geglu_bwd_colsum_max_h).
long geglu_bwd_colsum_max_h() { return 256 * 8; }

std::vector<at::Tensor> geglu_bwd_colsum(at::Tensor dy, at::Tensor x) {
  TORCH_CHECK(dy.is_contiguous() && x.is_contiguous(),
              "geglu_bwd_colsum: inputs must be contiguous");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 &&
              dy.scalar_type() == at::kBFloat16 && dy.device() == x.device(),
              "geglu_bwd_colsum: bf16 tensors on one device");
  TORCH_CHECK(x.dim() >= 1 && x.numel() > 0,
              "geglu_bwd_colsum: x must be non-empty");
  const int H2 = x.size(-1);
  const int H = H2 / 2;
  TORCH_CHECK(H2 % 16 == 0 && H <= geglu_bwd_colsum_max_h(),
              "geglu_bwd_colsum: half width must be a multiple of 8 up to ",
              geglu_bwd_colsum_max_h(), ", got ", H);
  const long rows = x.numel() / H2;
  TORCH_CHECK(dy.numel() == rows * (long)H && dy.size(-1) == H,
              "geglu_bwd_colsum: dy must be (..., ", H, ") with x's rows");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0 &&
              reinterpret_cast<uintptr_t>(dy.data_ptr()) % 16 == 0,
              "geglu_bwd_colsum: tensors must be 16-byte aligned");
  auto dx = at::empty_like(x);

  const int block = 256;
  const int colt = H / 8;
  int row_shift = 0;
  if (colt < block && (colt & (colt - 1)) == 0) row_shift = __builtin_ctz(colt);
  const int rpi = row_shift ? block >> row_shift : 1;
  // blocks loop over the rows (grid-stride); whole resident rounds only
  const long grid = colsum_grid(
      reinterpret_cast<const void*>(geglu_bwd_colsum_kernel), block,
      (rows + rpi - 1) / rpi);
  auto fopt = x.options().dtype(at::kFloat);
  auto partials = at::empty({grid, H2}, fopt);
  auto colsum = at::empty({H2}, fopt);
  auto stream = at::cuda::getCurrentHIPStream();
  using T = __hip_bfloat16;
  hipLaunchKernelGGL(geglu_bwd_colsum_kernel, dim3(grid), dim3(block),
                     0, stream, reinterpret_cast<const T*>(dy.data_ptr()),
                     reinterpret_cast<const T*>(x.data_ptr()),
                     reinterpret_cast<T*>(dx.data_ptr()), rows, H, row_shift,
                     partials.data_ptr<float>());
  colsum_fold_launch(partials.data_ptr<float>(), colsum.data_ptr<float>(),
                     grid, H2, false, stream);
  return {dx, colsum};
}
