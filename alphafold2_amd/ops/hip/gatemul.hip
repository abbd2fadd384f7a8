// Fused sigmoid gating: out = x * sigmoid(g) — gfx950.
//
// Used by attention output gating (reference alphafold2.py:184-185) and
// the three triangle-multiplicative gates (:306-311).  One kernel
// instead of sigmoid + mul; inputs may be row-strided SLICES of a fused
// projection (no contiguous() copies); row-group parallelism keeps all
// lanes on 16-byte accesses at any channel width.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "common.h"
#include "colsum.h"

namespace {

__device__ __forceinline__ float sigmoid_f(float x) {
  return 1.0f / (1.0f + __expf(-x));
}

// rowmask: optional per-row multiplier (0/1 byte) fused in — saves the
// separate mask-multiply passes in the triangle module
template <typename T, int VEC, int GROUP, bool RM>
__global__ void gatemul_fwd_kernel(const T* __restrict__ x, long xs,
                                   const T* __restrict__ g, long gs,
                                   const unsigned char* __restrict__ rowmask,
                                   T* __restrict__ y,
                                   long rows, int C) {
  const int RPB = blockDim.x / GROUP;
  const int lane = threadIdx.x % GROUP;
  const int grp = threadIdx.x / GROUP;
  for (long row = (long)blockIdx.x * RPB + grp; row < rows;
       row += (long)gridDim.x * RPB) {
    const T* xr = x + row * xs;
    const T* gr = g + row * gs;
    T* yr = y + row * (long)C;
    const float mv = RM ? (float)rowmask[row] : 1.f;
    for (int i = lane * VEC; i < C; i += GROUP * VEC) {
      T xv[VEC], gv[VEC], yv[VEC];
      vload<T, VEC>(xr + i, xv);
      vload<T, VEC>(gr + i, gv);
#pragma unroll
      for (int k = 0; k < VEC; ++k)
        yv[k] = from_f32<T>(to_f32(xv[k]) * mv *
                            sigmoid_f(to_f32(gv[k])));
      vstore<T, VEC>(yr + i, yv);
    }
  }
}

template <typename T, int VEC, int GROUP, bool RM>
__global__ void gatemul_bwd_kernel(const T* __restrict__ dy,
                                   const T* __restrict__ x, long xs,
                                   const T* __restrict__ g, long gs,
                                   const unsigned char* __restrict__ rowmask,
                                   T* __restrict__ dx, long dxs,
                                   T* __restrict__ dg, long dgs,
                                   long rows, int C) {
  const int RPB = blockDim.x / GROUP;
  const int lane = threadIdx.x % GROUP;
  const int grp = threadIdx.x / GROUP;
  for (long row = (long)blockIdx.x * RPB + grp; row < rows;
       row += (long)gridDim.x * RPB) {
    const T* dyr = dy + row * (long)C;
    const T* xr = x + row * xs;
    const T* gr = g + row * gs;
    T* dxr = dx + row * dxs;
    T* dgr = dg + row * dgs;
    const float mv = RM ? (float)rowmask[row] : 1.f;
    for (int i = lane * VEC; i < C; i += GROUP * VEC) {
      T xv[VEC], gv[VEC], dov[VEC], dxv[VEC], dgv[VEC];
      vload<T, VEC>(xr + i, xv);
      vload<T, VEC>(gr + i, gv);
      vload<T, VEC>(dyr + i, dov);
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        float go = to_f32(dov[k]) * mv;
        float s = sigmoid_f(to_f32(gv[k]));
        dxv[k] = from_f32<T>(go * s);
        dgv[k] = from_f32<T>(go * to_f32(xv[k]) * s * (1.f - s));
      }
      vstore<T, VEC>(dxr + i, dxv);
      vstore<T, VEC>(dgr + i, dgv);
    }
  }
}

// Gate backward of gated attention in one pass.  dy (rows, C = H * 64)
// and o (the attention output in its (B, L, H, 64) memory) are
// contiguous; g is the gate slice of the packed projection (row stride
// gs).  Writes
//   dO    = bf16(dy * sigmoid(g)), contiguous in o's layout,
//   dg    = bf16(dy * o * s * (1 - s)) into the gate slice of the packed
//           gradient (row stride dgs),
//   delta = rowsum over each head's 64 channels of dO * o in fp32, from
//           the ROUNDED dO — lane mapping and summation order of
//           attn_delta_kernel (8 lanes x 8 channels per head segment,
//           xor-shuffles 4, 2, 1), stored as (B, H, L),
//   and, with CS, one fp32 (C,) partial row per block: the column sums
//   of the rounded dg over the block's rows (colsum_fold_kernel folds
//   them).  The dO / dg expressions are gatemul_bwd_kernel's.
// GROUP lanes share a row; a thread owns channels (it * GROUP + lane) * 8
// for it < NIT, the same for every row it visits.
template <int GROUP, int NIT, bool CS>
__global__ __launch_bounds__(256)
void attn_gate_bwd_kernel(const __hip_bfloat16* __restrict__ dy,
                          const __hip_bfloat16* __restrict__ o,
                          const __hip_bfloat16* __restrict__ g, long gs,
                          __hip_bfloat16* __restrict__ d_o,
                          __hip_bfloat16* __restrict__ dg, long dgs,
                          float* __restrict__ delta,
                          float* __restrict__ partials,
                          long rows, int C, int H, int L) {
  using T = __hip_bfloat16;
  constexpr int RPB = 256 / GROUP;
  constexpr int CPAD = GROUP * 8 * NIT;  // channels a row group covers
  const int lane = threadIdx.x % GROUP;
  const int grp = threadIdx.x / GROUP;
  float acc[NIT][8];
#pragma unroll
  for (int it = 0; it < NIT; ++it)
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[it][k] = 0.f;

  // row = b * L + l, kept as (b, l) without a division per row: the
  // pass is close to VALU-bound, a 64-bit divide per row shows
  const long step = (long)gridDim.x * RPB;
  const long step_b = step / L;
  const int step_l = (int)(step - step_b * L);
  long row = (long)blockIdx.x * RPB + grp;
  long b = row / L;
  int l = (int)(row - b * L);
  for (; row < rows; row += step, b += step_b, l += step_l) {
    if (l >= L) {
      l -= L;
      ++b;
    }
    const T* dyr = dy + row * (long)C;
    const T* orow = o + row * (long)C;
    const T* gr = g + row * gs;
    T* dor = d_o + row * (long)C;
    T* dgr = dg + row * dgs;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int i = (it * GROUP + lane) * 8;
      // C is a multiple of 64: the 8 lanes of a head segment agree
      if (i < C) {
        T xv[8], gv[8], dov[8], dxv[8], dgv[8];
        vload<T, 8>(orow + i, xv);
        vload<T, 8>(gr + i, gv);
        vload<T, 8>(dyr + i, dov);
        float v = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          float go = to_f32(dov[k]);
          float s = sigmoid_f(to_f32(gv[k]));
          dxv[k] = from_f32<T>(go * s);
          dgv[k] = from_f32<T>(go * to_f32(xv[k]) * s * (1.f - s));
          v += to_f32(dxv[k]) * to_f32(xv[k]);
          if (CS) acc[it][k] += to_f32(dgv[k]);
        }
        vstore<T, 8>(dor + i, dxv);
        vstore<T, 8>(dgr + i, dgv);
#pragma unroll
        for (int off = 4; off > 0; off >>= 1) v += __shfl_xor(v, off, 8);
        if ((lane & 7) == 0)
          delta[(b * H + (i >> 6)) * (long)L + l] = v;
      }
    }
  }

  if (CS) {
    __shared__ float red[RPB * CPAD];
#pragma unroll
    for (int it = 0; it < NIT; ++it)
#pragma unroll
      for (int k = 0; k < 8; ++k)
        red[grp * CPAD + (it * GROUP + lane) * 8 + k] = acc[it][k];
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
      float t = 0.f;
#pragma unroll
      for (int r = 0; r < RPB; ++r) t += red[r * CPAD + c];
      partials[(long)blockIdx.x * C + c] = t;
    }
  }
}

int gm_group(int C, int VEC) {
  int per_row = (C + VEC - 1) / VEC;
  if (per_row <= 16) return 16;
  if (per_row <= 32) return 32;
  return 64;
}

long gm_grid(long rows, int rpb) {
  long blocks = (rows + rpb - 1) / rpb;
  const long cap = 65536;
  return blocks < cap ? blocks : (cap > 0 ? cap : 1);
}

// operands are reinterpreted as T* by the launch macros: a mismatched
// dtype or a strided innermost dim would be read past its end
void gm_check_operand(const at::Tensor& t, const at::Tensor& x,
                      const char* fn, const char* name) {
  TORCH_CHECK(t.scalar_type() == x.scalar_type(), fn, ": ", name,
              " must have x's dtype (", x.scalar_type(), "), got ",
              t.scalar_type());
  TORCH_CHECK(t.device() == x.device(), fn, ": ", name,
              " must be on x's device");
  TORCH_CHECK(t.sizes() == x.sizes(), fn, ": ", name,
              " must have x's shape");
  TORCH_CHECK(t.size(-1) == 1 || t.stride(-1) == 1, fn, ": ", name,
              " must be dense in its last dim");
}

bool gm_aligned16(const at::Tensor& t) {
  return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0;
}

const unsigned char* gm_check_rowmask(const c10::optional<at::Tensor>& rm,
                                      const at::Tensor& x, long rows,
                                      const char* fn) {
  if (!rm.has_value()) return nullptr;
  TORCH_CHECK(rm->scalar_type() == at::kByte, fn,
              ": rowmask must be uint8, got ", rm->scalar_type());
  TORCH_CHECK(rm->device() == x.device(), fn,
              ": rowmask must be on x's device");
  TORCH_CHECK(rm->numel() == rows && rm->is_contiguous(), fn,
              ": rowmask must be contiguous with one byte per row (", rows,
              "), got ", rm->numel());
  return rm->data_ptr<unsigned char>();
}

}  // namespace

// x/g: (rows, C) with uniform row strides xs/gs (elements); y contiguous
at::Tensor gatemul_fwd(at::Tensor x, at::Tensor g, long xs, long gs,
                       c10::optional<at::Tensor> rowmask) {
  TORCH_CHECK(x.dim() >= 1 && x.numel() > 0,
              "gatemul_fwd: x must be non-empty");
  TORCH_CHECK(x.size(-1) == 1 || x.stride(-1) == 1,
              "gatemul_fwd: x must be dense in its last dim");
  gm_check_operand(g, x, "gatemul_fwd", "g");
  const int C = x.size(-1);
  const long rows = x.numel() / C;
  const bool rm = rowmask.has_value();
  const unsigned char* rm_ptr =
      gm_check_rowmask(rowmask, x, rows, "gatemul_fwd");
  auto y = at::empty(x.sizes(), x.options());
  const int block = 256;
  auto stream = at::cuda::getCurrentHIPStream();

#define LAUNCH_G2(T, VEC, GROUP, RM)                                        \
  hipLaunchKernelGGL((gatemul_fwd_kernel<T, VEC, GROUP, RM>),               \
                     dim3(gm_grid(rows, block / GROUP)), dim3(block), 0,    \
                     stream, reinterpret_cast<const T*>(x.data_ptr()), xs,  \
                     reinterpret_cast<const T*>(g.data_ptr()), gs, rm_ptr,  \
                     reinterpret_cast<T*>(y.data_ptr()), rows, C)
#define LAUNCH_G(T, VEC, GROUP)                                             \
  do {                                                                      \
    if (rm) LAUNCH_G2(T, VEC, GROUP, true);                                 \
    else LAUNCH_G2(T, VEC, GROUP, false);                                   \
  } while (0)
#define LAUNCH(T, VEC)                                                      \
  do {                                                                      \
    int gg = gm_group(C, VEC);                                              \
    if (gg == 16) LAUNCH_G(T, VEC, 16);                                     \
    else if (gg == 32) LAUNCH_G(T, VEC, 32);                                \
    else LAUNCH_G(T, VEC, 64);                                              \
  } while (0)

  // the vector paths move 16 bytes per access: row strides AND base
  // pointers (a slice can start mid-vector) must keep every row aligned
  const bool base16 = gm_aligned16(x) && gm_aligned16(g);
  const bool al8 = base16 && (C % 8) == 0 && (xs % 8) == 0 && (gs % 8) == 0;
  const bool al4 = base16 && (C % 4) == 0 && (xs % 4) == 0 && (gs % 4) == 0;
  if (x.scalar_type() == at::kBFloat16) {
    if (al8) LAUNCH(__hip_bfloat16, 8);
    else LAUNCH(__hip_bfloat16, 1);
  } else if (x.scalar_type() == at::kFloat) {
    if (al4) LAUNCH(float, 4); else LAUNCH(float, 1);
  } else if (x.scalar_type() == at::kHalf) {
    if (al8) LAUNCH(__half, 8); else LAUNCH(__half, 1);
  } else {
    TORCH_CHECK(false, "gatemul_fwd: unsupported dtype");
  }
#undef LAUNCH
#undef LAUNCH_G
#undef LAUNCH_G2
  return y;
}

// dx_out/dg_out (with row strides dxs/dgs) let the backward write its
// gradients straight into slices of a packed buffer — the autograd
// SplitBackward concatenation disappears (it was ~16 ms/step).
std::vector<at::Tensor> gatemul_bwd(at::Tensor dy, at::Tensor x,
                                    at::Tensor g, long xs, long gs,
                                    c10::optional<at::Tensor> rowmask,
                                    c10::optional<at::Tensor> dx_out,
                                    c10::optional<at::Tensor> dg_out,
                                    long dxs, long dgs) {
  TORCH_CHECK(dy.is_contiguous(), "gatemul_bwd: dy must be contiguous");
  TORCH_CHECK(x.dim() >= 1 && x.numel() > 0,
              "gatemul_bwd: x must be non-empty");
  TORCH_CHECK(x.size(-1) == 1 || x.stride(-1) == 1,
              "gatemul_bwd: x must be dense in its last dim");
  gm_check_operand(g, x, "gatemul_bwd", "g");
  gm_check_operand(dy, x, "gatemul_bwd", "dy");
  TORCH_CHECK(dx_out.has_value() == dg_out.has_value(),
              "gatemul_bwd: dx_out and dg_out must be given together");
  const int C = x.size(-1);
  const long rows = x.numel() / C;
  const bool rm = rowmask.has_value();
  const unsigned char* rm_ptr =
      gm_check_rowmask(rowmask, x, rows, "gatemul_bwd");
  at::Tensor dx, dg;
  if (dx_out.has_value()) {
    gm_check_operand(*dx_out, x, "gatemul_bwd", "dx_out");
    gm_check_operand(*dg_out, x, "gatemul_bwd", "dg_out");
    dx = *dx_out;
    dg = *dg_out;
  } else {
    dx = at::empty(x.sizes(), x.options());
    dg = at::empty(x.sizes(), x.options());
    dxs = dgs = C;
  }
  const int block = 256;
  auto stream = at::cuda::getCurrentHIPStream();

#define LAUNCH_G2(T, VEC, GROUP, RM)                                        \
  hipLaunchKernelGGL((gatemul_bwd_kernel<T, VEC, GROUP, RM>),               \
                     dim3(gm_grid(rows, block / GROUP)), dim3(block), 0,    \
                     stream, reinterpret_cast<const T*>(dy.data_ptr()),     \
                     reinterpret_cast<const T*>(x.data_ptr()), xs,          \
                     reinterpret_cast<const T*>(g.data_ptr()), gs, rm_ptr,  \
                     reinterpret_cast<T*>(dx.data_ptr()), dxs,              \
                     reinterpret_cast<T*>(dg.data_ptr()), dgs, rows, C)
#define LAUNCH_G(T, VEC, GROUP)                                             \
  do {                                                                      \
    if (rm) LAUNCH_G2(T, VEC, GROUP, true);                                 \
    else LAUNCH_G2(T, VEC, GROUP, false);                                   \
  } while (0)
#define LAUNCH(T, VEC)                                                      \
  do {                                                                      \
    int gg = gm_group(C, VEC);                                              \
    if (gg == 16) LAUNCH_G(T, VEC, 16);                                     \
    else if (gg == 32) LAUNCH_G(T, VEC, 32);                                \
    else LAUNCH_G(T, VEC, 64);                                              \
  } while (0)

  const bool base16 = gm_aligned16(x) && gm_aligned16(g) &&
      gm_aligned16(dy) && gm_aligned16(dx) && gm_aligned16(dg);
  const bool al8 = base16 && (C % 8) == 0 && (xs % 8) == 0 && (gs % 8) == 0
      && (dxs % 8) == 0 && (dgs % 8) == 0;
  const bool al4 = base16 && (C % 4) == 0 && (xs % 4) == 0 && (gs % 4) == 0
      && (dxs % 4) == 0 && (dgs % 4) == 0;
  if (x.scalar_type() == at::kBFloat16) {
    if (al8) LAUNCH(__hip_bfloat16, 8);
    else LAUNCH(__hip_bfloat16, 1);
  } else if (x.scalar_type() == at::kFloat) {
    if (al4) LAUNCH(float, 4); else LAUNCH(float, 1);
  } else if (x.scalar_type() == at::kHalf) {
    if (al8) LAUNCH(__half, 8); else LAUNCH(__half, 1);
  } else {
    TORCH_CHECK(false, "gatemul_bwd: unsupported dtype");
  }
#undef LAUNCH
#undef LAUNCH_G
#undef LAUNCH_G2
  return {dx, dg};
}

namespace {

// (B, L, C) with a dense last dim and ONE row stride over (B, L): a
// channel slice of a packed projection qualifies
long ag_row_stride(const at::Tensor& t, long B, long L, long C,
                   const char* name) {
  TORCH_CHECK(t.scalar_type() == at::kBFloat16, "attn_gate_bwd: ", name,
              " must be bf16, got ", t.scalar_type());
  TORCH_CHECK(t.dim() == 3 && t.size(0) == B && t.size(1) == L &&
              t.size(2) == C, "attn_gate_bwd: ", name, " must be (", B, ", ",
              L, ", ", C, "), got ", t.sizes());
  const long rs = t.stride(1);
  TORCH_CHECK(t.stride(2) == 1 && rs >= C && (B == 1 || t.stride(0) == L * rs),
              "attn_gate_bwd: ", name,
              " must be dense in its last dim with one row stride");
  TORCH_CHECK(rs % 8 == 0 && gm_aligned16(t), "attn_gate_bwd: ", name,
              " rows must be 16-byte aligned");
  return rs;
}

}  // namespace

// Gate backward of gated attention (see attn_gate_bwd_kernel).
//   dy     (B, L, C = H * 64) contiguous: gradient of out * sigmoid(g)
//   out    (B, H, L, 64) view of (B, L, H, 64) memory, as attn_fwd returns
//   g      (B, L, C) gate slice of the packed projection
//   dg_out (B, L, C) gate slice of the packed gradient, written in place
// Returns {dO (same view as out), delta (B, H, L) fp32[, colsum (C,) fp32:
// the sum over all rows of the rounded dg]}.
std::vector<at::Tensor> attn_gate_bwd(at::Tensor dy, at::Tensor out,
                                      at::Tensor g, at::Tensor dg_out,
                                      bool want_colsum) {
  TORCH_CHECK(out.scalar_type() == at::kBFloat16 && out.dim() == 4 &&
              out.size(3) == 64 && out.numel() > 0,
              "attn_gate_bwd: out must be non-empty bf16 (B, h, L, 64)");
  const long B = out.size(0), H = out.size(1), L = out.size(2);
  const long C = H * 64, rows = B * L;
  TORCH_CHECK(out.permute({0, 2, 1, 3}).is_contiguous() && gm_aligned16(out),
              "attn_gate_bwd: out must be a view of contiguous, 16-byte "
              "aligned (B, L, h, 64) memory");
  TORCH_CHECK(dy.scalar_type() == at::kBFloat16 && dy.is_contiguous() &&
              dy.numel() == rows * C && dy.size(-1) == C && gm_aligned16(dy),
              "attn_gate_bwd: dy must be contiguous, 16-byte aligned bf16 "
              "(..., ", C, ") with ", rows, " rows");
  TORCH_CHECK(dy.device() == out.device() && g.device() == out.device() &&
              dg_out.device() == out.device(),
              "attn_gate_bwd: all tensors must be on one device");
  TORCH_CHECK(L <= INT_MAX && C <= INT_MAX, "attn_gate_bwd: shape too large");
  const long gs = ag_row_stride(g, B, L, C, "g");
  const long dgs = ag_row_stride(dg_out, B, L, C, "dg_out");

  auto d_o = at::empty({B, L, H, 64}, out.options());
  auto delta = at::empty({B, H, L}, out.options().dtype(at::kFloat));

  // lanes per row: a power of two covering C / 8, at most 64; wider rows
  // take NIT passes
  int group = 8;
  while (group < 64 && group * 8 < C) group *= 2;
  const int nit = (int)((C + group * 8 - 1) / (group * 8));
  TORCH_CHECK(nit <= 4, "attn_gate_bwd: at most 32 heads, got ", H);
  const int rpb = 256 / group;
  using T = __hip_bfloat16;
  using Kern = void (*)(const T*, const T*, const T*, long, T*, T*, long,
                        float*, float*, long, int, int, int);
  Kern kern = nullptr;
#define PICK_AG(GROUP, NIT)                                                 \
  kern = want_colsum ? attn_gate_bwd_kernel<GROUP, NIT, true>               \
                     : attn_gate_bwd_kernel<GROUP, NIT, false>
  if (group == 8) PICK_AG(8, 1);
  else if (group == 16) PICK_AG(16, 1);
  else if (group == 32) PICK_AG(32, 1);
  else if (nit == 1) PICK_AG(64, 1);
  else if (nit == 2) PICK_AG(64, 2);
  else PICK_AG(64, 4);
#undef PICK_AG
  // blocks loop over the rows (grid-stride); whole resident rounds only
  const long grid = colsum_grid(reinterpret_cast<const void*>(kern), 256,
                                (rows + rpb - 1) / rpb);

  at::Tensor partials, colsum;
  if (want_colsum) {
    partials = at::empty({grid, C}, delta.options());
    colsum = at::empty({C}, delta.options());
  }
  auto stream = at::cuda::getCurrentHIPStream();
  hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, stream,
                     reinterpret_cast<const T*>(dy.data_ptr()),
                     reinterpret_cast<const T*>(out.data_ptr()),
                     reinterpret_cast<const T*>(g.data_ptr()), gs,
                     reinterpret_cast<T*>(d_o.data_ptr()),
                     reinterpret_cast<T*>(dg_out.data_ptr()), dgs,
                     delta.data_ptr<float>(),
                     want_colsum ? partials.data_ptr<float>() : nullptr,
                     rows, (int)C, (int)H, (int)L);
  {
    const hipError_t err = hipGetLastError();
    TORCH_CHECK(err == hipSuccess, "attn_gate_bwd: launch failed: ",
                hipGetErrorString(err));
  }

  std::vector<at::Tensor> ret = {d_o.permute({0, 2, 1, 3}), delta};
  if (want_colsum) {
    colsum_fold_launch(partials.data_ptr<float>(), colsum.data_ptr<float>(),
                       grid, C, false, stream);
    ret.push_back(colsum);
  }
  return ret;
}
