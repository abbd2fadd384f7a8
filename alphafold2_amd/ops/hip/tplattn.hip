// Template pointwise attention (K5), forward and backward — gfx950.
//
// Alphafold2.forward pools T embedded templates into the pair
// representation with one cross-attention per pair position: b * P batch
// entries (P = n^2), ONE query each, T <= 16 keys.  The flash kernels of
// attention.hip stage a 128-row Q tile and a 64-row K/V tile for that one
// query; here the problem is treated as what it is, a streaming pass over
// operands that are read once:
//
//   q    (b, P, H*d)        output of to_q, any 16-byte aligned row strides
//   kv   (b, T, P, 2*H*d)   output of to_kv on the templates as they stand;
//                           k = channels [0, H*d), v = [H*d, 2*H*d), head h
//                           owns [h*d, (h+1)*d) of each half
//   key_mask   (b, T, P)    optional, bool / uint8, contiguous
//   query_mask (b, P)       optional, bool / uint8, contiguous
//   out  (b, P, H*d), lse (b, P, H) fp32
//
// so nothing is permuted, padded or expanded.  A group of G = d / 8 lanes
// owns one (position, head); each lane owns 8 channels (one 16-byte access
// in bf16, two in fp32).  The flat thread index runs over b * P * H * G,
// channel-fastest, so a wave reads contiguous q and, per template,
// contiguous k and v.  Groups are aligned runs of G <= 8 lanes and the
// thread count is a multiple of G: a group never straddles a wave and is
// active or idle as a whole, so the xor-shuffles below only ever meet live
// lanes.  No LDS, no atomics, no MFMA; every output element has exactly one
// writer, so results are the same from run to run.
//
// Math is fp32 whatever the storage type.  s_t = scale * q.k_t; a logit
// whose key or query is masked is -FLT_MAX (eager's masked_fill), so a
// row with every logit masked gets the uniform weights 1 / T and any other
// row gives its masked logits weight exactly 0.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <cfloat>

#include "common.h"

namespace {

constexpr int TPL_BLOCK = 256;

// 8 consecutive channels -> fp32 registers
template <typename T>
__device__ __forceinline__ void load8(const T* __restrict__ p, float* f) {
  T raw[8];
  if constexpr (sizeof(T) == 2) {
    vload<T, 8>(p, raw);
  } else {
    vload<T, 4>(p, raw);
    vload<T, 4>(p + 4, raw + 4);
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) f[k] = to_f32(raw[k]);
}

template <typename T>
__device__ __forceinline__ void store8(T* __restrict__ p, const float* f) {
  T raw[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) raw[k] = from_f32<T>(f[k]);
  if constexpr (sizeof(T) == 2) {
    vstore<T, 8>(p, raw);
  } else {
    vstore<T, 4>(p, raw);
    vstore<T, 4>(p + 4, raw + 4);
  }
}

// sum over the G lanes of a group, the same bits in every lane of it
template <int G>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int off = G / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, WAVE);
  return v;
}

__device__ __forceinline__ float dot8(const float* a, const float* b) {
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < 8; ++k) s = fmaf(a[k], b[k], s);
  return s;
}

struct TplShape {
  long P;       // positions per batch entry
  int T;        // templates
  int C;        // H * d
  int LP;       // lanes per position = C / 8
  long total;   // b * P * LP threads
  long q_bs, q_rs;           // q strides over (b, P), elements
  long kv_bs, kv_ts, kv_rs;  // kv strides over (b, T, P), elements
};

// forward: online softmax over a runtime loop on t (running max, running
// sum, 8 accumulators); k_t and v_t are each loaded once
template <typename T, int G>
__global__ __launch_bounds__(TPL_BLOCK)
void tplattn_fwd_kernel(const T* __restrict__ q, const T* __restrict__ kv,
                        const unsigned char* __restrict__ key_mask,
                        const unsigned char* __restrict__ query_mask,
                        T* __restrict__ out, float* __restrict__ lse,
                        TplShape sh, float scale) {
  const long idx = (long)blockIdx.x * TPL_BLOCK + threadIdx.x;
  if (idx >= sh.total) return;  // whole groups leave together
  const long pos = idx / sh.LP;          // bi * P + p
  const int ch = (int)(idx - pos * sh.LP) * 8;
  const long bi = pos / sh.P;
  const long p = pos - bi * sh.P;

  float qf[8], acc[8];
  load8<T>(q + bi * sh.q_bs + p * sh.q_rs + ch, qf);
#pragma unroll
  for (int k = 0; k < 8; ++k) acc[k] = 0.f;
  const bool q_on = query_mask == nullptr || query_mask[pos] != 0;

  float m = -INFINITY, l = 0.f;
  const T* kvp = kv + bi * sh.kv_bs + p * sh.kv_rs + ch;
  const unsigned char* kmp =
      key_mask ? key_mask + bi * sh.T * sh.P + p : nullptr;
  for (int t = 0; t < sh.T; ++t) {
    float kf[8], vf[8];
    load8<T>(kvp + t * sh.kv_ts, kf);
    load8<T>(kvp + t * sh.kv_ts + sh.C, vf);
    float s = scale * group_sum<G>(dot8(qf, kf));
    const bool on = q_on && (kmp == nullptr || kmp[t * sh.P] != 0);
    if (!on) s = -FLT_MAX;
    // m_new is finite from the first template on: no inf - inf
    const float m_new = fmaxf(m, s);
    const float alpha = expf(m - m_new);
    const float pt = expf(s - m_new);
    l = l * alpha + pt;
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] = fmaf(pt, vf[k], acc[k] * alpha);
    m = m_new;
  }
  const float inv = 1.f / l;
#pragma unroll
  for (int k = 0; k < 8; ++k) acc[k] *= inv;
  store8<T>(out + pos * sh.C + ch, acc);
  // an all-masked row keeps lse == -FLT_MAX (log T is far below its ulp):
  // the backward reads that as "uniform weights"
  if ((threadIdx.x & (G - 1)) == 0)
    lse[pos * (sh.C / (G * 8)) + ch / (G * 8)] = m + logf(l);
}

// backward: one pass over t from the saved out and lse.
//   delta = dout . out           p_t  = exp(s_t - lse)
//   dp_t  = dout . v_t           ds_t = scale * p_t * (dp_t - delta)
//   dq   += ds_t * k_t           dk_t = ds_t * q,  dv_t = p_t * dout
// A masked logit takes no gradient (masked_fill); its weight is 0, or
// 1 / T in a row whose logits are all masked, and dv gets that weight.
template <typename T, int G>
__global__ __launch_bounds__(TPL_BLOCK)
void tplattn_bwd_kernel(const T* __restrict__ dout, const T* __restrict__ q,
                        const T* __restrict__ kv, const T* __restrict__ out,
                        const float* __restrict__ lse,
                        const unsigned char* __restrict__ key_mask,
                        const unsigned char* __restrict__ query_mask,
                        T* __restrict__ dq, T* __restrict__ dkv,
                        TplShape sh, float scale) {
  const long idx = (long)blockIdx.x * TPL_BLOCK + threadIdx.x;
  if (idx >= sh.total) return;  // whole groups leave together
  const long pos = idx / sh.LP;
  const int ch = (int)(idx - pos * sh.LP) * 8;
  const long bi = pos / sh.P;
  const long p = pos - bi * sh.P;

  float qf[8], of[8], gof[8], dqf[8];
  load8<T>(q + bi * sh.q_bs + p * sh.q_rs + ch, qf);
  load8<T>(out + pos * sh.C + ch, of);
  load8<T>(dout + pos * sh.C + ch, gof);
#pragma unroll
  for (int k = 0; k < 8; ++k) dqf[k] = 0.f;
  const float delta = group_sum<G>(dot8(gof, of));
  const float row_lse = lse[pos * (sh.C / (G * 8)) + ch / (G * 8)];
  const bool q_on = query_mask == nullptr || query_mask[pos] != 0;
  const float p_masked = row_lse < -0.5f * FLT_MAX ? 1.f / (float)sh.T : 0.f;

  const T* kvp = kv + bi * sh.kv_bs + p * sh.kv_rs + ch;
  // dkv is contiguous (b, T, P, 2C)
  T* dkvp = dkv + ((bi * sh.T) * sh.P + p) * (2L * sh.C) + ch;
  const unsigned char* kmp =
      key_mask ? key_mask + bi * sh.T * sh.P + p : nullptr;
  for (int t = 0; t < sh.T; ++t) {
    float kf[8], vf[8], dkf[8], dvf[8];
    load8<T>(kvp + t * sh.kv_ts, kf);
    load8<T>(kvp + t * sh.kv_ts + sh.C, vf);
    const float s = scale * group_sum<G>(dot8(qf, kf));
    const float dp = group_sum<G>(dot8(gof, vf));
    const bool on = q_on && (kmp == nullptr || kmp[t * sh.P] != 0);
    const float pt = on ? expf(s - row_lse) : p_masked;
    const float ds = on ? scale * pt * (dp - delta) : 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      dqf[k] = fmaf(ds, kf[k], dqf[k]);
      dkf[k] = ds * qf[k];
      dvf[k] = pt * gof[k];
    }
    T* drow = dkvp + t * sh.P * (2L * sh.C);
    store8<T>(drow, dkf);
    store8<T>(drow + sh.C, dvf);
  }
  store8<T>(dq + pos * sh.C + ch, dqf);
}

bool tpl_aligned16(const at::Tensor& t) {
  return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0;
}

// the kernels reinterpret every row as 16-byte vectors: the base pointer
// and every stride that is multiplied by a nonzero index must keep them
// aligned, and the channels themselves must be dense
void tpl_check_rows(const at::Tensor& t, const char* fn, const char* name) {
  const long vec = 16 / t.element_size();
  TORCH_CHECK(t.stride(-1) == 1, fn, ": ", name,
              " must be dense in its last dim, got stride ", t.stride(-1));
  TORCH_CHECK(tpl_aligned16(t), fn, ": ", name,
              " must start at a 16-byte aligned address");
  for (int i = 0; i + 1 < t.dim(); ++i)
    TORCH_CHECK(t.size(i) == 1 || t.stride(i) % vec == 0, fn, ": ", name,
                " stride ", t.stride(i), " of dim ", i,
                " is not a multiple of 16 bytes");
}

const unsigned char* tpl_check_mask(const c10::optional<at::Tensor>& m,
                                    const at::Tensor& q,
                                    at::IntArrayRef shape, const char* fn,
                                    const char* name) {
  if (!m.has_value()) return nullptr;
  TORCH_CHECK(m->scalar_type() == at::kBool || m->scalar_type() == at::kByte,
              fn, ": ", name, " must be bool or uint8, got ",
              m->scalar_type());
  TORCH_CHECK(m->device() == q.device(), fn, ": ", name,
              " must be on q's device");
  TORCH_CHECK(m->sizes() == shape && m->is_contiguous(), fn, ": ", name,
              " must be contiguous with shape ", shape, ", got ", m->sizes());
  return static_cast<const unsigned char*>(m->data_ptr());
}

// checks q / kv / heads and fills the shape block; returns G = d / 8
int tpl_check(const at::Tensor& q, const at::Tensor& kv, long heads,
              const char* fn, TplShape* sh) {
  TORCH_CHECK(q.is_cuda() && kv.device() == q.device(), fn,
              ": q and kv must be on one GPU device");
  TORCH_CHECK(q.scalar_type() == at::kBFloat16 ||
              q.scalar_type() == at::kFloat, fn,
              ": q must be bf16 or fp32, got ", q.scalar_type());
  TORCH_CHECK(kv.scalar_type() == q.scalar_type(), fn,
              ": kv must have q's dtype (", q.scalar_type(), "), got ",
              kv.scalar_type());
  TORCH_CHECK(q.dim() == 3 && kv.dim() == 4 && q.numel() > 0 &&
              kv.numel() > 0, fn,
              ": q must be non-empty (b, P, H*d) and kv (b, T, P, 2*H*d)");
  const long b = q.size(0), P = q.size(1), C = q.size(2);
  TORCH_CHECK(heads >= 1 && C % heads == 0, fn, ": channels ", C,
              " do not split into ", heads, " heads");
  const long d = C / heads;
  TORCH_CHECK(d == 8 || d == 16 || d == 32 || d == 64, fn,
              ": head dim must be 8, 16, 32 or 64, got ", d);
  TORCH_CHECK(kv.size(0) == b && kv.size(2) == P && kv.size(3) == 2 * C, fn,
              ": kv must be (", b, ", T, ", P, ", ", 2 * C, "), got ",
              kv.sizes());
  TORCH_CHECK(kv.size(1) <= INT_MAX && C <= INT_MAX / 2, fn,
              ": shape too large");
  tpl_check_rows(q, fn, "q");
  tpl_check_rows(kv, fn, "kv");
  sh->P = P;
  sh->T = (int)kv.size(1);
  sh->C = (int)C;
  sh->LP = (int)(C / 8);
  sh->total = b * P * sh->LP;
  sh->q_bs = q.stride(0);
  sh->q_rs = q.stride(1);
  sh->kv_bs = kv.stride(0);
  sh->kv_ts = kv.stride(1);
  sh->kv_rs = kv.stride(2);
  TORCH_CHECK((sh->total + TPL_BLOCK - 1) / TPL_BLOCK <= INT_MAX, fn,
              ": too many positions for one launch");
  return (int)(d / 8);
}

void tpl_check_launch(const char* fn) {
  const hipError_t err = hipGetLastError();
  TORCH_CHECK(err == hipSuccess, fn, ": launch failed: ",
              hipGetErrorString(err));
}

}  // namespace

#define TPL_DISPATCH(LAUNCH)                                                \
  do {                                                                      \
    if (q.scalar_type() == at::kBFloat16) {                                 \
      if (G == 1) LAUNCH(__hip_bfloat16, 1);                                \
      else if (G == 2) LAUNCH(__hip_bfloat16, 2);                           \
      else if (G == 4) LAUNCH(__hip_bfloat16, 4);                           \
      else LAUNCH(__hip_bfloat16, 8);                                       \
    } else {                                                                \
      if (G == 1) LAUNCH(float, 1);                                         \
      else if (G == 2) LAUNCH(float, 2);                                    \
      else if (G == 4) LAUNCH(float, 4);                                    \
      else LAUNCH(float, 8);                                                \
    }                                                                       \
  } while (0)

// -> [out (b, P, H*d), lse (b, P, H) fp32]
std::vector<at::Tensor> tplattn_fwd(at::Tensor q, at::Tensor kv, long heads,
                                    c10::optional<at::Tensor> key_mask,
                                    c10::optional<at::Tensor> query_mask) {
  const char* fn = "tplattn_fwd";
  TplShape sh;
  const int G = tpl_check(q, kv, heads, fn, &sh);
  const long b = q.size(0);
  const unsigned char* km =
      tpl_check_mask(key_mask, q, {b, (long)sh.T, sh.P}, fn, "key_mask");
  const unsigned char* qm =
      tpl_check_mask(query_mask, q, {b, sh.P}, fn, "query_mask");
  const float scale = 1.f / sqrtf((float)(sh.C / heads));

  auto out = at::empty({b, sh.P, (long)sh.C}, q.options());
  auto lse = at::empty({b, sh.P, heads}, q.options().dtype(at::kFloat));
  const long grid = (sh.total + TPL_BLOCK - 1) / TPL_BLOCK;
  auto stream = at::cuda::getCurrentHIPStream();
#define LAUNCH_FWD(T, GG)                                                   \
  hipLaunchKernelGGL((tplattn_fwd_kernel<T, GG>), dim3(grid),               \
                     dim3(TPL_BLOCK), 0, stream,                            \
                     reinterpret_cast<const T*>(q.data_ptr()),              \
                     reinterpret_cast<const T*>(kv.data_ptr()), km, qm,     \
                     reinterpret_cast<T*>(out.data_ptr()),                  \
                     lse.data_ptr<float>(), sh, scale)
  TPL_DISPATCH(LAUNCH_FWD);
#undef LAUNCH_FWD
  tpl_check_launch(fn);
  return {out, lse};
}

// -> [dq (b, P, H*d), dkv (b, T, P, 2*H*d)], both contiguous
std::vector<at::Tensor> tplattn_bwd(at::Tensor dout, at::Tensor q,
                                    at::Tensor kv, at::Tensor out,
                                    at::Tensor lse, long heads,
                                    c10::optional<at::Tensor> key_mask,
                                    c10::optional<at::Tensor> query_mask) {
  const char* fn = "tplattn_bwd";
  TplShape sh;
  const int G = tpl_check(q, kv, heads, fn, &sh);
  const long b = q.size(0);
  const unsigned char* km =
      tpl_check_mask(key_mask, q, {b, (long)sh.T, sh.P}, fn, "key_mask");
  const unsigned char* qm =
      tpl_check_mask(query_mask, q, {b, sh.P}, fn, "query_mask");
  for (const at::Tensor* t : {&dout, &out}) {
    TORCH_CHECK(t->scalar_type() == q.scalar_type() &&
                t->device() == q.device() && t->sizes() == q.sizes() &&
                t->is_contiguous() && tpl_aligned16(*t), fn,
                ": dout and out must be contiguous, 16-byte aligned, with "
                "q's dtype, device and shape");
  }
  TORCH_CHECK(lse.scalar_type() == at::kFloat && lse.device() == q.device() &&
              lse.is_contiguous() && lse.dim() == 3 && lse.size(0) == b &&
              lse.size(1) == sh.P && lse.size(2) == heads, fn,
              ": lse must be contiguous fp32 (", b, ", ", sh.P, ", ", heads,
              ")");
  const float scale = 1.f / sqrtf((float)(sh.C / heads));

  auto dq = at::empty({b, sh.P, (long)sh.C}, q.options());
  auto dkv = at::empty({b, (long)sh.T, sh.P, 2L * sh.C}, q.options());
  const long grid = (sh.total + TPL_BLOCK - 1) / TPL_BLOCK;
  auto stream = at::cuda::getCurrentHIPStream();
#define LAUNCH_BWD(T, GG)                                                   \
  hipLaunchKernelGGL((tplattn_bwd_kernel<T, GG>), dim3(grid),               \
                     dim3(TPL_BLOCK), 0, stream,                            \
                     reinterpret_cast<const T*>(dout.data_ptr()),           \
                     reinterpret_cast<const T*>(q.data_ptr()),              \
                     reinterpret_cast<const T*>(kv.data_ptr()),             \
                     reinterpret_cast<const T*>(out.data_ptr()),            \
                     lse.data_ptr<float>(), km, qm,                         \
                     reinterpret_cast<T*>(dq.data_ptr()),                   \
                     reinterpret_cast<T*>(dkv.data_ptr()), sh, scale)
  TPL_DISPATCH(LAUNCH_BWD);
#undef LAUNCH_BWD
  tpl_check_launch(fn);
  return {dq, dkv};
}

#undef TPL_DISPATCH
