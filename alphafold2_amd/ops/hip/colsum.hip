// The fixed-order fold of colsum.h as an entry point of its own (tests,
// tools/reduce_bench.py) -- gfx950.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "colsum.h"

// The fixed-order fold of colsum.h on its own: (nb, C) fp32 partial rows
// -> (C,), or added into accumulate_into (C,) in place.  v1 keeps the
// scalar body (what AF2AMD_COLSUM_FOLD_V1=1 selects everywhere).
at::Tensor colsum_fold(at::Tensor part,
                       c10::optional<at::Tensor> accumulate_into, bool v1) {
  TORCH_CHECK(part.is_cuda() && part.scalar_type() == at::kFloat &&
              part.is_contiguous() && part.dim() == 2 && part.size(0) >= 1 &&
              part.size(1) >= 1,
              "colsum_fold: part must be contiguous fp32 (nb, C)");
  const long nb = part.size(0), C = part.size(1);
  TORCH_CHECK(nb <= INT_MAX && C <= INT_MAX, "colsum_fold: nb, C must fit int");
  at::Tensor out;
  if (accumulate_into.has_value()) {
    out = *accumulate_into;
    TORCH_CHECK(out.is_cuda() && out.device() == part.device() &&
                out.scalar_type() == at::kFloat && out.is_contiguous() &&
                out.numel() == C,
                "colsum_fold: accumulate_into must be contiguous fp32 (C,)");
  } else {
    out = at::empty({C}, part.options());
  }
  colsum_fold_launch(part.data_ptr<float>(), out.data_ptr<float>(), nb, C,
                     accumulate_into.has_value(),
                     at::cuda::getCurrentHIPStream(), v1);
  const hipError_t err = hipGetLastError();
  TORCH_CHECK(err == hipSuccess, "colsum_fold: launch failed: ",
              hipGetErrorString(err));
  return out;
}
