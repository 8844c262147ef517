// Host side of the work-list contract (common.h), shared by the launchers
// of kernels.hip and gatv2.hip.
#pragma once
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>
#include "common.h"

inline void check_f32(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() &&
                  t.scalar_type() == at::kFloat,
              name, " must be contiguous fp32 CUDA tensor");
}

// The four schedule arrays as built by ops/csr_torch.build_worklist,
// validated once for every entry point. n_waves % 8 == 0 is what lets each
// launcher size its grid as n_waves / (waves per 256-thread block) without
// a remainder — a schedule that broke it would silently skip its last
// items.
struct WorkListArgs {
  WorkList wl;
  int n_waves;
};

inline WorkListArgs worklist_args(const at::Tensor& wrow,
                                  const at::Tensor& wbeg,
                                  const at::Tensor& wend,
                                  const at::Tensor& wave_start) {
  TORCH_CHECK(wrow.scalar_type() == at::kInt &&
                  wbeg.scalar_type() == at::kLong &&
                  wend.scalar_type() == at::kLong &&
                  wave_start.scalar_type() == at::kInt,
              "worklist: wrow/wave_start int32 and wbeg/wend int64 expected");
  for (const at::Tensor* t : {&wrow, &wbeg, &wend, &wave_start})
    TORCH_CHECK(t->is_cuda() && t->is_contiguous() &&
                    t->device() == wave_start.device(),
                "worklist arrays must be contiguous CUDA tensors on one "
                "device");
  // array-length consistency: the kernels index wbeg/wend by item id
  TORCH_CHECK(wave_start.numel() >= 1 && wbeg.numel() == wrow.numel() &&
                  wend.numel() == wrow.numel(),
              "worklist: inconsistent array lengths (wrow ", wrow.numel(),
              ", wbeg ", wbeg.numel(), ", wend ", wend.numel(),
              ", wave_start ", wave_start.numel(), ")");
  const int n_waves = (int)wave_start.numel() - 1;
  TORCH_CHECK(n_waves % 8 == 0, "worklist: n_waves (", n_waves,
              ") must be a multiple of 8");
  return {{wrow.data_ptr<int32_t>(), wbeg.data_ptr<int64_t>(),
           wend.data_ptr<int64_t>(), wave_start.data_ptr<int32_t>()},
          n_waves};
}

// One work-list kernel launch: 256-thread blocks of 256 / subw waves (or
// subgroups) each; the schedule pointers lead the argument list.
template <typename K, typename... Args>
void launch_worklist(K kernel, const WorkListArgs& w, int subw,
                     Args... args) {
  hipLaunchKernelGGL(kernel, dim3(w.n_waves / (256 / subw)), dim3(256), 0,
                     at::cuda::getCurrentCUDAStream(), w.wl.row, w.wl.beg,
                     w.wl.end, w.wl.wave_start, args...);
}
