// Per-epoch sampled-halo plan build (plan_build.hip) — bound into the
// extension module by kernels.hip.
#pragma once
#include <torch/extension.h>

namespace bns {

// Adds csr_gather_rows, csr_filter_cols, build_worklist and the two
// composite builders (halo_epoch_build, rows_halo_build) to the module.
void bind_plan_build(pybind11::module& m);

}  // namespace bns
