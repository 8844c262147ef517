// Fused SyncBatchNorm + ReLU + dropout (bn_fused.hip) — bound into the
// extension module by kernels.hip.
#pragma once
#include <torch/extension.h>

namespace bns {

// Adds bn_colsums_fwd, bn_finalize, bn_act_drop_fwd, bn_colsums_bwd and
// bn_act_drop_bwd_dx to the module.
void bind_bn_fused(pybind11::module& m);

}  // namespace bns
