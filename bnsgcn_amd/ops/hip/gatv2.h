// GATv2 attention score kernels (gatv2.hip) — bound into the extension
// module by kernels.hip.
#pragma once
#include <torch/extension.h>

namespace bns {

// Adds gatv2_score and gatv2_score_bwd to the module.
void bind_gatv2(pybind11::module& m);

}  // namespace bns
