// Per-epoch boundary-node selection (bns_select.hip) — bound into the
// extension module by kernels.hip.
#pragma once
#include <torch/extension.h>

namespace bns {

// Adds bns_select_philox, bns_select_raw, BNS_SELECT_CAP and
// BNS_SELECT_SLICE_MIN to the module.
void bind_bns_select(pybind11::module& m);

}  // namespace bns
