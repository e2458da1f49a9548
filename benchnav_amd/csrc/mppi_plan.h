// mppi_plan.h -- everything bn_mppi_create decides, decided before the device is touched: the argument checks, the derived
// SolveParams scalars, the launch policy (which kernel family, what may overlap, how many streams) and which conditional buffer
// groups the handle gets.  plan_mppi makes no HIP call and reads no handle, so tests/test_mppi_plan.py holds it to a recorded
// golden without a GPU (bn_mppi_debug_plan).  Private, host only, not installed.
#pragma once
#include "mppi_handle.h"

// The policy bits, the buffer groups (has_*: bn_mppi_create registers them under exactly these) and buffer_bytes -- what
// bn_mppi_device_buffer reports per bn_buffer_id, the one place these sizes are written -- are the public bn_mppi_plan_info's
// fields (include/benchnav_mppi.h), which also shows the scalars of p that plan_mppi derives.
struct MppiPlan : bn_mppi_plan_info {
    bn::SolveParams p{};             // every scalar derived from the configuration; the pointers stay null until create has allocated
};

namespace bn {
namespace host __attribute__((visibility("hidden"))) {

// BN_OK and *out, or the error bn_mppi_create reports for this configuration on a device of n_cus compute units
int plan_mppi(const bn_mppi_config &cfg, int n_cus, MppiPlan *out);

}  // namespace host
}  // namespace bn
