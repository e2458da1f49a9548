// rollout_launch.h -- host helpers of the kernel translation units' launchers, and the launchers that live in their own
// translation units.
#pragma once
#include "mppi_kernels.h"
#include "mppi_geometry.h"

namespace bn {

namespace {

template <typename Kern>
hipError_t ensure_lds(Kern kern, size_t bytes)
{
    if (bytes <= 48 * 1024) return hipSuccess;
    return hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

int geo_of(const SolveParams &p)
{
    if (!p.pow2) return kGeoGeneral;
    return (p.x0 == 0.0f && p.y0 == 0.0f) ? kGeoPow2Origin0 : kGeoPow2;
}

static int grid_for(size_t n) { return (int)((n + 255) / 256 > 2048 ? 2048 : (n + 255) / 256); }

}  // namespace

// launchers that live in their own translation units (one per kernel family)
hipError_t launch_rollout_role_philox(const SolveParams &p, hipStream_t s);
hipError_t launch_rollout_role_kt2(const SolveParams &p, hipStream_t s);
hipError_t launch_rollout_role_t2k(const SolveParams &p, hipStream_t s);
hipError_t launch_rollout_lat_self_philox(const SolveParams &p, hipStream_t s);    // rollout_lat_self_*.hip
hipError_t launch_rollout_lat_self_kt2(const SolveParams &p, hipStream_t s);
hipError_t launch_rollout_lat_self_t2k(const SolveParams &p, hipStream_t s);
hipError_t launch_rollout_lat_self_ref_philox(const SolveParams &p, hipStream_t s);
hipError_t launch_rollout_lat_self_ref_kt2(const SolveParams &p, hipStream_t s);
hipError_t launch_rollout_lat_self_ref_t2k(const SolveParams &p, hipStream_t s);
hipError_t launch_rollout_role_ref_philox(const SolveParams &p, hipStream_t s);   // rollout_role_ref_*.hip: BN_FLAG_REFERENCE_ORDER
hipError_t launch_rollout_role_ref_kt2(const SolveParams &p, hipStream_t s);
hipError_t launch_rollout_role_ref_t2k(const SolveParams &p, hipStream_t s);
hipError_t launch_rollout_wave(const SolveParams &p, EpsMode mode, hipStream_t s);
hipError_t launch_rollout_wave_ref(const SolveParams &p, EpsMode mode, hipStream_t s);   // rollout_wave_ref.hip

}  // namespace bn
