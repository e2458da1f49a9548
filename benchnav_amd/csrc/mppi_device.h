// mppi_device.h -- everything the rollout kernels (rollout_*.inc, rollout_sampled.hip) and mppi_kernels.hip share, one header per
// concern.  Everything in them has internal linkage (anonymous namespace); each .hip file instantiates what it launches.
#pragma once
#include "mppi_stamps.h"
#include "mppi_geometry.h"
#include "mppi_grid.h"
#include "mppi_chain.h"
#include "mppi_env_step.h"
#include "mppi_slip.h"
#include "mppi_sync.h"
#include "mppi_merge.h"
#include "mppi_tail.h"
#include "mppi_noise.h"
#include "rollout_launch.h"
