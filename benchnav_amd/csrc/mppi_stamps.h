// mppi_stamps.h -- the kernels' measurement hooks: empty statements in the shipped library, csrc/experiments.h in the measurement builds.
#pragma once

// In-kernel time stamps and per-workgroup traces (BN_STAMP, BN_WSTAMP, BN_TRACE_*, BN_TIMING_DO(statements)): compiled in by the measurement builds only
// (-DBN_EXPERIMENTS -DBN_TIMING, tools/stamps*.py, tools/block_trace*.py); csrc/experiments.h holds them, the shipped library sees
// empty statements.  Round 5 took everything else of the lab bench out of the kernels: the ablation and critical-path switches
// (BN_ABLATE, BN_VAR_*: compile-time bit tests inside the arithmetic) and the alternative cuts they selected are gone from the
// sources -- the measurements they produced are in DESIGN_NOTEBOOK.md, the code that produced them in the history (round 4's head).
#ifdef BN_EXPERIMENTS
#include "experiments.h"
#else
#define BN_STAMP(slot) do { } while (0)
#define BN_STAMP_ANY(slot) do { } while (0)
#define BN_WSTAMP(i) do { } while (0)
#define BN_TRACE_BEGIN() do { } while (0)
#define BN_TRACE_END() do { } while (0)
#define BN_TIMING_DO(...)
#define BN_SSTAMP(i) do { } while (0)
#endif
