// episode_log.h -- the log of a closed loop on the MPPI handle: the fused MPPI episode (mppi_env.cpp), the A* + DWA loop and the
// CL-RRT loop (mppi_loops.cpp).  One device block, laid out by the rows it holds (cap), not by the rows the latest call ran (len):
//   states (cap + 1, B, 3), row 0 the call's start | rewards (cap, B) | actions (cap, B, 2) | the loop's own 4-byte columns (cap, B)
// The one place the layout is written: the entry points size, fill, view and copy the log through it.  Host only.
#pragma once
#include "bn_host.h"
#include "episode_rows.h"

namespace bn {
namespace {

struct EpisodeLog {
    float *block = nullptr;
    size_t B = 0;
    int n_extra = 0;             // 4-byte columns per row behind the three common ones
    int cap = 0, len = 0;        // rows the block holds / the latest call ran (the MPPI episode: steps enqueued so far)

    // the block joins its concern's group; the first reserve allocates it
    void attach(DeviceBuffers &bufs, size_t B_, int n_extra_) { B = B_; n_extra = n_extra_; bufs.add_later(&block); }
    bool empty() const { return !block || len < 1; }
    size_t floats(size_t n) const { return (n + 1) * B * 3 + n * B * (3 + n_extra); }
    size_t rows() const { return (size_t)len * B; }                                     // elements of one column of the latest call
    float *states() const { return block; }
    float *reward() const { return block + ((size_t)cap + 1) * B * 3; }
    float *action() const { return reward() + (size_t)cap * B; }
    float *extra(int k) const { return action() + (size_t)cap * B * (2 + k); }
    EpisodeRows columns() const { return EpisodeRows{states(), reward(), action()}; }

    // Room for a call of n rows.  Growing drops the contents: the previous call's kernels on `s` may still write the old block, and
    // the new block's zero fill runs on the null stream (fills_done, mppi_handle.h).
    template <typename Fail>
    int reserve(DeviceBuffers &bufs, hipStream_t s, int n, Fail fail)
    {
        if (n <= cap) return BN_OK;
        BN_HIP_OR(fail, hipStreamSynchronize(s));
        cap = 0;
        if (int rc = bufs.resize(&block, floats((size_t)n) * sizeof(float), fail)) return rc;
        if (hipStreamSynchronize(nullptr) != hipSuccess) return fail(BN_ERR_HIP, "hipStreamSynchronize failed behind an allocation");
        cap = n;
        return BN_OK;
    }

    // the latest call's rows of the common columns, each destination optional (the stream has been synchronised)
    template <typename Fail>
    int copy_out(float *states_host, float *rewards_host, float *actions_host, Fail fail) const
    {
        if (states_host) BN_HIP_OR(fail, hipMemcpy(states_host, states(), (rows() + B) * 3 * sizeof(float), hipMemcpyDeviceToHost));
        if (rewards_host) BN_HIP_OR(fail, hipMemcpy(rewards_host, reward(), rows() * sizeof(float), hipMemcpyDeviceToHost));
        if (actions_host) BN_HIP_OR(fail, hipMemcpy(actions_host, action(), rows() * 2 * sizeof(float), hipMemcpyDeviceToHost));
        return BN_OK;
    }
};

}  // namespace
}  // namespace bn
