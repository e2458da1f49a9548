// gp_handle.h -- the layout of one GP slip regressor on the device, shared by the files that fill it (gp_kernels.hip from host
// arrays, gp_fit_kernels.hip from its own factorisation) and by the predict kernels that read it.  Private to csrc/.
#pragma once
#include <cstdint>

#include "bn_host.h"

namespace bn {
namespace {

// one class's regressor as the predict kernel reads it
struct GpRegDev {
    const double *x, *alpha;             // (npad), zero beyond n
    const double *linv;                  // L^-1 in fragment order: row block i, k step j (j < 4 (i + 1)), lane
    int32_t n, npad;                     // npad: n rounded up to 16
    double c, s, q, noise;               // q = -1 / (2 l^2)
};

}  // namespace
}  // namespace bn

struct bn_gp {
    int device = 0, n = 0, npad = 0;
    double c = 0, s = 0, l = 0, noise = 0;
    bn::DeviceBuffers bufs;
    double *x = nullptr, *alpha = nullptr, *linv = nullptr;
};

namespace bn {
namespace {

// The layout of a regressor of g->n points, written once: npad, and the three buffers entered in the table.  Returns the
// number of doubles of L^-1 in fragment order (nb (nb + 1) fragments of 128, nb = npad / 16).
size_t gp_layout(bn_gp *g)
{
    g->npad = (g->n + 15) / 16 * 16;
    const size_t nb = (size_t)g->npad / 16, frag = 128 * nb * (nb + 1);
    g->bufs.add(&g->x, (size_t)g->npad * 8);
    g->bufs.add(&g->alpha, (size_t)g->npad * 8);
    g->bufs.add(&g->linv, frag * 8);
    return frag;
}

}  // namespace
}  // namespace bn
