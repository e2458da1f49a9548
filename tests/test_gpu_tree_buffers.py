"""GPU: the device buffers of the bn_rrt and bn_clrrt handles, as bn_*_device_buffer hands them out: every public id, the size
include/benchnav_mppi.h documents for it, distinct pointers, the rejection of an id past the last, and destroy on a handle that
has planned and on fresh ones.  The shapes are the smallest at which a size can go wrong: B = 2, max_iterations = 3 (and for
CL-RRT max_seqs = 2, path_cap = 5), so that B, max_iterations, max_iterations + 1, max_seqs, max_seqs + 1, path_cap and
path_cap + 1 are all different numbers and a swapped factor changes the product."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import clrrt_cases as Cs

pytestmark = pytest.mark.gpu

B, I, S, P = 2, 3, 2, 5
F4 = I4 = U4 = 4
F8 = 8
# id name -> (shape as the header's comment on the id gives it, bytes per element)
RRT_BUFFERS = {
    "NODES": ((B, I + 1, 2), F4), "EDGES": ((B, I + 1), I4), "COSTS": ((B, I + 1), F4), "COUNTS": ((B,), I4),
    "SAMPLES": ((B, I, 2), F4), "SAMPLE_FLAGS": ((B, I), I4),
    "PATHS": ((B, I + 1, 2), F4),                            # path_cap = 0 in the config: max_iterations + 1
    "RESULTS": ((B, 4), I4),
}
CLRRT_BUFFERS = {
    "NODES": ((B, I + 1, 3), F4), "EDGES": ((B, I + 1), I4), "COSTS": ((B, I + 1), F4), "COUNTS": ((B,), I4),
    "SEQ_LENGTHS": ((B, I + 1), I4), "CONTROLLERS": ((B, I + 1, 4), F4), "ACTION_SEQS": ((B, I + 1, S, 2), F4),
    "STATE_SEQS": ((B, I + 1, S + 1, 3), F4), "SAMPLES": ((B, I, 3), F4), "SAMPLE_FLAGS": ((B, I), I4), "NEAREST": ((B, I), I4),
    "FEASIBLE": ((B, I), I4), "PATH_ACTIONS": ((B, P, 2), F4), "PATH_STATES": ((B, P + 1, 3), F4), "RESULTS": ((B, 6), I4),
    "STEER_ACTIONS": ((B, S, 2), F4), "STEER_STATES": ((B, S + 1, 3), F4), "STEER_PATHS": ((B, 64, 2), F8), "STEER_TARGETS": ((B, S), I4),
    "STEER_RESULTS": ((B, 4), I4), "STEER_COSTS": ((B,), F4), "STEER_CONTROLLERS": ((B, 4), F8), "MT_STATE": ((B, 624), U4),
    "MT_POS": ((B,), I4),
}


def _rrt():
    from benchnav_amd import RRT
    gm = types.SimpleNamespace(resolution=0.5, x_limits=(0.0, 32.0), y_limits=(0.0, 32.0))
    pl = RRT(gm, torch.tensor([24.0, 24.0]), max_iterations=I)
    return pl, lambda: pl.plan_batch(np.float32([[8.0, 8.0], [9.0, 9.5]]), None, [1, 2])


def _clrrt():
    pl = Cs.planner(0, max_iterations=I, max_seqs=S, path_cap=P)
    return pl, lambda: pl.plan_batch(np.float32([[8.0, 8.0, 0.3], [9.0, 9.5, 1.0]]), None, [1, 2])


@pytest.mark.parametrize("family, prefix, table, make, unknown", [
    ("rrt", "BN_RRT_BUF_", RRT_BUFFERS, _rrt, "unknown RRT buffer id"),
    ("clrrt", "BN_CLRRT_BUF_", CLRRT_BUFFERS, _clrrt, "unknown CL-RRT buffer id"),
])
def test_every_public_buffer_has_its_documented_size_and_its_own_memory(family, prefix, table, make, unknown):
    from benchnav_amd import _capi
    ids = {name: getattr(_capi, prefix + name) for name in table}
    assert sorted(ids.values()) == list(range(len(table))), "the table above names every public id of the family"
    pl, plan = make()
    lib = pl._lib
    device_buffer, last_error = getattr(lib, f"bn_{family}_device_buffer"), getattr(lib, f"bn_{family}_last_error")

    def check_handle(h):
        seen = {}
        for name, (shape, item) in table.items():
            ptr, nbytes = C.c_void_p(), C.c_size_t()
            assert device_buffer(h.h, ids[name], C.byref(ptr), C.byref(nbytes)) == _capi.BN_OK, name
            assert ptr.value, name
            assert ptr.value not in seen, f"{name} shares its pointer with {seen.get(ptr.value)}"
            seen[ptr.value] = name
            assert nbytes.value == int(np.prod(shape)) * item, f"{name}: {nbytes.value} bytes for {shape} x {item}"
        ptr, nbytes = C.c_void_p(), C.c_size_t()
        for bad in (len(table), -1):                      # one past the last; and the id the internal buffers carry
            assert device_buffer(h.h, bad, C.byref(ptr), C.byref(nbytes)) == _capi.BN_ERR_INVALID
            assert last_error().decode() == unknown

    h = pl._handle(B)
    check_handle(h)
    plan()                                                # one plan_async and the wait for it: every buffer has been in use
    check_handle(h)
    del pl._handles[B]
    h.close()                                             # destroy a handle that has planned ...
    assert not h.h
    for _ in range(2):                                    # ... and fresh ones, twice in a row
        h = pl._handle_type(lib, pl._dev, B, pl)
        check_handle(h)
        h.close()
        assert not h.h
