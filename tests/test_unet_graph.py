"""CPU: the U-Net's host-side plans -- workspace sizes, the feature layout with its offsets, parameter counts and the single-layer
workspaces -- equal tests/golden/unet_plan.json, recorded before the network's graph moved into one table (csrc/unet_graph.h).
Pure host code: none of these functions touches a device."""
import importlib.util
import json
import os

from benchnav_amd import _capi

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_plans_equal_the_recorded_ones():
    spec = importlib.util.spec_from_file_location("make_golden_unet_plan", os.path.join(GOLDEN_DIR, "make_golden_unet_plan.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    want = json.load(open(gen.GOLDEN))
    assert [tuple(s["shape"]) for s in want["shapes"]] == [(1, 32, 32), (2, 32, 32), (1, 32, 64), (2, 64, 96), (3, 64, 64), (16, 64, 64),
                                                           (16, 256, 256), (64, 256, 256)]
    assert [p["classes"] for p in want["param_count"]] == [1, 10, 32]
    assert [tuple(c["args"]) for c in want["conv2d_workspace_bytes"]] == [(3, 4, 3), (768, 256, 3), (64, 128, 1)]
    assert [tuple(c["args"]) for c in want["conv2d_backward_workspace_bytes"]] == [(1, 3, 8, 8, 4, 3, 1, 1), (2, 64, 16, 16, 128, 3, 2, 1),
                                                                                   (2, 64, 16, 16, 128, 1, 2, 0)]
    assert want["shapes"][0]["segtrain_workspace_bytes"] == 0 and all(s["segtrain_workspace_bytes"] > 0 for s in want["shapes"][1:])
    got = gen.record(_capi.load())
    for key in ("param_count", "conv2d_workspace_bytes", "conv2d_backward_workspace_bytes"):
        assert got[key] == want[key], key
    for g, w in zip(got["shapes"], want["shapes"]):
        assert g == w, w["shape"]


def test_conv_inputs_walks_the_same_graph():
    """unet.conv_inputs at 64 x 64: the input side of each of the 31 convolutions, the decoder's skip channels and upsamples."""
    from benchnav_amd import unet
    got = unet.conv_inputs(10, 64)
    assert [s for s, _, _ in got] == [64, 16, 16, 16, 16, 16, 8, 16, 8, 8, 8, 4, 8, 4, 4, 4, 2, 4, 2, 2, 4, 4, 8, 8, 16, 16, 32, 32, 64, 64, 64]
    assert [(i, cb) for i, (_, cb, up) in enumerate(got) if up] == [(20, 256), (22, 128), (24, 64), (26, 64), (28, 0)]
    assert all(cb == 0 for _, cb, up in got if not up)
    assert [s for s, _, _ in unet.conv_inputs(10, 256)] == [4 * s for s, _, _ in got]
