"""Writes tests/golden/unet_plan.json: what the U-Net's host-side planning functions return (workspace sizes, the feature layout,
parameter counts, the single-layer workspaces) -- recorded before the graph of the network moved into one table (csrc/unet_graph.h),
so that tests/test_unet_graph.py holds every later build to the same numbers.  Pure host code, no GPU; run from the repository
root on a build whose numbers are the ones to keep:  python tests/golden/make_golden_unet_plan.py"""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

SHAPES = [(1, 32, 32), (2, 32, 32), (1, 32, 64), (2, 64, 96), (3, 64, 64), (16, 64, 64), (16, 256, 256), (64, 256, 256)]
CLASSES = [1, 10, 32]
CONV_WORKSPACES = [(3, 4, 3), (768, 256, 3), (64, 128, 1)]
CONV_BACKWARD_WORKSPACES = [(1, 3, 8, 8, 4, 3, 1, 1), (2, 64, 16, 16, 128, 3, 2, 1), (2, 64, 16, 16, 128, 1, 2, 0)]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "unet_plan.json")


def record(lib):
    """the planning functions' answers as JSON-ready lists"""
    shapes = []
    for n, H, W in SHAPES:
        features = []
        for i in range(10):
            off, ch, fh, fw = C.c_size_t(), C.c_int32(), C.c_int32(), C.c_int32()
            assert lib.bn_unet_feature_layout(n, H, W, i, C.byref(off), C.byref(ch), C.byref(fh), C.byref(fw)) == 0
            features.append([off.value, ch.value, fh.value, fw.value])
        shapes.append({"shape": [n, H, W], "unet_workspace_bytes": lib.bn_unet_workspace_bytes(n, H, W),
                       "segtrain_workspace_bytes": lib.bn_segtrain_workspace_bytes(n, H, W), "features": features})
    return {"shapes": shapes,
            "param_count": [{"classes": c, "unet": lib.bn_unet_param_count(c), "segtrain": lib.bn_segtrain_param_count(c)} for c in CLASSES],
            "conv2d_workspace_bytes": [{"args": list(a), "bytes": lib.bn_unet_conv2d_workspace_bytes(*a)} for a in CONV_WORKSPACES],
            "conv2d_backward_workspace_bytes": [{"args": list(a), "bytes": lib.bn_segtrain_conv2d_backward_workspace_bytes(*a)}
                                                for a in CONV_BACKWARD_WORKSPACES]}


def main():
    from benchnav_amd import _capi
    out = {"what": "bn_unet_workspace_bytes, bn_segtrain_workspace_bytes and the ten bn_unet_feature_layout tuples (offset, channels, height, "
                   "width) per (num_maps, H, W); the parameter counts per class count; the single-layer workspaces per argument list"}
    out.update(record(_capi.load()))
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
