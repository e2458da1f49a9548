"""What tests/test_mppi_plan.py (CPU) and tests/test_gpu_mppi_plan.py share: the recorded golden, the plan export, and the
observables of a live handle restated from the plan by the formulas of csrc/mppi_query.cpp and bn_mppi_overlap_mode."""
import ctypes as C
import importlib.util
import json
import os

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_golden_mppi_plan", os.path.join(GOLDEN_DIR, "make_golden_mppi_plan.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

BUF = dict(STATES=0, WEIGHTS=1, COSTS=2, CONTROLS=3, USTAR=4, XSTAR=5, MEAN=6, MAP=7, GOAL=8, USTAR_XSTAR=9, STATES_ALT=10, CONTROLS_ALT=11)
BN_OK, BN_ERR_STATE = 0, -4


def golden():
    return json.load(open(gen.GOLDEN))


def plan(lib, capi, entry, n_cus):
    """(status, bn_mppi_plan_info as a dict) of bn_mppi_debug_plan."""
    cfg, info = gen.config(lib, capi, entry), capi.PlanInfo()
    info.struct_size = C.sizeof(capi.PlanInfo)
    status = lib.bn_mppi_debug_plan(C.byref(cfg), n_cus, C.byref(info))
    out = {name: getattr(info, name) for name, _ in capi.PlanInfo._fields_ if name != "buffer_bytes"}
    out["buffer_bytes"] = list(info.buffer_bytes)
    return status, out


def predict(entry, p):
    """The `observed` record of make_golden_mppi_plan.observe for a handle created from plan p."""
    flag = lambda name: name in entry.get("flags", ())
    K, T, G = entry.get("num_samples", 1024), entry.get("horizon", 50), entry.get("grid_size", 64)
    # bn_mppi_algorithmic_bytes: map, mean and state, the trajectory batch unless lean, weights, U* and X*; + injected noise; + stored controls
    base = 4 * G * G + (8 * T + 12) + (0 if flag("LEAN") else 12 * K * (T + 1)) + 4 * K + 8 * T + 12 * (T + 1) + (8 * K * T if flag("STORE_CONTROLS") else 0)
    alg = [base, base + 8 * K * T]
    W = p["WN"] if p["WN"] > 0 else G                  # ..._window: the map term replaced by the staged window
    capable = bool(p["lat_kernel"] or p["role_overlap"] or p["ticket_overlap"]) and p["n_streams"] > 1 and not (flag("PROFILE") or flag("NO_OVERLAP"))
    # paced_setup's conditions, bar the stream probe
    paces = (flag("HOST_PACED") and entry.get("num_instances", 1) == 1 and p["lat_kernel"] and p["has_granules"] and p["may_overlap"]
             and p["n_streams"] > 1 and not p["slip_on"] and not (flag("NO_PIPELINE") or flag("PROFILE")))
    present = {name: True for name in BUF}
    present.update(STATES=bool(p["has_X"]), CONTROLS=bool(p["has_U"]), STATES_ALT=bool(p["has_alt"] and p["has_X"]),
                   CONTROLS_ALT=bool(p["has_alt"] and p["has_U"]))
    by_id = sorted(BUF, key=BUF.get)
    return dict(status=BN_OK, arithmetic=p["ref_order"], launches_per_solve=1 if (p["pipelined"] or p["ticket_mode"]) else 2,
                launches_per_forward=1 if (p["lat_kernel"] and p["pipelined"] and not flag("NO_PIPELINE")) else 2,
                host_paced=int(bool(paces)), row_pitch=p["Kp"], fast_quotient=2 if p["pow2"] else 1, never_overlaps=int(not capable),
                algorithmic_bytes=alg, algorithmic_bytes_window=[a - 4 * G * G + 4 * W * W for a in alg],
                buffers=[[BN_OK if present[name] else BN_ERR_STATE, p["buffer_bytes"][BUF[name]]] for name in by_id])


def comparable(observed):
    """An observed record with what depends on the machine, not on the plan, reduced to what the plan decides: host pacing counts as
    "paces or not" (1 or 2 says whether the platform offers device memory the CPU may write)."""
    out = dict(observed)
    if "host_paced" in out:
        out["host_paced"] = int(out["host_paced"] > 0)
    return out
