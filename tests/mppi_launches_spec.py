"""What tests/test_mppi_launches.py (CPU) and tests/test_gpu_mppi_launches.py share: the recorded launch logs and their recipe."""
import importlib.util
import json
import os

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_golden_mppi_launches", os.path.join(GOLDEN_DIR, "make_golden_mppi_launches.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


def golden():
    return json.load(open(gen.GOLDEN))


def path_key(entry, decided, arithmetic, host_paced):
    """What tells two launch paths apart (the grouping of the recipe)."""
    flags = entry.get("flags", ())
    return tuple(decided[k] for k in gen.PATH_KEY) + tuple(f in flags for f in gen.PATH_FLAGS) + (arithmetic, int(host_paced > 0))
