"""Records tests/golden/mppi_tail.json: per case of mppi_tail_cases.yardstick_cases(), how much of the derived bound of
tests/mppi_tail_spec.py the float32 CPU oracle (oracle/mppi_oracle.c) uses -- its distance to the float64 spec over the bound, for
the weights, for U* and for the sum of the weights -- with the case's K, T, lambda and z spread.  Needs no GPU:

    python tests/golden/make_golden_mppi_tail.py

The numbers are yardsticks: the device's measured / bound (printed by tests/test_gpu_mppi_tail.py) reads against them.  The one-hot
cases are not recorded: oracle and spec agree exactly there."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "mppi_tail.json")


def record(case):
    import mppi_tail_cases as TC
    from mppi_tail_spec import ratios, tail
    orc = TC.reference(case)
    spec = tail(orc["cost"], orc["U"], case["lam"])
    r = ratios(orc["w"], orc["Ustar"], spec)
    return dict(K=case["K"], T=case["T"], lam=case["lam"], z_spread=spec["spread"], oracle_w_over_bound=r["w"], oracle_Ustar_over_bound=r["U"],
                oracle_sum_over_bound=r["sum"], w_bound_max=float(spec["w_bound"].max()), Ustar_bound_max=float(spec["U_bound"].max()))


def main():
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import mppi_tail_cases as TC
    out = dict(what="per case: the float32 CPU oracle's distance to the float64 spec over the derived bound (mppi_tail_spec.tail), and the "
                    "largest bound of a weight and of an element of U*",
               cases={c["name"]: record(c) for c in TC.yardstick_cases()})
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{GOLDEN}: {len(out['cases'])} cases")


if __name__ == "__main__":
    main()
