"""Writes tests/golden/policy_small.json: plans of the numpy restatement of SPEC.md 2.6
(tests/policy_ref.py) on small generator scenarios, one per strategy, pinned so that a change to the
reference itself fails a test.  Run from the repository root: python tests/golden/make_policy_golden.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import policy_ref as R  # noqa: E402
from oracle import oracle as O  # noqa: E402

CASES = [(0x5EED0004, 3, 40, 9, 7, R.FIRST_FIT, 0), (0x5EED0004, 3, 40, 9, 7, R.SPREAD, 0),
         (0x5EED0004, 3, 40, 9, 7, R.PACK, 0), (0x5EED0004, 3, 40, 9, 7, R.FILL_LOWEST, 0),
         (0x5EED0004, 5, 30, 7, 0, R.SPREAD, (1 << 4) | (1 << 8))]


def main():
    cases = []
    for seed, scen, C, N, flags, strategy, pref in CASES:
        cont, nodes = O.gen_scenario(seed, scen, C, N, flags)
        a, r, after, cnt = R.place(cont, nodes, strategy, preferred=pref)
        cases.append({"seed": seed, "scenario": scen, "C": C, "N": N, "flags": flags, "strategy": strategy,
                      "preferred": pref, "assign": a.tolist(), "reason": r.tolist(), "node_count": cnt.tolist(),
                      "cpu_free": after[0].tolist()})
    with open(os.path.join(HERE, "policy_small.json"), "w") as f:
        json.dump({"cases": cases}, f, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
