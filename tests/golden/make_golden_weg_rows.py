"""Writes tests/golden/weg_rows_loop.npz: the oracle's record of the per-row WEG loop case (tests/weg_rows_ref.py, LOOP) -- per guided
iteration the rows' returned losses, their refinement rounds and every loss a decision compared (NaN-padded).  No reference import: the
oracle alone.  Run from the repository root: python tests/golden/make_golden_weg_rows.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from tests import weg_rows_ref  # noqa: E402

if __name__ == "__main__":
    _, _, log = weg_rows_ref.loop_oracle()
    B = weg_rows_ref.LOOP["B"]
    width = max(len(s) for e in log for s in e["evaluated"])
    evaluated = np.full((len(log), B, width), np.nan, dtype=np.float64)
    for k, e in enumerate(log):
        for b, s in enumerate(e["evaluated"]):
            evaluated[k, b, :len(s)] = s
    target = 1.0 - list(weg_rows_ref.LOOP["params"]["thresholds"].values())[0]
    it = list(weg_rows_ref.LOOP["params"]["thresholds"])[0]
    # (the closing evaluation of a row that entered refinement is compared with 0 only)
    compared = [v for e in log if e["i"] == it for s in e["evaluated"] for v in (s[:-1] if len(s) > 1 else s)]
    margin = float(np.min(np.abs(np.array(compared) - target)))
    print("rounds", [e["rounds"] for e in log], "closest compared loss to the target", margin)
    assert margin >= 1e-3
    np.savez(os.path.join(os.path.dirname(os.path.abspath(__file__)), "weg_rows_loop.npz"), iterations=np.array([e["i"] for e in log]),
             losses=np.array([e["losses"] for e in log], dtype=np.float64), rounds=np.array([e["rounds"] for e in log], dtype=np.int64),
             evaluated=evaluated)
