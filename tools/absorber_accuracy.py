#!/usr/bin/env python3
"""The absorber rule's transmission (include/qfa_hip.h, qfa_absorber_mask_f32: the Tepper-Garcia form of the Voigt function)
against exp(-tau) with the Voigt function itself, H = Re w(x + i a) (scipy.special.wofz), on the CPU in float64:
tests/_absorber_ref.py accuracy_against_faddeeva.  Writes profiles/absorber_accuracy.txt, whose figures times 1.5 are the bars of
tests/test_absorbers_cpu.py (float64 on the CPU is deterministic).

    python tools/absorber_accuracy.py [--out profiles/absorber_accuracy.txt]
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

import _absorber_ref as R  # noqa: E402

CASES = [(lg, b, lyb) for lyb in (True, False) for lg in (20.3, 21.0, 22.0) for b in (10.0, 30.0)]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "absorber_accuracy.txt"))
    a = ap.parse_args(argv)
    lines = ["# max |T_rule - T_Faddeeva| over the kept pixels (T_rule >= t_min = 0.8) of one absorber at z_abs = 2.5; observed",
             "# wavelengths 3400 .. 5200 A in steps of 0.02 A plus 2 000 points across every step that crosses t_min.",
             "# float64 on the CPU (numpy, scipy.special.wofz).  tools/absorber_accuracy.py",
             "# log_nhi  b_kms  lines          max|dT|      min(T - t_min)  points"]
    for lg, b, lyb in CASES:
        d, edge, n = R.accuracy_against_faddeeva(lg, b, lyb)
        lines.append(f"{lg:8.1f}  {b:5.0f}  {'Lya+Lyb' if lyb else 'Lya    '}  {d:14.6e}  {edge:14.3e}  {n}")
    lines.append("# the small-P series against the main form at the switch P = 1/16, and H(a, 0) against the Faddeeva function")
    lines.append("# b_kms  lam0      a             series - main   H(a,0) - Re w(ia)")
    for b in (10.0, 30.0):
        for lam0, _, gamma in R.LINES:
            aa = R.damping(lam0, gamma, b)
            ka = aa / np.sqrt(np.pi)
            P = np.array([R.P_SERIES])
            join = float((R.voigt_series(ka, P) - R.voigt_main(ka, P))[0])
            h0 = float((R.voigt_h(aa, np.zeros(1)) - R.voigt_faddeeva(aa, np.zeros(1)))[0])
            lines.append(f"{b:7.0f}  {lam0:8.2f}  {aa:.6e}  {join:14.3e}  {h0:14.3e}")
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
