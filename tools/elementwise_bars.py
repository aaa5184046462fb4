"""The reference values behind the elementwise bars (CPU only; profiles/elementwise_accuracy.txt holds the output).

The numpy float32 oracle is run as the implementation and the float64 oracle as the reference over EXACTLY the cases of
tests/test_predict_rows.py and tests/test_gradient_elements.py (tests/_elementwise_ref.py builds both).  The worst value per
quantity times 8 is the bar of that quantity (PREDICT_BARS, GRADIENT_BARS there), capped by the ceilings the suite already had.

    python tools/elementwise_bars.py            # a few seconds
"""
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

import _elementwise_ref as E  # noqa: E402


def main():
    t0 = time.time()
    worst = {k: 0.0 for k in E.PKEYS}
    print("# posterior: float32 numpy oracle against the float64 oracle, worst row per case")
    print("# npix nh B | " + " ".join(f"{k:>9s}" for k in E.PKEYS) + " | pixels of unc left out (oracle value 0)")
    for npix, nh, B in E.PREDICT_CASES:
        p, mu, wav, nb, b, rows = E.predict_case(npix, nh, B)
        ref = E.predict_rows(p, mu, b, rows)
        f32 = E.predict_rows(p, mu, b, rows, dtype=np.float32)
        errs = E.predict_row_errors(f32, ref)
        for k in E.PKEYS:
            worst[k] = max(worst[k], float(errs[k].max()))
        print(f"{npix:5d} {nh:2d} {B:3d} | " + " ".join(f"{errs[k].max():9.2e}" for k in E.PKEYS)
              + f" | {int((ref['unc'] <= 0).sum())}")
    print("# worst  | " + " ".join(f"{worst[k]:9.2e}" for k in E.PKEYS))
    print("# x 8    | " + " ".join(f"{8 * worst[k]:9.2e}" for k in E.PKEYS))
    print()
    gw = {(k, c): 0.0 for k in E.GKEYS for c in (0, 1)}
    print("# gradients: the same pair, worst element per case in units of its sum of |terms| -- elements of two and more terms,")
    print("# then elements of ONE term (count 1: the term's own pieces cancel, nothing averages); min |sum| / sum|terms|")
    print("# npix nb nh B | " + " ".join(f"{k:>9s} {k + '(1)':>9s}" for k in E.GKEYS) + " | min condition | elements with count 0 (NaN on both sides)")
    for npix, nb_, nh, B in E.GRADIENT_CASES:
        p, mu, wav, nb, b, rows = E.gradient_case(npix, nb_, nh, B)
        ref = E.gradient_units(p, b, rows)
        f32 = E.gradient_units(p, b, rows, dtype=np.float32)
        line, cond, empty = [], np.inf, 0
        for k in E.GKEYS:
            u = E.grad_error_units(f32[k]["grad"], ref[k]["grad"], ref[k]["abssum"], ref[k]["count"])
            assert np.array_equal(f32[k]["count"], ref[k]["count"]), k
            for c in (0, 1):
                w = E.worst_element(np.where((ref[k]["count"] == 1) == bool(c), u, np.nan))[1]
                gw[k, c] = max(gw[k, c], w)
                line.append(f"{w:9.2e}")
            ok = ref[k]["count"] > 0
            empty += int((~ok).sum())
            if ok.any():
                cond = min(cond, float(np.min(np.abs(ref[k]["sum"][ok]) / ref[k]["abssum"][ok])))
        print(f"{npix:5d} {nb:3d} {nh:2d} {B:3d} | " + " ".join(line) + f" | {cond:9.2e} | {empty}")
    print("# worst        | " + " ".join(f"{gw[k, c]:9.2e}" for k in E.GKEYS for c in (0, 1)))
    print("# x 8          | " + " ".join(f"{8 * gw[k, c]:9.2e}" for k in E.GKEYS for c in (0, 1)))
    print(f"# {time.time() - t0:.0f} s")


if __name__ == "__main__":
    main()
