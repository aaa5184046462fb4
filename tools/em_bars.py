"""The reference values behind the bars of the EM statistics' element judge (CPU only; profiles/em_accuracy.txt holds the output).

The float32 numpy restatement ``em_terms(dtype=np.float32)`` is run as the implementation and the float64 one as the reference
over EXACTLY the cases of tests/test_em_elements.py (tests/_em_ref.py: ELEMENT_CASES).  Per case: the worst element of S2 and of
S1 in units of its own sum of |terms| (``stat_units``) over the pixels that two and more spectra see, then over the pixels that
ONE spectrum sees (a term's own pieces cancel, nothing averages: STAT_BARS explains), and where each sits.  The worst value per
quantity and class times 8 is its bar (STAT_BARS there).

    python tools/em_bars.py            # about two minutes: the four cases past the fold hold 4101 x 4040 elements each
"""
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

import _em_ref as E  # noqa: E402


def main():
    t0 = time.time()
    worst = {(k, c): 0.0 for k in ("S2", "S1") for c in (0, 1)}
    print("# statistics: float32 numpy restatement against the float64 one, worst element per case in units of its sum of |terms|:")
    print("# pixels with cnt >= 2, then pixels with cnt = 1 (-: the case has none)")
    print("# kind   npix nh    B form     |        S2    (pixel, a, b)     S2(1)    (pixel, a, b) |        S1      (pixel, a)"
          "     S1(1)      (pixel, a) | pixels with cnt 0, 1")
    for case in E.ELEMENT_CASES:
        kind, npix, nh, B, form, seed = case
        ref, f32 = E.case_terms(case), E.case_terms(case, np.float32)
        if kind == "accum":                              # the float64 sum of both batches, the float32 sum of the float32 ones
            ref = {k: ref[0][k] + ref[1][k] for k in ("S2", "S1", "absS2", "absS1", "cnt")}
            f32 = {k: f32[0][k] + f32[1][k] for k in ("S2", "S1", "cnt")}
        assert np.array_equal(f32["cnt"], ref["cnt"])
        line = []
        for k in ("S2", "S1"):
            part = []
            for c, (w, idx) in enumerate(E.class_worst(E.stat_units(f32[k], ref[k], ref["abs" + k]), ref["cnt"])):
                worst[k, c] = max(worst[k, c], w)
                part.append(f"{w:9.2e} {str(idx):>16s}" if idx else f"{'-':>9s} {'':16s}")
            line.append(" ".join(part))
        print(f"{kind:6s} {npix:5d} {nh:2d} {B:4d} {form:8s} | " + " | ".join(line)
              + f" | {int((ref['cnt'] == 0).sum())}, {int((ref['cnt'] == 1).sum())}", flush=True)
    print("# worst  | " + " ".join(f"{k}{'(1)' if c else ''} {worst[k, c]:9.2e}" for k, c in worst))
    print("# x 8    | " + " ".join(f"{k}{'(1)' if c else ''} {8 * worst[k, c]:9.2e}" for k, c in worst))
    print(f"# {time.time() - t0:.0f} s", file=sys.stderr)


if __name__ == "__main__":
    main()
