"""The accuracy of the redshift finder's scan against its float64 restatement (tests/_zscan_ref.py) at the shape cases of
tests/test_zscan.py: per case the worst achieved fraction of the two bars -- |llr - llr_f64| <= 1e-5 max(|NLL_0|, |NLL_s|) per
element and |nll0 - nll0_f64| <= 5e-6 |nll0_f64| -- and over the three recovery sets the same figures with the parabola's worst
deviation in pixels and the smallest |NLL_0| per used pixel (the nll0 bar is relative: a spectrum whose NLL_0 happens to
vanish -- the low-S/N set has one at 2e-4 per pixel against terms of order 1 -- is judged against a bar of nothing).  Writes
profiles/zscan_accuracy.txt.

    python tools/zscan_accuracy.py"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def main():
    import numpy as np
    import _zscan_ref as R
    import test_zscan as Z
    lines = ["case: worst |d llr| / bar, worst |d nll0| / bar   (bars: 1e-5 max(|NLL_0|, |NLL_s|); 5e-6 |NLL_0|)"]
    worst = [0.0, 0.0]

    def fractions(scan, rl, r0, rn):
        llr, nll0 = scan.llr.cpu().numpy().astype(np.float64), scan.nll0.cpu().numpy().astype(np.float64)
        a = float(np.max(np.abs(llr - rl) / (R.BAR * np.maximum(np.abs(r0)[:, None], np.abs(rn)))))
        b = float(np.max(np.abs(nll0 - r0) / (R.NLL_BAR * np.abs(r0))))
        worst[0], worst[1] = max(worst[0], a), max(worst[1], b)
        return a, b

    for case in Z.CASES:
        nh, npix, m, rule, B, tau = case
        nb = Z.nb_of(rule, npix, m)
        params, mu, wav, _ = R.model(npix, nb, nh, seed=npix + nh)
        t = np.random.default_rng(m + nh).integers(-m, m + 1, size=B)
        d = R.draw(params, mu, wav, B, 7 * npix + nh + m, t, zq=(4.8, 5.0) if rule == "npix" else (2.2, 3.4), tau_which=tau)
        ref = R.scan(params, mu, d["flux"], d["error"], d["mask"], d["zqso"], wav, m, tau)
        a, b = fractions(Z.gpu_scan(Z.make_model(params, mu, nb, tau), d, wav, m), *ref)
        lines.append("nh%d_px%d_m%d_nb%s_B%d_%s: %.4f %.4f" % (case + (a, b)))
    for i in range(len(R.RECOVERY)):
        c = R.recovery_case(i)
        scan = Z.gpu_scan(Z.make_model(c["params"], c["mu"], c["nb"]), c, c["wav"], c["m"])
        a, b = fractions(scan, c["llr"], c["nll0"], c["nll"])
        off, sig = R.parabola(c["llr"], c["shift"])
        inner = np.abs(c["shift"]) < c["m"]
        lines.append("recovery px%d_nh%d_m%d_B%d: %.4f %.4f; best_s == injected on %d of %d; max |d off| %.2e, max |d sig| %.2e pixels; min |NLL_0| / n %.5f"
                     % (len(c["wav"]), c["nh"], c["m"], len(c["shift"]), a, b, int(np.sum(scan.best_s.cpu().numpy() == c["shift"])),
                        len(c["shift"]), float(np.max(np.abs(scan.offset.cpu().numpy() - off)[inner])),
                        float(np.max(np.abs(scan.sigma_pix.cpu().numpy() - sig)[inner])),
                        float(np.min(np.abs(c["nll0"]) / c["mask"][:, c["m"]:len(c["wav"]) - c["m"]].sum(axis=1)))))
    lines.append("worst over all cases: llr %.4f of its bar, nll0 %.4f of its bar" % tuple(worst))
    os.makedirs(os.path.join(REPO, "profiles"), exist_ok=True)
    with open(os.path.join(REPO, "profiles", "zscan_accuracy.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
