// qfa_gt.hip -- the pixel-resident form of pass 2 (qfa_grads_t.h) in its own translation unit: its register budget (72
// image + 64 accumulator registers per wave, two waves per SIMD) wants its own scheduler settings (Makefile, GTFLAGS).
#include "qfa_grads_t.h"

#include "qfa_host.h"

// ---- pass 2, pixel-resident form (qfa_grads_t.h)
size_t qfa_gt_state_bytes(int KP, int B) {
    return by_kp<16>(KP, [&](auto kp) { return (size_t)((B + 15) / 16) * GTT<decltype(kp)::value>::STATE_B; });
}
// tiles, pixel blocks of 8 tiles, ranges of spectra groups: about one workgroup per CU; a multiple of 8 ranges (the
// workgroups of a range then share an XCD, block = pb R + r) where the batch has the groups for it
// (even_ranges = false: the plan before the range length is made even -- at least as many ranges and work items as any launch has)
static GtPlan gt_plan(int KP, int B, int Npix, int max_ranges, bool even_ranges = true) {
    GtPlan g;
    g.nxcd = xcd_count();
    const int pxw = by_kp<16>(KP, [](auto kp) { return (int)GTT<decltype(kp)::value>::PXW; });       // pixels per wave
    g.T16 = (Npix + pxw - 1) / pxw;
    g.PB = (g.T16 + 7) / 8;
    const int G = (B + 15) / 16, ncu = cu_count();
    // ranges: the workgroups run one per CU in rounds, so R is chosen for full rounds -- the smallest R whose
    // rounds(PB R) / R (time per unit of work) is within 3 % of the best; then a multiple of 8 if that costs nothing
    int R = 1;
    {
        const int rmax = std::max(1, std::min(4 * ncu / std::max(1, g.PB) + 1, std::max(1, G / 2)));
        auto cost = [&](int r) { return (double)((g.PB * r + ncu - 1) / ncu) / r; };
        double best = cost(1);
        for (int r = 2; r <= rmax; ++r) best = std::min(best, cost(r));
        for (int r = 1; r <= rmax; ++r)
            if (cost(r) <= 1.03 * best) { R = r; break; }
        const int X = g.nxcd;
        if (R >= X && R % X != 0 && (R + X - 1) / X * X <= rmax && cost((R + X - 1) / X * X) <= cost(R)) R = (R + X - 1) / X * X;
    }
    R = std::max(1, std::min(R, max_ranges));
    g.gpr = (G + R - 1) / R;
    // even where stage 3 contracts pairs of groups: a range starts at an even group, so no pair straddles two ranges
    if (even_ranges && by_kp<16>(KP, [](auto kp) { return (bool)GTT<decltype(kp)::value>::PAIR; })) g.gpr = (g.gpr + 1) & ~1;
    g.R = (G + g.gpr - 1) / g.gpr;
    return g;
}
int qfa_gt_items(int KP, int B, int Npix, int max_ranges) { return gt_plan(KP, B, Npix, max_ranges).items(); }
int qfa_gt_ranges(int KP, int B, int Npix, int max_ranges) { return gt_plan(KP, B, Npix, max_ranges).R; }
// what the workspace is sized for: no launch has more ranges or items (an even range length only merges ranges)
int qfa_gt_range_groups(int KP, int B, int Npix, int max_ranges) { return gt_plan(KP, B, Npix, max_ranges).gpr; }
int qfa_gt_items_bound(int KP, int B, int Npix) { return gt_plan(KP, B, Npix, 1 << 30, false).items(); }
int qfa_gt_ranges_bound(int KP, int B, int Npix) { return gt_plan(KP, B, Npix, 1 << 30, false).R; }
void qfa_gt_launch(int KP, const Pass2Call &a, int max_ranges, const unsigned char *PGT, const unsigned char *PST) {
    const GtPlan g = gt_plan(KP, a.B, a.Npix, max_ranges);        // (g.R rows leave: qfa_gt_ranges)
    by_kp<16>(KP, [&](auto kp) {
        by_form(a.b, a.ZS != nullptr, a.exact != 0, [&](auto f) {
            using Fm = decltype(f);
            k_grads_t<decltype(kp)::value, Fm::hasa, Fm::zf, Fm::idx, Fm::exact><<<g.items(), 512, 0, a.st>>>(
                a.p, a.b, a.tau, a.B, a.Npix, a.Nb, a.Nh, g, PGT, PST, a.ZS, a.accum, a.rows, a.rowsS, a.row_stride, a.sc64);
        });
    });
}

#if QFA_GT_STAMPS
extern "C" int qfa_gt_debug_stamps(unsigned long long *out) {      // diagnostic build only
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(qfa_gt_stamps), 32 * sizeof(unsigned long long));
}
#endif
