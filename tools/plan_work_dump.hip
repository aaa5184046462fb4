// plan_work_dump.hip -- prints plan_work (qfa_amd/csrc/qfa_host.h) over a grid of arguments: the values that
// tests/golden/plan_work_values.npz pins the Python port of tests/_elementwise_ref.py to.  Host code only; no device is touched.
//   hipcc -O1 -std=c++17 --offload-arch=gfx950 -I qfa_amd/csrc tools/plan_work_dump.hip -o plan_work_dump
// (python tests/test_s12_walk_edges_cpu.py builds it, runs it and records the fixture).
// One line per call: B ntiles pro slots spb max_chain | full rem nseg seg_tiles
#include <cstdio>

#include "qfa_host.h"

int main() {
    const int Bs[] = {1, 15, 17, 63, 64, 65, 129, 199, 513, 2049, 4097, 16385, 20000, 100000};
    const int tiles[] = {1, 2, 3, 4, 5, 7, 10, 13, 19, 25, 32, 33, 64, 65, 66, 97, 125, 161, 250};
    const int ncus[] = {64, 256, 304};
    // (pro, resident workgroups per compute unit, spectra per block, max_chain): the calls of make_layout_t
    const int forms[][4] = {{4, 1, 64, 0}, {4, 2, 64, 0}, {3, 1, 64, 0}, {1, 2, 64, 0}, {1, 1, 64, QFA_P1_MAX_CHAIN}, {1, 2, 128, 0}};
    for (int ncu : ncus)
        for (const auto &f : forms)
            for (int B : Bs)
                for (int nt : tiles) {
                    const WorkPlan w = plan_work(B, nt, f[0], ncu * f[1], f[2], f[3]);
                    std::printf("%d %d %d %d %d %d %d %d %d %d\n", B, nt, f[0], ncu * f[1], f[2], f[3], w.full, w.rem, w.nseg, w.seg_tiles);
                }
    return 0;
}
