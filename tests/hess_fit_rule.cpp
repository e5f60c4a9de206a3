// Host-only view of the launch-geometry rule of the look-ahead Hessenberg reduction (csrc/psd_hess2.h: psd_h2_fit_chain,
// psd_h2_fit_panel) for tests/test_hess_fit_rule.py, which compiles this file and checks the printed geometry of every
// launch of a reduction against the kernels' own indexing.
//   hess_fit_rule chain n p CR GS fused   one line "q NK nC nT nB" per chain position q = -1 .. (n - 1) p + 1
//   hess_fit_rule panel n p K CPG         one line "idx0 NK nC nT nB" per batch of K links, the drain position included
#define PSD_HOSTSIM 1
#include "psd_hess2.h"

int main(int argc, char** argv) {
    if (argc < 6) return 2;
    const int n = atoi(argv[2]), p = atoi(argv[3]), Q = (n - 1) * p;
    if (strcmp(argv[1], "chain") == 0 && argc == 7) {
        const int CR = atoi(argv[4]), GS = atoi(argv[5]), fused = atoi(argv[6]);
        for (int q = -1; q <= Q + 1; ++q) {
            const psd_h2_geom g = psd_h2_fit_chain(n, p, q, CR, GS, fused != 0);
            printf("%d %d %d %d %d\n", q, g.NK, g.nC, g.nT, g.nB);
        }
        return 0;
    }
    if (strcmp(argv[1], "panel") == 0) {
        const int K = atoi(argv[4]), CPG = atoi(argv[5]);
        for (int idx0 = 0; idx0 <= Q; idx0 += K) {
            psd_h2_geom g{0, 0, 0, 0};
            psd_h2_fit_panel(n, p, idx0, K, CPG, g);
            printf("%d %d %d %d %d\n", idx0, g.NK, g.nC, g.nT, g.nB);
        }
        return 0;
    }
    return 2;
}
