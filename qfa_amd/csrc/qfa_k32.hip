// qfa_k32.hip -- the N_h = 17..32 instantiations of the step kernels (see qfa_host.h for why they live
// in their own translation unit).
#include "qfa_host.h"

int qfa_k32_nll_grad(const BatchCall &c, float *nll, float *accum, void *const *events, void *slab) {
    return run_nll_grad<32>(c, nll, accum, events, slab);
}

int qfa_k32_estep(const BatchCall &c, float *nll, QfaEStep *out) { return run_estep<32>(c, nll, out); }

int qfa_k32_predict(const BatchCall &c, const float *mu, float *ll, float *hmean, float *hcov, float *cont, float *unc, void *const *events) {
    return run_predict<32>(c, mu, ll, hmean, hcov, cont, unc, events);
}
