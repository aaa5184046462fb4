// qfa_estep.h -- what the host code of a call on a batch shares between translation units: the argument block of the call (BatchCall),
// the dispatch of its input form to compile-time constants (by_form), and the hand-over between the step's translation units
// (qfa_capi.hip, qfa_k32.hip: images, pass 1, solve) and the EM update of F (qfa_em.hip), which runs them as its E-step.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "qfa_call.h"

// One call on a batch, as every level of the host code passes it on.  The C entry point fills it once, behind its argument checks.
struct BatchCall {
    qfa_params_t p;
    qfa_batch_t b;               // normalised (norm_batch)
    qfa_tau_t tau;
    int B, Npix, Nb, Nh;
    float *ws;                   // qfa_workspace_bytes(B, Npix, Nh)
    hipStream_t st;
    unsigned flags;              // QFA_F_*
};

// The input form of a call as compile-time constants: a host-supplied A_blue | the factored z (zq1 x pix_ratio) | zabs; rows taken
// through the resident index (never with A_blue: check_batch); exact gradients.  by_form is the one place that turns the run-time
// form into these; a kernel's callable names the axes its template has and ignores the others, so no instantiation is added.
template <bool HASA, bool ZF, bool IDX, bool EXACT>
struct Form {
    static constexpr bool hasa = HASA, zf = ZF, idx = IDX, exact = EXACT;
};
template <class Fn>
inline void by_form(const qfa_batch_t &b, bool zfac, bool exact, Fn &&fn) {
    using T = std::true_type;
    using F = std::false_type;
    auto ex = [&](auto a, auto z, auto i) {
        if (exact) fn(Form<decltype(a)::value, decltype(z)::value, decltype(i)::value, true>{});
        else fn(Form<decltype(a)::value, decltype(z)::value, decltype(i)::value, false>{});
    };
    auto ix = [&](auto z) {
        if (b.rows) ex(F{}, z, T{});
        else ex(F{}, z, F{});
    };
    if (b.A_blue) ex(T{}, F{}, F{});
    else if (zfac) ix(T{});
    else ix(F{});
}

struct QfaEStep {
    const float *SOL;            // the solve's records, `nsol` floats per spectrum: y at 0, C^-1 pairs (row-major upper triangle of
    int nsol, KP, sol_ci;        // KP, off-diagonals doubled) at sol_ci
    const float4 *ZS, *ZP;       // factored-z input form: the per-spectrum / per-pixel factor tables of this call, else NULL
    float *nll;                  // (B,) per-spectrum NLL: the caller's array, or a row of the workspace
};

// argument checks of the step's entry points (QFA_E_*; no device work)
int qfa_estep_check(const qfa_params_t *p, const qfa_batch_t *b, const qfa_tau_t *tau, int B, int Npix, int Nb, int Nh);
// images + pass 1 + solve of the training step in its exact-gradient flavour on the call's stream
int qfa_estep(const BatchCall &c, float *nll, QfaEStep *out);
int qfa_k32_estep(const BatchCall &c, float *nll, QfaEStep *out);
