// qfa_estep.h -- the hand-over between the step's translation units (qfa_capi.hip, qfa_k32.hip: images, pass 1, solve) and the
// EM update of F (qfa_em.hip), which runs them as its E-step.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/qfa_hip.h"

struct QfaEStep {
    const float *SOL;            // the solve's records, `nsol` floats per spectrum: y at 0, C^-1 pairs (row-major upper triangle of
    int nsol, KP, sol_ci;        // KP, off-diagonals doubled) at sol_ci
    const float4 *ZS, *ZP;       // factored-z input form: the per-spectrum / per-pixel factor tables of this call, else NULL
    float *nll;                  // (B,) per-spectrum NLL: the caller's array, or a row of the workspace
    qfa_batch_t batch;           // the batch as the kernels take it (row_stride filled in)
};

// argument checks of the step's entry points (QFA_E_*; no device work)
int qfa_estep_check(const qfa_params_t *p, const qfa_batch_t *b, const qfa_tau_t *tau, int B, int Npix, int Nb, int Nh);
// images + pass 1 + solve of the training step in its exact-gradient flavour on `stream`; ws = qfa_workspace_bytes(B, Npix, Nh)
int qfa_estep(const qfa_params_t &p, const qfa_batch_t &b, const qfa_tau_t &tau, int B, int Npix, int Nb, int Nh, float *nll,
              float *ws, hipStream_t st, QfaEStep *out);
int qfa_k32_estep(const qfa_params_t &p, const qfa_batch_t &b, const qfa_tau_t &tau, int B, int Npix, int Nb, int Nh, float *nll,
                  float *ws, hipStream_t st, QfaEStep *out);
