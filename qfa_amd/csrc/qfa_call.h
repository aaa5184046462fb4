// qfa_call.h -- what the host code of every C entry point shares: the batch as the kernels take it (norm_batch), the dispatch of N_h
// onto the kernels' compile-time width (by_nhm) and the status a call returns (hip_status).
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/qfa_hip.h"

// the batch as the kernels take it: row_stride filled in
inline qfa_batch_t norm_batch(const qfa_batch_t &b, int Npix) {
    qfa_batch_t r = b;
    if (r.row_stride == 0) r.row_stride = Npix;
    return r;
}

// NHM >= Nh, the width of the latent row a kernel is compiled for: fn(std::integral_constant<int, 8 | 16 | 32>)
template <class Fn>
inline void by_nhm(int Nh, Fn &&fn) {
    if (Nh <= 8) fn(std::integral_constant<int, 8>{});
    else if (Nh <= 16) fn(std::integral_constant<int, 16>{});
    else fn(std::integral_constant<int, 32>{});
}

// launch errors of the calls just made; with QFA_F_SYNC also the asynchronous ones (the stream is drained first)
inline int hip_status(hipStream_t st = nullptr, unsigned flags = 0) {
    if (flags & QFA_F_SYNC) {
        hipError_t s = hipStreamSynchronize(st);
        if (s != hipSuccess) { (void)hipGetLastError(); return (int)s; }
    }
    return (int)hipGetLastError();
}
