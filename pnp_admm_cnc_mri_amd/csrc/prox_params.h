// Scalars of the z / w update, shared by the host (api.hip) and every kernel that applies the update.  No HIP: fft16.h includes
// it, and the host emulations include fft16.h.
#pragma once

namespace pnp {

// pre-combined on the host in double and rounded once to R
template <typename R>
struct ProxParamsT {
    R thr;      // L1: reo*lambda1            CNC: alpha*reo*lambda1   (outer soft threshold)
    R c1;       // CNC: 1-alpha
    R c2;       // CNC: alpha
    R c3;       // CNC: alpha*reo*lambda1*b
    R ib;       // CNC: 1/b   (inner clip level: z - soft(z,1/b) == clip(z,-1/b,1/b))
};
using ProxParams = ProxParamsT<float>;

}  // namespace pnp
