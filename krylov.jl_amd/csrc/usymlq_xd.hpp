// usymlq_xd.hpp -- the x / d̅ update that usymlq! (usymlq.cpp) and the primal side of trilqr! (trilqr.cpp) share: one expression,
// one place, so that the two solvers' LQ iterates cannot drift apart.
#pragma once

#include <hip/hip_runtime.h>

namespace khip {

// x and d̅ of one element from iteration 2 on (src/usymlq.jl:285-290, src/trilqr.jl:289-294):
// kaxpy!(ζₖ₋₁cₖ, d̅, x) ; kaxpy!(ζₖ₋₁sₖ, uₖ, x) ; kaxpby!(-cₖ, uₖ, sₖ, d̅)
__device__ __forceinline__ void usymlq_xd(double u, double &x, double &d, double zc, double zs, double nc, double sn) {
  x = fma(zs, u, fma(zc, d, x));
  d = fma(nc, u, sn * d);
}

}  // namespace khip
