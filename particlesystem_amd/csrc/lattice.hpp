// lattice.hpp -- the cloud-in-cell weights of include/psamd.h ("mass on a lattice"), shared by deposit.hip, which spreads a
// body over the voxels around it, and sample.hip, which reads a caller's lattice back at a point with the same weights
// (device-inline only).  The lattice itself (DepLattice, kernels.h) comes from the host's deposit_lattice (services.hip).
#pragma once

#include "kernels_common.hpp"

namespace psamd {

__device__ __forceinline__ bool dep_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// one axis of one body: u = RN(RN(s inv_h) + off) clamped to [0, M - 1]; n0 = floor, f = u - n0 (exact); the weights
// RN(1 - f) for voxel n0 and f for n0 + 1
struct DepAxis {
    int n0;
    float w0, w1;
    __device__ __forceinline__ DepAxis(float s, const DepLattice &a)
    {
        const float u = __fadd_rn(__fmul_rn(s, a.inv_h), a.off);
        const float uc = fminf(fmaxf(u, 0.f), a.top), fl = floorf(uc);
        n0 = (int)fl; w1 = __fsub_rn(uc, fl); w0 = __fsub_rn(1.f, w1);
    }
    // the weight the body gives voxel n of this axis (n0 + 1 == M is no voxel: never asked for)
    __device__ __forceinline__ float at(int n) const { return n == n0 ? w0 : n == n0 + 1 ? w1 : 0.f; }
};

}  // namespace psamd
