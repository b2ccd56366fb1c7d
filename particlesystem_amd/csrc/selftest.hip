// selftest.hip -- the kernels that check pair_math.hpp's short forms against the compiler's over whole float ranges
#include "pair_math.hpp"

namespace psamd {

// ------------------------------------------------------------------ self test
// Compare the hand-written sqrt / reciprocal with the compiler's correctly rounded forms
// on every float whose bit pattern lies in [lo_bits, hi_bits].  out[0..3] = mismatch
// counts of sqrt_rn_short, rcp_rn_newton, their composition (what the pair kernel uses)
// and of the rejected one-transcendental shortcut; out[4] = mismatches of inv_sqrt_guarded that it
// did not report, out[5] = inputs it reported; out[8..15] / out[16..23] = first
// offending inputs of sqrt / composition; out[24], out[25] = cursors.
__global__ void k_selftest_math(uint32_t lo_bits, uint32_t hi_bits, unsigned long long *out)
{
    const uint64_t span = (uint64_t)hi_bits - lo_bits + 1;
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    unsigned long long bad[6] = {0, 0, 0, 0, 0, 0};
    for (; i < span; i += stride) {
        const float a = __uint_as_float(lo_bits + (uint32_t)i);
        const float s_ref = sqrtf(a), r_ref = 1.0f / a, c_ref = 1.0f / s_ref;
        if (__float_as_uint(sqrt_rn_short(a)) != __float_as_uint(s_ref)) {
            bad[0]++;
            const unsigned long long k = atomicAdd(&out[25], 1ull);
            if (k < 8) out[8 + k] = __float_as_uint(a);
        }
        if (__float_as_uint(rcp_rn_newton(a)) != __float_as_uint(r_ref)) bad[1]++;
        if (__float_as_uint(inv_sqrt_selected(a)) != __float_as_uint(c_ref)) {
            bad[2]++;
            const unsigned long long k = atomicAdd(&out[24], 1ull);
            if (k < 8) out[16 + k] = __float_as_uint(a);
        }
        if (__float_as_uint(inv_sqrt_one_transcendental(a)) != __float_as_uint(c_ref)) bad[3]++;
        bool tie = false;
        const float gq = inv_sqrt_guarded(a, tie);
        if (tie) bad[5]++;
        else if (__float_as_uint(gq) != __float_as_uint(c_ref)) bad[4]++;
    }
    for (int k = 0; k < 6; k++) if (bad[k]) atomicAdd(&out[k], bad[k]);
}

// out[0] += number of floats x with bits in [lo_bits, hi_bits] for which the fp32 add of
// eps2f differs from the reference's double add rounded to float
__global__ void k_validate_eps(uint32_t lo_bits, uint32_t hi_bits, double eps2, float eps2f, unsigned long long *out)
{
    const uint64_t span = (uint64_t)hi_bits - lo_bits + 1;
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    unsigned long long bad = 0;
    for (; i < span; i += stride) {
        const float x = __uint_as_float(lo_bits + (uint32_t)i);
        if (__float_as_uint(x + eps2f) != __float_as_uint((float)((double)x + eps2))) bad++;
    }
    if (bad) atomicAdd(out, bad);
}

hipError_t launch_validate_eps(hipStream_t st, uint32_t lo_bits, uint32_t hi_bits, double eps2, float eps2f,
                               unsigned long long *out)
{
    k_validate_eps<<<2048, 256, 0, st>>>(lo_bits, hi_bits, eps2, eps2f, out);
    return hipGetLastError();
}

hipError_t launch_selftest_math(hipStream_t st, uint32_t lo_bits, uint32_t hi_bits, unsigned long long *out24)
{
    k_selftest_math<<<4096, 256, 0, st>>>(lo_bits, hi_bits, out24);
    return hipGetLastError();
}

}  // namespace psamd
