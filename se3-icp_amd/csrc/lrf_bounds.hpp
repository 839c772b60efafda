// lrf_bounds.hpp — the f32 bounds of k_lrf8.hip's lists and the certificate of a taken list
// (DESIGN sections 17 and 21), written for the device and the host alike: tests/take_host.cpp
// checks them against long double evaluation.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace se3icp {
namespace knn {

constexpr unsigned kIdBits = 0xfffu;     // low bits of a list entry: the candidate id
// bound of the accept-all phase: every finite key (a lane past the leaf's end carries an
// infinite distance, so its entry is above every bound)
constexpr unsigned kAll = 0x7f7fffffu;

__host__ __device__ __forceinline__ float bits_f32(unsigned u) { return __builtin_bit_cast(float, u); }
__host__ __device__ __forceinline__ unsigned f32_bits(float f) { return __builtin_bit_cast(unsigned, f); }

// |f32 squared distance of the f32-rounded points - exact squared distance of the f64
// points| for distances <= d (loopdev.hpp f32_err, D = 3); S bounds the sum of the norms
__host__ __device__ __forceinline__ float f32_err3(float d, float S) {
    const float u = 5.9604645e-08f;
    return 1.25f * (2.f * u * S * sqrtf(fmaxf(d, 0.f)) + 6.f * u * d + 4.f * u * u * S * S) + 1e-30f;
}
// the list bound from the Kw-th smallest entry t (f32 keys): every point whose exact
// distance is within the Kw-th smallest exact distance has an f32 key <= the value of t
// plus two errors
__host__ __device__ __forceinline__ unsigned widen_bound(unsigned t, float S) {
    if (t >= 0x7f800000u) return kAll;
    const float b = bits_f32(t);
    const unsigned w = (f32_bits(fmaf(2.02f, f32_err3(b, S), b)) + 2u) | kIdBits;
    return w < kAll ? w : kAll;
}
// The other direction: a list collected under the bound t holds every
// point whose f32 scan key is <= the value of t, so a point outside it has a scan key above it
// and, were its exact distance within narrow_bound(t), its scan key would be within one error
// of that, at or below t.  Hence every point outside the list has an exact squared distance
// above narrow_bound(t): a lower bound, rounded down, never negative.  A list under kAll holds
// its whole cloud.
__host__ __device__ __forceinline__ float narrow_bound(unsigned t, float S) {
    if (t >= kAll) return bits_f32(kAll);
    const float b = bits_f32(t);
    const float x = fmaf(-1.01f, f32_err3(b, S), b);
    if (!(x > 0.f)) return 0.f;
    const unsigned xb = f32_bits(x);
    return xb > 2u ? bits_f32(xb - 2u) : 0.f;
}
// the f32 key of the first rank a list does not hand on, as a lower bound of every f64 key
// that rounds to it or to a larger f32: times (1 - 2^-23), at least one ulp down
__host__ __device__ __forceinline__ float key_floor(float key) { return key * 0.99999988079071044921875f; }

// Certificate of a taken list.  lb: a lower bound, in the storing class's coordinates, of the
// computed f64 squared distance (nanoflann's arithmetic) from the query to every point that is
// not in the list; rho2 = fl(fl(s_b / s_a)^2) for the taking class b; nb >= |q| + |p| over class
// b.  Returns a bound that every such point's computed f64 squared distance in class b exceeds
// or equals, with the paddings of DESIGN section 21: a list whose farthest key is strictly below
// it holds the nearest points of class b.
__host__ __device__ __forceinline__ double take_bound(double rho2, float lb, float nb) {
    double x = sqrt(rho2 * (double)lb) - 0x1p-48 * (double)nb;
    x = x > 0.0 ? x : 0.0;
    return (1.0 - 0x1p-40) * (x * x);
}

}  // namespace knn
}  // namespace se3icp
