// The tower Fq6 = Fq2[v]/(v^3-(9+u)), Fq12 = Fq6[w]/(w^2-v) on the device (fp6_3over2.tcc, fp12_2over3over2.tcc) and the proof record: the types that kernel
// K9 (pairing.cuh) and the block check (gpu_verify_block.hip) share.
#pragma once
#include <hip/hip_runtime.h>
#include "curve.cuh"

namespace zk {

struct Fq6 {
  Fq2 c0, c1, c2;
  static __device__ __forceinline__ Fq6 zero() { return {Fq2::zero(), Fq2::zero(), Fq2::zero()}; }
  static __device__ __forceinline__ Fq6 one() { return {Fq2::one(), Fq2::zero(), Fq2::zero()}; }
  friend __device__ __forceinline__ Fq6 operator+(const Fq6 &a, const Fq6 &b) { return {a.c0 + b.c0, a.c1 + b.c1, a.c2 + b.c2}; }
  friend __device__ __forceinline__ Fq6 operator-(const Fq6 &a, const Fq6 &b) { return {a.c0 - b.c0, a.c1 - b.c1, a.c2 - b.c2}; }
  __device__ __forceinline__ Fq6 neg() const { return {c0.neg(), c1.neg(), c2.neg()}; }
  friend __device__ __forceinline__ Fq6 operator*(const Fq6 &a, const Fq6 &b) {   // Karatsuba, fp6_3over2.tcc:94-108
    Fq2 aA = a.c0 * b.c0, bB = a.c1 * b.c1, cC = a.c2 * b.c2;
    return {aA + ((a.c1 + a.c2) * (b.c1 + b.c2) - bB - cC).mul_xi(), (a.c0 + a.c1) * (b.c0 + b.c1) - aA - bB + cC.mul_xi(),
        (a.c0 + a.c2) * (b.c0 + b.c2) - aA + bB - cC};
  }
  __device__ __forceinline__ Fq6 mul_by_v() const { return {c2.mul_xi(), c0, c1}; }
  __device__ __forceinline__ bool operator==(const Fq6 &o) const { return c0 == o.c0 && c1 == o.c1 && c2 == o.c2; }
};
struct Fq12 { Fq6 c0, c1; __device__ __forceinline__ bool operator==(const Fq12 &o) const { return c0 == o.c0 && c1 == o.c1; } };

// Montgomery form, as parsed from the 512 hex characters
struct VerifyItem { Affine<Fq> A; Affine<Fq2> B; Affine<Fq> C; };

}  // namespace zk
