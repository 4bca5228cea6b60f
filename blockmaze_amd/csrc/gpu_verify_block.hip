// Device half of the randomized block check (DESIGN.md "Block verification"): for every record i of a call and its 128-bit weight r_i
//   * the screen of verifyBatch: A, B, C on their curves (is_well_formed), and whether the record's input accumulator acc_i is the point at infinity;
//   * f_i^{r_i}, f_i = Miller(A_i, B_i) — the ate loop of libff (alt_bn128_pairing.cpp:368-418), no gamma / delta lines, no final exponentiation;
//   * r_i C_i;
// then the product of the f_i^{r_i} and the sum of the r_i C_i over the records that passed the screen. The host closes the check (groth16_verifier.cpp).
// One LANE per record, as kernel K9's first generation: the work of a record is one dependent chain (about 11,000 field products for the Miller loop, 7,000 for the
// exponentiation by a 128-bit weight in 4-bit windows) and a record never waits for another. The point work (screen, acc_i, r_i C_i: about 3,000 products) runs in
// waves of its own in the same launch, beside the pairing waves.
#include <cstring>
#include "gpu_internal.hpp"
#include "pairing_types.cuh"

namespace zk {

struct BlockConsts { Fq2 twist_b, q_x, q_y; Fq two_inv; };   // 3/(9+u); twist_mul_by_q_x / _y (alt_bn128_g2.cpp:367-372); 1/2

__device__ __forceinline__ Fq12 bk_mul(const Fq12 &x, const Fq12 &y) {                  // fp12_2over3over2.tcc:91-104
  const Fq6 aA = x.c0 * y.c0, bB = x.c1 * y.c1;
  return {aA + bB.mul_by_v(), (x.c0 + x.c1) * (y.c0 + y.c1) - aA - bB};
}
__device__ __forceinline__ Fq12 bk_sqr(const Fq12 &x) {                                 // squared_complex, fp12_2over3over2.tcc
  const Fq6 ab = x.c0 * x.c1;
  return {(x.c0 + x.c1) * (x.c0 + x.c1.mul_by_v()) - ab - ab.mul_by_v(), ab + ab};
}
// x * (la, 0, lc | 0, le, 0): mul_by_024 (fp12_2over3over2.tcc:240-335), the form of pairing.cuh's VM_MUL024
__device__ __forceinline__ Fq12 bk_mul024(const Fq12 &x, const Fq2 &la, const Fq2 &le, const Fq2 &lc) {
  const Fq2 p0 = x.c0.c0 * la, p2 = x.c0.c2 * lc, p1c = x.c0.c1 * lc, p1a = x.c0.c1 * la, pm = (x.c0.c0 + x.c0.c2) * (la + lc);
  const Fq6 t0 = {p0 + p1c.mul_xi(), p1a + p2.mul_xi(), pm - p0 - p2};
  const Fq6 t1 = {(x.c1.c2 * le).mul_xi(), x.c1.c0 * le, x.c1.c1 * le};
  const Fq6 sx = x.c0 + x.c1, sl = {la, le, lc}, t2 = sx * sl;
  return {t0 + t1.mul_by_v(), t2 - t0 - t1};
}

// flag[i]: 1 the record takes part in the equation, 0 rejected by the screen (a point off its curve or at infinity), 2 its input accumulator is the point at
// infinity (the per-proof path decides it, as verifyBatch does with kernel K9's verdict 2).  Blocks [0, pair_blocks) do the pairing work, the rest the point work.
static __global__ void __launch_bounds__(64) k_block_records(const VerifyItem *__restrict__ items, const Fr *__restrict__ inputs, uint32_t n_inputs,
    const Affine<Fq> *__restrict__ tables, Affine<Fq> ic0, const uint4 *__restrict__ weights, BlockConsts K, uint32_t n, uint32_t pair_blocks,
    Fq12 *__restrict__ f_out, XYZZ<Fq> *__restrict__ c_out, uint8_t *__restrict__ flag) {
  const bool pairing = blockIdx.x < pair_blocks;
  const uint32_t i = (pairing ? blockIdx.x : blockIdx.x - pair_blocks) * 64 + threadIdx.x; if (i >= n) return;
  const uint4 wv = weights[i]; const uint32_t wl[4] = {wv.x, wv.y, wv.z, wv.w};
  auto digit = [&](int k) { return (wl[k >> 3] >> ((k & 7) * 4)) & 15u; };              // 4-bit window k of the weight, k = 0 the lowest
  if (pairing) {
    const Affine<Fq> A = items[i].A; const Affine<Fq2> B = items[i].B;
    // miller_loop :368-418 over the bits of 6z+2 below the leading one (0x19d797039be763ba8), the G2 point homogeneous projective
    const uint64_t ATE_LO = 0x9d797039be763ba8ull;
    Fq12 f = {Fq6::one(), Fq6::zero()}; Fq2 X = B.x, Y = B.y, Z = Fq2::one();
    auto add_step = [&](const Fq2 &x2, const Fq2 &y2) {                                   // mixed_addition_step_for_flipped_miller_loop :270-293
      const Fq2 D = X - x2 * Z, E = Y - y2 * Z, F = D.sqr(), G = E.sqr(), H = D * F, I = X * F, J = H + Z * G - (I + I), Y1 = Y;
      X = D * J; Y = E * (I - J) - H * Y1; Z = Z * H;
      f = bk_mul024(f, (E * x2 - D * y2).mul_xi(), D.mul_fq(A.y), E.neg().mul_fq(A.x));
    };
#pragma unroll 1
    for (int b = 63; b >= 0; b--) {
      f = bk_sqr(f);
      { // doubling_step_for_flipped_miller_loop :242-268
        const Fq2 Av = (X * Y).mul_fq(K.two_inv), Bv = Y.sqr(), C = Z.sqr(), D = C + C + C, E = K.twist_b * D, F = E + E + E, G = (Bv + F).mul_fq(K.two_inv),
            H = (Y + Z).sqr() - (Bv + C), I = E - Bv, J = X.sqr(), E2 = E.sqr();
        X = Av * (Bv - F); Y = G.sqr() - (E2 + E2 + E2); Z = Bv * H;
        f = bk_mul024(f, I.mul_xi(), H.neg().mul_fq(A.y), (J + J + J).mul_fq(A.x));
      }
      if ((ATE_LO >> b) & 1) add_step(B.x, B.y);
    }
    // the two Frobenius corrections (mul_by_q, alt_bn128_g2.cpp:367-372)
    const Fq2 q1x = K.q_x * B.x.frob(1), q1y = K.q_y * B.y.frob(1), q2x = K.q_x * q1x.frob(1), q2y = (K.q_y * q1y.frob(1)).neg();
    add_step(q1x, q1y); add_step(q2x, q2y);
    // f^r, 4-bit windows from the top: T[d] = f^d
    Fq12 T[16]; T[0] = {Fq6::one(), Fq6::zero()}; T[1] = f;
#pragma unroll 1
    for (int d = 2; d < 16; d++) T[d] = bk_mul(T[d - 1], f);
    Fq12 acc = T[digit(31)];
#pragma unroll 1
    for (int k = 30; k >= 0; k--) { acc = bk_sqr(acc); acc = bk_sqr(acc); acc = bk_sqr(acc); acc = bk_sqr(acc); acc = bk_mul(acc, T[digit(k)]); }
    f_out[i] = acc;
    return;
  }
  const VerifyItem it = items[i];
  // is_well_formed (on-curve only) as kernel K9 tests it (pairing.cuh: k_verify_batch)
  const bool good = !it.A.is_inf() && !it.B.is_inf() && !it.C.is_inf() && it.A.y.sqr() == it.A.x.sqr() * it.A.x + Fq::from_u64(3) &&
      it.C.y.sqr() == it.C.x.sqr() * it.C.x + Fq::from_u64(3) && it.B.y.sqr() == it.B.x.sqr() * it.B.x + K.twist_b;
  // acc_i = IC[0] + sum_j inputs[i][j] IC[j+1] from the 8-bit window tables, complete additions (only whether it is the point at infinity is used)
  XYZZ<Fq> a = XYZZ<Fq>::from_affine(ic0);
#pragma unroll 1
  for (uint32_t j = 0; j < n_inputs; j++) { const Fr x = inputs[(size_t)i * n_inputs + j]; const Affine<Fq> *t = tables + (size_t)j * 32 * 255;
#pragma unroll 1
    for (int w = 0; w < 32; w++) { const uint32_t d = (x.l[w >> 2] >> ((w & 3) * 8)) & 0xffu; if (d) a.madd_inl(t[w * 255 + d - 1]); } }
  flag[i] = !good ? 0 : a.is_inf() ? 2 : 1;
  // r_i C_i, 4-bit windows from the top
  XYZZ<Fq> P[16]; P[0] = XYZZ<Fq>::inf(); P[1] = XYZZ<Fq>::from_affine(it.C);
#pragma unroll 1
  for (int d = 2; d < 16; d++) { P[d] = P[d - 1]; P[d].madd_inl(it.C); }
  XYZZ<Fq> s = P[digit(31)];
#pragma unroll 1
  for (int k = 30; k >= 0; k--) { s = s.dbl_inl(); s = s.dbl_inl(); s = s.dbl_inl(); s = s.dbl_inl(); s.add_inl(P[digit(k)]); }
  c_out[i] = s;
}

// one level of the two reductions: out[i] = in[2i] * in[2i+1] and the sum of the two points; with `flag`, a record whose flag is not 1 counts as 1 / infinity
static __global__ void __launch_bounds__(64) k_block_reduce(const Fq12 *__restrict__ f_in, const XYZZ<Fq> *__restrict__ p_in, const uint8_t *__restrict__ flag,
    uint32_t n, Fq12 *__restrict__ f_out, XYZZ<Fq> *__restrict__ p_out) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x, a = 2 * i, b = 2 * i + 1; if (a >= n) return;
  const bool ua = !flag || flag[a] == 1, ub = b < n && (!flag || flag[b] == 1); const Fq12 one = {Fq6::one(), Fq6::zero()};
  f_out[i] = bk_mul(ua ? f_in[a] : one, ub ? f_in[b] : one);
  XYZZ<Fq> p = ua ? p_in[a] : XYZZ<Fq>::inf(); if (ub) p.add_inl(p_in[b]); p_out[i] = p;
}

// the screen of a call from records: a record whose 512 characters are not a proof is rejected whatever its zeroed points are
static __global__ void __launch_bounds__(256) k_block_and_parsed(const uint8_t *__restrict__ parsed, uint32_t n, uint8_t *__restrict__ flag) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x; if (i < n && !parsed[i]) flag[i] = 0;
}

// run_resident's workspace: device arrays for `cap` records, and pinned memory for the weights on their way in and the results on their way out
struct BlockWorkspace { size_t cap = 0; DevBuf<uint8_t> w, fl, f, c, f2, c2, sums; PinnedBuf<Fe32> hw, hres; };
struct BlockVerifier::Impl { size_t n_inputs = 0; DevBuf<uint8_t> tables; Affine<Fq> ic0; BlockConsts K; BlockWorkspace ws; };

template <class T, class H> static T bk_to_dev(const H &h) { static_assert(sizeof(T) == sizeof(H), "layout"); T t; memcpy(&t, &h, sizeof(T)); return t; }

BlockVerifier::BlockVerifier(const host::HFq *ic_x, const host::HFq *ic_y, size_t n_inputs, const G1AffineRaw &ic0) : impl(new Impl) {
  Impl &d = *impl; d.n_inputs = n_inputs; const size_t nt = n_inputs * 32 * 255;
  std::vector<G1AffineRaw> tab(nt + 1);
  for (size_t k = 0; k < nt; k++) { memcpy(&tab[k].x, ic_x[k].l, 32); memcpy(&tab[k].y, ic_y[k].l, 32); }
  d.tables = DevBuf<uint8_t>(tab.size() * sizeof(G1AffineRaw)); d.tables.upload((const uint8_t *)tab.data(), tab.size() * sizeof(G1AffineRaw));
  memcpy(&d.ic0, &ic0, sizeof ic0);
  using host::HFq; using host::HFq2;
  const HFq2 tb = HFq2{HFq::from_u64(3), HFq::zero()} * HFq2{HFq::from_u64(9), HFq::one()}.inv(); const host::FrobeniusTables &ft = host::frobenius_tables();
  d.K.twist_b = bk_to_dev<Fq2>(tb); d.K.q_x = bk_to_dev<Fq2>(ft.twist_mul_by_q_x); d.K.q_y = bk_to_dev<Fq2>(ft.twist_mul_by_q_y);
  d.K.two_inv = bk_to_dev<Fq>(HFq::from_u64(2).inv());
}
BlockVerifier::~BlockVerifier() = default;
size_t BlockVerifier::num_inputs() const { return impl->n_inputs; }

void BlockVerifier::run(const void *proofs_mont, const Fe32 *inputs_canonical, const uint8_t *weights, size_t n, uint8_t *flags, host::HFq12 &prod,
    host::HG1 &sum_c) {
  if (!n || n > 0x7fffffffu) throw GpuError("block verify: record count");
  Impl &d = *impl; hipStream_t s = gpu().stream; const size_t half = (n + 1) / 2;
  DevBuf<uint8_t> items(n * sizeof(VerifyItem)), in(n * d.n_inputs * sizeof(Fe32) + 32), w(n * 16), fl(n), f(n * sizeof(Fq12)), c(n * sizeof(XYZZ<Fq>)),
      f2(half * sizeof(Fq12)), c2(half * sizeof(XYZZ<Fq>));
  items.upload((const uint8_t *)proofs_mont, n * sizeof(VerifyItem)); if (d.n_inputs) in.upload((const uint8_t *)inputs_canonical, n * d.n_inputs * sizeof(Fe32));
  w.upload(weights, n * 16);
  HIP_CHECK(hipMemsetAsync(fl.get(), 0xff, n, s));                           // (as BatchVerifier::verify: a flag that never arrives is not read as one)
  Stage st("verify.block");
  const uint32_t nb = cdiv(n, 64);
  hipLaunchKernelGGL(k_block_records, dim3(2 * nb), dim3(64), 0, s, (const VerifyItem *)items.get(), (const Fr *)in.get(), (uint32_t)d.n_inputs,
      (const Affine<Fq> *)d.tables.get(), d.ic0, (const uint4 *)w.get(), d.K, (uint32_t)n, nb, (Fq12 *)f.get(), (XYZZ<Fq> *)c.get(), fl.get());
  // a binary tree, one Fq12 product deep a level (16 levels for 65,536 records).  Ping-pong: level 1 reads the record arrays and writes the half-size ones, and
  // every later level fits either
  uint8_t *fa = f.get(), *ca = c.get(), *fb = f2.get(), *cb = c2.get(); size_t m = n; bool first = true;
  while (first || m > 1) {
    const size_t h = (m + 1) / 2;
    hipLaunchKernelGGL(k_block_reduce, dim3(cdiv(h, 64)), dim3(64), 0, s, (const Fq12 *)fa, (const XYZZ<Fq> *)ca, first ? (const uint8_t *)fl.get() : nullptr,
        (uint32_t)m, (Fq12 *)fb, (XYZZ<Fq> *)cb);
    std::swap(fa, fb); std::swap(ca, cb); m = h; first = false;
  }
  HIP_CHECK(hipGetLastError()); HIP_CHECK(hipStreamSynchronize(s));
  fl.download(flags, n);
  Fq12 pd; HIP_CHECK(hipMemcpy(&pd, fa, sizeof pd, hipMemcpyDeviceToHost)); memcpy(&prod, &pd, sizeof pd);
  XYZZ<Fq> p; HIP_CHECK(hipMemcpy(&p, ca, sizeof p, hipMemcpyDeviceToHost));
  host::HFq X, Y, ZZ, ZZZ; memcpy(X.l, p.X.l, 32); memcpy(Y.l, p.Y.l, 32); memcpy(ZZ.l, p.ZZ.l, 32); memcpy(ZZZ.l, p.ZZZ.l, 32);
  sum_c = host::HG1::from_xyzz(X, Y, ZZ, ZZZ);
  for (size_t k = 0; k < n; k++) if (flags[k] > 2) throw GpuError("block verify: a flag did not arrive");
}

void BlockVerifier::run_resident(const void *items_dev, const Fe32 *inputs_dev, const uint8_t *parsed_dev, const uint8_t *weights, size_t n, uint8_t *flags,
    host::HFq12 &prod, host::HG1 &sum_c, uint64_t *sums) {
  if (!n || n > (1u << 26)) throw GpuError("block verify: record count");
  try { run_resident_unsynced(items_dev, inputs_dev, parsed_dev, weights, n, flags, prod, sum_c, sums); }
  catch (...) { (void)hipStreamSynchronize(gpu().stream); throw; }             // (the pinned weights and results are the next caller's as soon as this one leaves)
}
void BlockVerifier::run_resident_unsynced(const void *items_dev, const Fe32 *inputs_dev, const uint8_t *parsed_dev, const uint8_t *weights, size_t n, uint8_t *flags,
    host::HFq12 &prod, host::HG1 &sum_c, uint64_t *sums) {
  Impl &d = *impl; BlockWorkspace &ws = d.ws; hipStream_t s = gpu().stream; const size_t rows = d.n_inputs + 1, sum_bytes = rows * 7 * sizeof(uint64_t);
  if (n > ws.cap) {
    const size_t cap = n + n / 4 + 64, half = (cap + 1) / 2;
    ws.w = DevBuf<uint8_t>(cap * 16); ws.fl = DevBuf<uint8_t>(cap); ws.f = DevBuf<uint8_t>(cap * sizeof(Fq12)); ws.c = DevBuf<uint8_t>(cap * sizeof(XYZZ<Fq>));
    ws.f2 = DevBuf<uint8_t>(half * sizeof(Fq12)); ws.c2 = DevBuf<uint8_t>(half * sizeof(XYZZ<Fq>));
    ws.sums = DevBuf<uint8_t>((block_scalar_sums_scratch(d.n_inputs) + rows * 7) * sizeof(uint64_t));
    ws.hw = PinnedBuf<Fe32>(cap * 16 / sizeof(Fe32) + 1); ws.hres = PinnedBuf<Fe32>((cap + sizeof(Fq12) + sizeof(XYZZ<Fq>) + sum_bytes) / sizeof(Fe32) + 4); ws.cap = cap;
  }
  memcpy(ws.hw.get(), weights, n * 16); upload_async(ws.w.get(), ws.hw.get(), n * 16);
  HIP_CHECK(hipMemsetAsync(ws.fl.get(), 0xff, n, s));
  uint8_t *fa = ws.f.get(), *ca = ws.c.get(), *fb = ws.f2.get(), *cb = ws.c2.get();
  { Stage st("verify.block");
    const uint32_t nb = cdiv(n, 64);
    hipLaunchKernelGGL(k_block_records, dim3(2 * nb), dim3(64), 0, s, (const VerifyItem *)items_dev, (const Fr *)inputs_dev, (uint32_t)d.n_inputs,
        (const Affine<Fq> *)d.tables.get(), d.ic0, (const uint4 *)ws.w.get(), d.K, (uint32_t)n, nb, (Fq12 *)ws.f.get(), (XYZZ<Fq> *)ws.c.get(), ws.fl.get());
    hipLaunchKernelGGL(k_block_and_parsed, dim3(cdiv(n, 256)), dim3(256), 0, s, parsed_dev, (uint32_t)n, ws.fl.get());
    size_t m = n; bool first = true;
    while (first || m > 1) {                                                   // the tree of run()
      const size_t h = (m + 1) / 2;
      hipLaunchKernelGGL(k_block_reduce, dim3(cdiv(h, 64)), dim3(64), 0, s, (const Fq12 *)fa, (const XYZZ<Fq> *)ca, first ? (const uint8_t *)ws.fl.get() : nullptr,
          (uint32_t)m, (Fq12 *)fb, (XYZZ<Fq> *)cb);
      std::swap(fa, fb); std::swap(ca, cb); m = h; first = false;
    } }
  uint64_t *partials = (uint64_t *)ws.sums.get(), *sums_dev = partials + block_scalar_sums_scratch(d.n_inputs);
  { Stage st("verify.sums"); block_scalar_sums_dev(inputs_dev, d.n_inputs, ws.w.get(), ws.fl.get(), n, partials, sums_dev); }   // (behind the flags)
  HIP_CHECK(hipGetLastError());
  // one pinned block for everything that comes back: the product, the sum, the integer sums (each 32-byte aligned), then the flags
  uint8_t *hr = (uint8_t *)ws.hres.get(), *h_prod = hr, *h_sum = hr + sizeof(Fq12), *h_sums = h_sum + sizeof(XYZZ<Fq>), *h_fl = h_sums + (sum_bytes + 31) / 32 * 32;
  HIP_CHECK(hipMemcpyAsync(h_prod, fa, sizeof(Fq12), hipMemcpyDeviceToHost, s)); HIP_CHECK(hipMemcpyAsync(h_sum, ca, sizeof(XYZZ<Fq>), hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(h_sums, sums_dev, sum_bytes, hipMemcpyDeviceToHost, s)); HIP_CHECK(hipMemcpyAsync(h_fl, ws.fl.get(), n, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));                                          // (a fault surfaces in the call that caused it)
  memcpy(flags, h_fl, n); memcpy(&prod, h_prod, sizeof(Fq12)); memcpy(sums, h_sums, sum_bytes);
  XYZZ<Fq> p; memcpy(&p, h_sum, sizeof p);
  host::HFq X, Y, ZZ, ZZZ; memcpy(X.l, p.X.l, 32); memcpy(Y.l, p.Y.l, 32); memcpy(ZZ.l, p.ZZ.l, 32); memcpy(ZZZ.l, p.ZZZ.l, 32);
  sum_c = host::HG1::from_xyzz(X, Y, ZZ, ZZZ);
  for (size_t k = 0; k < n; k++) if (flags[k] > 2) throw GpuError("block verify: a flag did not arrive");
}

}  // namespace zk
