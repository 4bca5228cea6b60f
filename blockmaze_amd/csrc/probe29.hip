// Raw-limb probes of the arithmetic on nine 29-bit limbs (field29_gfx950.inc: Fq29 / Fr29) and of the point formulas built on it (msm.cuh, htail29.cuh,
// oct29.cuh): zkgpu_test_field29_op / zkgpu_test_point29_op in include/zkgpu.h.  Nothing is converted or normalized on the way in or out: an element is its nine
// limbs, so a test can hand the device operands at the edge of a contract and see exactly the limbs that come back (tests/test_gpu_field29.py).
// One __global__ per operation, as in probe.hip.
#include <hip/hip_runtime.h>
#include "gpu.hpp"
#include "msm.cuh"

namespace zk {
extern hipStream_t gpu_stream();
#define HIP_CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) throw GpuError(std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)

template <class F> __device__ __forceinline__ F ld29(const uint32_t *p) { F r;
#pragma unroll
  for (int i = 0; i < 9; i++) r.l[i] = p[i];
  return r; }
template <class F> __device__ __forceinline__ void st29(uint32_t *p, const F &v) {
#pragma unroll
  for (int i = 0; i < 9; i++) p[i] = v.l[i]; }
__device__ __forceinline__ void st8(uint32_t *p, const uint32_t (&w)[8]) {
#pragma unroll
  for (int i = 0; i < 8; i++) p[i] = w[i];
  p[8] = 0; }

// ---- field operations: operands a, b, c, d of nine words an element; FIELD29_OUT_WORDS[op] words an element out -----------------------------------------------
enum { F29_MUL, F29_MUL2, F29_SQR, F29_NORM, F29_SUB2, F29_SUB4, F29_SUB6, F29_SUB12, F29_SUB18, F29_COND_NEG, F29_SUB_PRODUCT, F29_NEG_PRODUCT, F29_ADD_RAW,
       F29_BARRETT, F29_ONE, F29_UNPACK, F29_PACK_WORDS, F29_TO_WORDS, F29_PRODUCT_IS_ZERO, F29_NTT_LAZY, F29_OPS };
static constexpr int F29_NTT_OUT = 45;
static int field29_out_words(int op) { return op == F29_NTT_LAZY ? F29_NTT_OUT : 9; }

template <class F, int OP> __global__ void __launch_bounds__(256) k_probe_f29(const uint32_t *a, const uint32_t *b, const uint32_t *c, const uint32_t *d,
    uint32_t *out, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; if (i >= n) return;
  const size_t e = (size_t)i * 9; uint32_t *o = out + (size_t)i * (OP == F29_NTT_LAZY ? F29_NTT_OUT : 9);
  if constexpr (OP == F29_MUL) st29(o, F::mul(ld29<F>(a + e), ld29<F>(b + e)));
  else if constexpr (OP == F29_MUL2) st29(o, F::mul2(ld29<F>(a + e), ld29<F>(b + e), ld29<F>(c + e), ld29<F>(d + e)));
  else if constexpr (OP == F29_SQR) st29(o, F::sqr(ld29<F>(a + e)));
  else if constexpr (OP == F29_NORM) st29(o, ld29<F>(a + e).norm());
  else if constexpr (OP == F29_SUB2) st29(o, F::template sub<2>(ld29<F>(a + e), ld29<F>(b + e)));
  else if constexpr (OP == F29_SUB4) st29(o, F::template sub<4>(ld29<F>(a + e), ld29<F>(b + e)));
  else if constexpr (OP == F29_SUB6) st29(o, F::template sub<6>(ld29<F>(a + e), ld29<F>(b + e)));
  else if constexpr (OP == F29_SUB12) st29(o, F::template sub<12>(ld29<F>(a + e), ld29<F>(b + e)));
  else if constexpr (OP == F29_SUB18) st29(o, F::template sub<18>(ld29<F>(a + e), ld29<F>(b + e)));
  else if constexpr (OP == F29_COND_NEG) st29(o, F::cond_neg(ld29<F>(a + e), (b[e] & 1u) != 0));          // the sense: bit 0 of b's first word
  else if constexpr (OP == F29_SUB_PRODUCT) st29(o, F::sub_product(ld29<F>(a + e), ld29<F>(b + e)));
  else if constexpr (OP == F29_NEG_PRODUCT) st29(o, F::neg_product(ld29<F>(a + e)));
  else if constexpr (OP == F29_ADD_RAW) st29(o, F::add_raw(ld29<F>(a + e), ld29<F>(b + e)));
  else if constexpr (OP == F29_BARRETT) st29(o, ld29<F>(a + e).barrett());
  else if constexpr (OP == F29_ONE) st29(o, F::one());
  else if constexpr (OP == F29_UNPACK) { uint32_t w[8];                                                   // eight words in (the ninth is ignored), nine limbs out
#pragma unroll
    for (int j = 0; j < 8; j++) w[j] = a[e + j];
    st29(o, F::unpack(w)); }
  else if constexpr (OP == F29_PACK_WORDS) { uint32_t w[8]; ld29<F>(a + e).pack_words(w); st8(o, w); }     // nine limbs in, eight words (and a zero) out
  else if constexpr (OP == F29_TO_WORDS) { uint32_t w[8]; ld29<F>(a + e).to_words(w); st8(o, w); }
  else if constexpr (OP == F29_PRODUCT_IS_ZERO) { F r = ld29<F>(a + e); const bool z = fq29_product_is_zero(r);
#pragma unroll
    for (int j = 0; j < 9; j++) o[j] = j == 0 && z ? 1u : 0u; }
  else {
    // the laziest sequence ntt29_lds_pass (ntt.cuh) may rely on: a normalized u through two butterfly stages without a carry step (t1, t2: products' results),
    // each result the WIDE operand of a product with a normalized twiddle w, and the butterfly that follows it, normalized.
    // out: dd = (u - t1) - t2 | ss = (u + t1) + t2 | dd w | ss w | norm(u - dd w)
    const F u = ld29<F>(a + e), t1 = ld29<F>(b + e), t2 = ld29<F>(c + e), w = ld29<F>(d + e);
    const F dd = F::sub_product(F::sub_product(u, t1), t2), ss = F::add_raw(F::add_raw(u, t1), t2), pd = F::mul(dd, w), ps = F::mul(ss, w);
    st29(o, dd); st29(o + 9, ss); st29(o + 18, pd); st29(o + 27, ps); st29(o + 36, F::sub_product(u, pd).norm());
  }
}

void probe_field29(int field, int op, const uint32_t *a, const uint32_t *b, const uint32_t *c, const uint32_t *d, uint32_t *out, size_t n) {
  if (field != 0 && field != 1) throw GpuError("probe_field29: field must be 0 (Fr29) or 1 (Fq29)");
  if (op < 0 || op >= F29_OPS) throw GpuError("probe_field29: unknown operation");
  if (!n) return;
  const size_t in_bytes = n * 9 * sizeof(uint32_t), out_bytes = n * field29_out_words(op) * sizeof(uint32_t);
  const uint32_t *src[4] = {a, b, c, d}; DevBuf<uint8_t> in[4]; const uint32_t *dev[4] = {nullptr, nullptr, nullptr, nullptr};
  for (int k = 0; k < 4; k++) if (src[k]) { in[k] = DevBuf<uint8_t>(in_bytes); in[k].upload((const uint8_t *)src[k], in_bytes); dev[k] = (const uint32_t *)in[k].get(); }
  const int need = op == F29_MUL2 || op == F29_NTT_LAZY ? 4 : op == F29_ONE ? 0
      : (op == F29_MUL || (op >= F29_SUB2 && op <= F29_SUB_PRODUCT) || op == F29_ADD_RAW) ? 2 : 1;
  for (int k = 0; k < need; k++) if (!dev[k]) throw GpuError("probe_field29: an operand of this operation is missing");
  DevBuf<uint8_t> dout(out_bytes); const unsigned g = (unsigned)((n + 255) / 256); hipStream_t s = gpu_stream();
#define ZK_F29(F, OP) case OP: hipLaunchKernelGGL((k_probe_f29<F, OP>), dim3(g), dim3(256), 0, s, dev[0], dev[1], dev[2], dev[3], (uint32_t *)dout.get(), (uint32_t)n); break
  if (field == 1) switch (op) {
    ZK_F29(Fq29, F29_MUL); ZK_F29(Fq29, F29_MUL2); ZK_F29(Fq29, F29_SQR); ZK_F29(Fq29, F29_NORM); ZK_F29(Fq29, F29_SUB2); ZK_F29(Fq29, F29_SUB4); ZK_F29(Fq29, F29_SUB6);
    ZK_F29(Fq29, F29_SUB12); ZK_F29(Fq29, F29_SUB18); ZK_F29(Fq29, F29_COND_NEG); ZK_F29(Fq29, F29_SUB_PRODUCT); ZK_F29(Fq29, F29_NEG_PRODUCT); ZK_F29(Fq29, F29_ADD_RAW);
    ZK_F29(Fq29, F29_BARRETT); ZK_F29(Fq29, F29_ONE); ZK_F29(Fq29, F29_UNPACK); ZK_F29(Fq29, F29_PACK_WORDS); ZK_F29(Fq29, F29_TO_WORDS); ZK_F29(Fq29, F29_PRODUCT_IS_ZERO);
    default: throw GpuError("probe_field29: Fq29 has no such operation");
  } else switch (op) {                                                                  // (Fr29 has no borrow-adjusted constants: the transforms only subtract products)
    ZK_F29(Fr29, F29_MUL); ZK_F29(Fr29, F29_SQR); ZK_F29(Fr29, F29_NORM); ZK_F29(Fr29, F29_SUB_PRODUCT); ZK_F29(Fr29, F29_NEG_PRODUCT); ZK_F29(Fr29, F29_ADD_RAW);
    ZK_F29(Fr29, F29_UNPACK); ZK_F29(Fr29, F29_PACK_WORDS); ZK_F29(Fr29, F29_TO_WORDS); ZK_F29(Fr29, F29_NTT_LAZY);
    default: throw GpuError("probe_field29: Fr29 has no such operation");
  }
#undef ZK_F29
  HIP_CHECK(hipGetLastError()); dout.download((uint8_t *)out, out_bytes);
}

// ---- point formulas: raw limbs of the coordinates in, raw limbs and one flag word a point out --------------------------------------------------------------------
// G1 accumulator: X | Y | ZZ | ZZZ (36 words, the order of a Piece29).  Affine operand: x | y | sign (19 words): sign bit 0 set = the point's negative.
// G2, lane-serial (XYZZ2_29): X.c0 X.c1 Y.c0 Y.c1 ZZ.c0 ZZ.c1 ZZZ.c0 ZZZ.c1 (72 words); affine: x.c0 x.c1 y.c0 y.c1 | sign (37 words).
// G2, spread over eight lanes (OPoint29): slot e = 4 h + k as in a Point29Rec2: X.c0 Y.c0 ZZ.c0 ZZZ.c0 X.c1 Y.c1 ZZ.c1 ZZZ.c1 (72 words).
// The cooperative forms take the point at infinity as all-zero ZZ limbs, like the records the kernels read, and report it in bit 0 of the flag word.
enum { P29_MADD, P29_MADD_PP, P29_DBL_AFFINE, P29_ADD, P29_QUAD_ADD, P29_QUAD_ADD_OPP, P29_OCT_ADD, P29_FQ2_MUL, P29_FQ2_SQR, P29_G2_MADD, P29_MADD_CHAIN, P29_OPS };
static constexpr int P29_CHAIN = 32;
struct Point29Shape { int a, b, out, lanes; };
static Point29Shape point29_shape(int op) {
  switch (op) {
    case P29_MADD: case P29_MADD_PP: return {36, 19, 36, 1};
    case P29_DBL_AFFINE: return {0, 19, 36, 1};
    case P29_ADD: return {36, 36, 36, 1};
    case P29_QUAD_ADD: case P29_QUAD_ADD_OPP: return {36, 36, 36, 4};
    case P29_OCT_ADD: return {72, 72, 72, 8};
    case P29_FQ2_MUL: return {18, 18, 18, 1};
    case P29_FQ2_SQR: return {18, 0, 18, 1};
    case P29_G2_MADD: return {72, 37, 72, 1};
    case P29_MADD_CHAIN: return {36, 19 * P29_CHAIN, 36 * P29_CHAIN, 1};
    default: throw GpuError("probe_point29: unknown operation");
  }
}
__device__ __forceinline__ XYZZ29 ld_xyzz29(const uint32_t *p) { XYZZ29 r; r.X = ld29<Fq29>(p); r.Y = ld29<Fq29>(p + 9); r.ZZ = ld29<Fq29>(p + 18); r.ZZZ = ld29<Fq29>(p + 27); return r; }
__device__ __forceinline__ void st_xyzz29(uint32_t *p, const XYZZ29 &v) { st29(p, v.X); st29(p + 9, v.Y); st29(p + 18, v.ZZ); st29(p + 27, v.ZZZ); }
__device__ __forceinline__ Fq2_29 ld_fq2_29(const uint32_t *p) { return {ld29<Fq29>(p), ld29<Fq29>(p + 9)}; }
__device__ __forceinline__ void st_fq2_29(uint32_t *p, const Fq2_29 &v) { st29(p, v.c0); st29(p + 9, v.c1); }
__device__ __forceinline__ bool all_zero9(const uint32_t *p) { uint32_t o = 0;
#pragma unroll
  for (int i = 0; i < 9; i++) o |= p[i];
  return o == 0; }

// lane-serial forms: one point a lane
template <int OP> __global__ void __launch_bounds__(256) k_probe_p29(const uint32_t *a, const uint32_t *b, uint32_t *out, uint32_t *flags, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; if (i >= n) return;
  uint32_t fl = 0;
  if constexpr (OP == P29_MADD || OP == P29_MADD_PP) {
    // the operand as k_hacc_runs29 / k_wacc_lanes29 feed it: x canonical, y canonical or the WIDE K_2 - y
    XYZZ29 acc = ld_xyzz29(a + (size_t)i * 36); const uint32_t *q = b + (size_t)i * 19;
    const Fq29 px = ld29<Fq29>(q), py = Fq29::cond_neg(ld29<Fq29>(q + 9), (q[18] & 1u) != 0); Fq29 Pv, Rv; acc.madd_head(px, py, Pv, Rv);
    if constexpr (OP == P29_MADD) acc.madd_tail(Pv, Rv);
    else { const Fq29 PP = Fq29::sqr(Pv); fl = (fq29_product_is_zero(PP) ? 1u : 0u) | (fq29_product_is_zero(Fq29::sqr(Rv)) ? 2u : 0u); acc.madd_tail_pp(Pv, Rv, PP); }
    st_xyzz29(out + (size_t)i * 36, acc);
  } else if constexpr (OP == P29_DBL_AFFINE) {
    const uint32_t *q = b + (size_t)i * 19; const Fq29 px = ld29<Fq29>(q), y = ld29<Fq29>(q + 9);
    st_xyzz29(out + (size_t)i * 36, xyzz29_dbl_affine(px, (q[18] & 1u) ? Fq29::cond_neg(y, true).norm() : y));
  } else if constexpr (OP == P29_ADD) {
    const XYZZ29 r = xyzz29_add(ld_xyzz29(a + (size_t)i * 36), ld_xyzz29(b + (size_t)i * 36)); fl = fq29_product_is_zero(r.ZZ) ? 2u : 0u;
    st_xyzz29(out + (size_t)i * 36, r);
  } else if constexpr (OP == P29_FQ2_MUL) st_fq2_29(out + (size_t)i * 18, fq2_29_mul(ld_fq2_29(a + (size_t)i * 18), ld_fq2_29(b + (size_t)i * 18)));
  else if constexpr (OP == P29_FQ2_SQR) st_fq2_29(out + (size_t)i * 18, fq2_29_sqr(ld_fq2_29(a + (size_t)i * 18)));
  else if constexpr (OP == P29_G2_MADD) {
    const uint32_t *p = a + (size_t)i * 72, *q = b + (size_t)i * 37; const bool neg = (q[36] & 1u) != 0;
    XYZZ2_29 acc; acc.X = ld_fq2_29(p); acc.Y = ld_fq2_29(p + 18); acc.ZZ = ld_fq2_29(p + 36); acc.ZZZ = ld_fq2_29(p + 54);
    const Fq2_29 px = ld_fq2_29(q), py = {Fq29::cond_neg(ld29<Fq29>(q + 18), neg).norm(), Fq29::cond_neg(ld29<Fq29>(q + 27), neg).norm()};   // (g2_29_unpack)
    acc.madd(px, py);
    uint32_t *o = out + (size_t)i * 72; st_fq2_29(o, acc.X); st_fq2_29(o + 18, acc.Y); st_fq2_29(o + 36, acc.ZZ); st_fq2_29(o + 54, acc.ZZZ);
  } else {
    // a run of k_hacc_runs29: one accumulator, P29_CHAIN mixed additions, the limbs after every one of them
    XYZZ29 acc = ld_xyzz29(a + (size_t)i * 36); const uint32_t *q = b + (size_t)i * 19 * P29_CHAIN; uint32_t *o = out + (size_t)i * 36 * P29_CHAIN;
#pragma unroll 1
    for (int j = 0; j < P29_CHAIN; j++, q += 19, o += 36) {
      const Fq29 px = ld29<Fq29>(q), py = Fq29::cond_neg(ld29<Fq29>(q + 9), (q[18] & 1u) != 0); Fq29 Pv, Rv;
      acc.madd_head(px, py, Pv, Rv); acc.madd_tail(Pv, Rv); st_xyzz29(o, acc);
    }
  }
  flags[i] = fl;
}
// cooperative forms: a point spread over LANES = 4 or 8 lanes; the host pads the operands to whole workgroups (all-zero points: infinity), so that every lane
// of every wave is active in the DPP moves
template <int OP> __global__ void __launch_bounds__(256) k_probe_p29_coop(const uint32_t *a, const uint32_t *b, uint32_t *out, uint32_t *flags) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if constexpr (OP == P29_OCT_ADD) {
    const uint32_t pt = t >> 3; const int e = t & 7, k = e & 3; const bool h0 = e < 4; const uint32_t *pa = a + (size_t)pt * 72, *pb = b + (size_t)pt * 72;
    OPoint29 A, B; A.c = ld29<Fq29>(pa + 9 * e); B.c = ld29<Fq29>(pb + 9 * e);
    A.inf = all_zero9(pa + 18) && all_zero9(pa + 54); B.inf = all_zero9(pb + 18) && all_zero9(pb + 54);
    const OPoint29 r = oct29_add(A, B, k, h0); st29(out + (size_t)pt * 72 + 9 * e, r.c); if (e == 0) flags[pt] = r.inf ? 1u : 0u;
  } else {
    const uint32_t pt = t >> 2; const int k = t & 3; const uint32_t *pa = a + (size_t)pt * 36, *pb = b + (size_t)pt * 36;
    QPoint29 A, B; A.c = ld29<Fq29>(pa + 9 * k); B.c = ld29<Fq29>(pb + 9 * k); A.inf = all_zero9(pa + 18); B.inf = all_zero9(pb + 18);
    const QPoint29 r = quad29_add<OP == P29_QUAD_ADD_OPP>(A, B, k); st29(out + (size_t)pt * 36 + 9 * k, r.c); if (k == 0) flags[pt] = r.inf ? 1u : 0u;
  }
}

void probe_point29(int op, const uint32_t *a, const uint32_t *b, uint32_t *out, uint32_t *flags, size_t n) {
  if (op < 0 || op >= P29_OPS) throw GpuError("probe_point29: unknown operation");
  const Point29Shape sh = point29_shape(op);
  if ((sh.a && !a) || (sh.b && !b) || !out || !flags) throw GpuError("probe_point29: an operand of this operation is missing");
  if (!n) return;
  const size_t per_block = 256 / sh.lanes, n_pad = (n + per_block - 1) / per_block * per_block;    // whole workgroups of points
  auto up = [&](const uint32_t *src, int words) { DevBuf<uint8_t> d(std::max<size_t>(n_pad * words, 1) * 4); d.zero(); if (words) d.upload((const uint8_t *)src, n * words * 4); return d; };
  DevBuf<uint8_t> da = up(a, sh.a), db = up(b, sh.b), dout(n_pad * sh.out * 4), dfl(n_pad * 4); dfl.zero();
  const uint32_t *pa = (const uint32_t *)da.get(), *pb = (const uint32_t *)db.get(); uint32_t *po = (uint32_t *)dout.get(), *pf = (uint32_t *)dfl.get();
  const unsigned g = (unsigned)(n_pad / per_block); hipStream_t s = gpu_stream();
#define ZK_P29(OP) case OP: hipLaunchKernelGGL((k_probe_p29<OP>), dim3(g), dim3(256), 0, s, pa, pb, po, pf, (uint32_t)n); break
#define ZK_P29C(OP) case OP: hipLaunchKernelGGL((k_probe_p29_coop<OP>), dim3(g), dim3(256), 0, s, pa, pb, po, pf); break
  switch (op) {
    ZK_P29(P29_MADD); ZK_P29(P29_MADD_PP); ZK_P29(P29_DBL_AFFINE); ZK_P29(P29_ADD); ZK_P29(P29_FQ2_MUL); ZK_P29(P29_FQ2_SQR); ZK_P29(P29_G2_MADD); ZK_P29(P29_MADD_CHAIN);
    ZK_P29C(P29_QUAD_ADD); ZK_P29C(P29_QUAD_ADD_OPP); ZK_P29C(P29_OCT_ADD);
  }
#undef ZK_P29
#undef ZK_P29C
  HIP_CHECK(hipGetLastError()); dout.download((uint8_t *)out, n * sh.out * 4); dfl.download((uint8_t *)flags, n * 4);
}
}  // namespace zk
