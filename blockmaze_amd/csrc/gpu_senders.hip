// Senders from signatures (DESIGN.md "Senders from signatures"; include/zk_senders.h): what the reference computes per transaction as types.Sender -> recoverPlain
// (core/types/transaction_signing.go:246-271) -> crypto.ValidateSignatureValues (crypto/crypto.go:199-210) -> crypto.Ecrecover -> secp256k1_ecdsa_recover
// (libsecp256k1 src/modules/recovery/main_impl.h:87-121) -> Keccak256(pub[1:])[12:], for n signatures in one call, one lane a signature.
// Six launches, in order on the library's main stream (lane 0) under the device mutex:
//   k_secp_lift      the checks of ValidateSignatureValues; R = (r, y) with y = (r^3 + 7)^((p+1)/4), refused where y^2 != r^3 + 7, y's parity from V
//   k_secp_scalars   u1 = -m / r, u2 = s / r mod N, m = hash mod N
//   k_secp_rtable    1 R ... 15 R, affine (one inversion a lane, Montgomery's trick over the fourteen Z)
//   k_secp_walk      Q = u1 G + u2 R: 64 windows of 4 bits from the top, four doublings and up to two mixed additions a window (Strauss)
//   k_secp_affine    Q affine, or the lane refused where Q is infinity
//   k_secp_address   Keccak-256 of X || Y, bytes 12 .. 31; ok, froms and pubs written, zero where the lane was refused
// The workspace is lane-interleaved: word j of lane i lies at W[j * stride + i], so the 64 lanes of a wave read 64 consecutive words.  1 G ... 15 G lie in a table of
// their own, built once by k_secp_gtable.  The R multiples are in the workspace, never in a private array: a digit is a run-time index.
// Rules every kernel keeps: no lane waits for another lane, wave or workgroup; every loop has a constant bound; what a launch writes with plain stores
// (everything but the four counters, which are atomicAdd only) is read by other lanes — here: by no other lane at all — only in later launches; no kernel uses scratch.
#include <algorithm>
#include <cstring>
#include <string>
#include "gpu_internal.hpp"
#include "secp256k1.cuh"
#include "txs_host.hpp"

namespace zk {
using namespace secp;

constexpr int SP_THREADS = 128;
// the workspace of a lane, in words
constexpr int SW_FLAG = 0, SW_RX = 1, SW_RY = 9, SW_U1 = 17, SW_U2 = 25, SW_QX = 33, SW_QY = 41, SW_QZ = 49, SW_QINF = 57, SW_TAB = 58;
constexpr int SW_ENTRY = 32 /* x, y, then during the build z and the running product */, SW_WORDS = SW_TAB + 15 * SW_ENTRY;
constexpr int SP_HEAD = 4;                            // the call's head: the four counters
enum { SO_FQ_MUL, SO_FQ_SQR, SO_FQ_ADD, SO_FQ_SUB, SO_FQ_NEG, SO_FQ_INV, SO_FQ_SQRT, SO_FQ_REDUCE, SO_N_MUL, SO_N_INV, SO_N_REDUCE, SO_OPS };

struct Ws { uint32_t *w; size_t stride; };
__device__ __forceinline__ U256 ws_get(const Ws &W, uint32_t lane, int word) { U256 r;
#pragma unroll
  for (int i = 0; i < 8; i++) r.l[i] = W.w[(size_t)(word + i) * W.stride + lane];
  return r; }
__device__ __forceinline__ void ws_put(const Ws &W, uint32_t lane, int word, const U256 &v) {
#pragma unroll
  for (int i = 0; i < 8; i++) W.w[(size_t)(word + i) * W.stride + lane] = v.l[i]; }
__device__ __forceinline__ uint32_t &ws_word(const Ws &W, uint32_t lane, int word) { return W.w[(size_t)word * W.stride + lane]; }

// crypto.go:199-210: r, s >= 1; homestead: s <= N / 2; r, s < N; v is 0 or 1.  Then libsecp256k1's recovery with recid = v: x = r (recid & 2 is never set), the
// point with that x and y's parity = recid & 1, refused where x is no x of the curve.
__global__ void __launch_bounds__(SP_THREADS) k_secp_lift(const uint32_t *__restrict__ rs, const uint8_t *__restrict__ v, uint32_t n, int homestead, Ws W) {
  const uint32_t i = blockIdx.x * SP_THREADS + threadIdx.x; if (i >= n) return;
  const U256 r = load_be(rs + 16 * (size_t)i), s = load_be(rs + 16 * (size_t)i + 8); const uint32_t vb = v[i];
  bool ok = !u256_is_zero(r) && !u256_is_zero(s) && !u256_geq(r, FnP::MOD) && !u256_geq(s, FnP::MOD) && vb <= 1;
  if (homestead && u256_geq(s, N_HALF) && !u256_eq(s, u256_of(N_HALF))) ok = false;
  if (ok) {                                                                                        // r < N < p: r is a canonical field element
    const Fe y2 = fe_add(fe_mul(fe_sqr(r), r), u256_small(7)); Fe y = fe_sqrt(y2);
    if (!u256_eq(fe_sqr(y), y2)) ok = false;
    else { if ((y.l[0] & 1u) != vb) y = fe_neg(y); ws_put(W, i, SW_RX, r); ws_put(W, i, SW_RY, y); }
  }
  ws_word(W, i, SW_FLAG) = ok ? 1u : 0u;
}
__global__ void __launch_bounds__(SP_THREADS) k_secp_scalars(const uint32_t *__restrict__ hash, const uint32_t *__restrict__ rs, uint32_t n, Ws W) {
  const uint32_t i = blockIdx.x * SP_THREADS + threadIdx.x; if (i >= n) return;
  if (!ws_word(W, i, SW_FLAG)) return;
  const Sc r = load_be(rs + 16 * (size_t)i), s = load_be(rs + 16 * (size_t)i + 8), m = mod_reduce<FnP>(load_be(hash + 8 * (size_t)i)), ri = sc_inv(r);
  ws_put(W, i, SW_U1, mod_neg<FnP>(sc_mul(m, ri))); ws_put(W, i, SW_U2, sc_mul(s, ri));
}
// the test entry's way in: u1, u2 and an affine point as they come (canonical; the point on the curve and not infinity)
__global__ void __launch_bounds__(SP_THREADS) k_secp_load_lincomb(const uint32_t *__restrict__ in, uint32_t n, Ws W) {
  const uint32_t i = blockIdx.x * SP_THREADS + threadIdx.x; if (i >= n) return;
  ws_put(W, i, SW_U1, load_be(in + 8 * (size_t)i)); ws_put(W, i, SW_U2, load_be(in + 8 * ((size_t)n + i)));
  ws_put(W, i, SW_RX, load_be(in + 8 * (2 * (size_t)n + i))); ws_put(W, i, SW_RY, load_be(in + 8 * (3 * (size_t)n + i))); ws_word(W, i, SW_FLAG) = 1u;
}
// Entry k of the table, k = 1 .. 15, is k R.  R has prime order N > 15, so no multiple is infinity, no two operands of the fourteen additions are equal or opposite
// ((k - 1) R = +-R only for k = 2, which is the doubling, or k = 0) and no Z is zero; gej_add_ge has its branches all the same.
__global__ void __launch_bounds__(SP_THREADS) k_secp_rtable(uint32_t n, Ws W) {
  const uint32_t i = blockIdx.x * SP_THREADS + threadIdx.x; if (i >= n) return;
  if (!ws_word(W, i, SW_FLAG)) return;
  Ge R; R.x = ws_get(W, i, SW_RX); R.y = ws_get(W, i, SW_RY); AddCounters unused;
  ws_put(W, i, SW_TAB, R.x); ws_put(W, i, SW_TAB + 8, R.y);
  Gej J; J.x = R.x; J.y = R.y; J.z = u256_small(1); J.inf = false; J = gej_double(J); Fe run = J.z;
#pragma unroll 1
  for (int k = 2; k <= 15; k++) {                                                                  // entry k: X, Y, Z and Z_2 ... Z_k
    if (k > 2) { J = gej_add_ge(J, R, unused); run = fe_mul(run, J.z); }
    const int e = SW_TAB + (k - 1) * SW_ENTRY; ws_put(W, i, e, J.x); ws_put(W, i, e + 8, J.y); ws_put(W, i, e + 16, J.z); ws_put(W, i, e + 24, run);
  }
  Fe inv = fe_inv(run);                                                                            // 1 / (Z_2 ... Z_15)
#pragma unroll 1
  for (int k = 15; k >= 2; k--) {
    const int e = SW_TAB + (k - 1) * SW_ENTRY; Fe zi = inv;
    if (k > 2) { zi = fe_mul(inv, ws_get(W, i, e - SW_ENTRY + 24)); inv = fe_mul(inv, ws_get(W, i, e + 16)); }   // 1 / Z_k; then inv = 1 / (Z_2 ... Z_(k-1))
    const Fe zi2 = fe_sqr(zi); ws_put(W, i, e, fe_mul(ws_get(W, i, e), zi2)); ws_put(W, i, e + 8, fe_mul(fe_mul(ws_get(W, i, e + 8), zi2), zi));
  }
}
// Q = u1 G + u2 R.  The digits come from the workspace word by word and the table entries from memory: nothing here is indexed in registers.
__global__ void __launch_bounds__(SP_THREADS) k_secp_walk(uint32_t n, Ws W, const uint32_t *__restrict__ gtab, uint32_t *__restrict__ head) {
  const uint32_t i = blockIdx.x * SP_THREADS + threadIdx.x; if (i >= n) return;
  if (!ws_word(W, i, SW_FLAG)) return;
  Gej Q; Q.x = u256_zero(); Q.y = u256_zero(); Q.z = u256_zero(); Q.inf = true; AddCounters cnt;
#pragma unroll 1
  for (int win = 63; win >= 0; win--) {
    if (!Q.inf) {
#pragma unroll 1
      for (int d = 0; d < 4; d++) Q = gej_double(Q);
    }
    const int word = win >> 3, shift = 4 * (win & 7);
    const uint32_t d1 = (ws_word(W, i, SW_U1 + word) >> shift) & 15u, d2 = (ws_word(W, i, SW_U2 + word) >> shift) & 15u;
    if (d1) { Ge P; const uint32_t *g = gtab + 16 * (d1 - 1);
#pragma unroll
      for (int j = 0; j < 8; j++) { P.x.l[j] = g[j]; P.y.l[j] = g[8 + j]; }
      Q = gej_add_ge(Q, P, cnt); }
    if (d2) { Ge P; const int e = SW_TAB + (int)(d2 - 1) * SW_ENTRY; P.x = ws_get(W, i, e); P.y = ws_get(W, i, e + 8); Q = gej_add_ge(Q, P, cnt); }
  }
  ws_put(W, i, SW_QX, Q.x); ws_put(W, i, SW_QY, Q.y); ws_put(W, i, SW_QZ, Q.z); ws_word(W, i, SW_QINF) = Q.inf ? 1u : 0u;
  if (cnt.equal) atomicAdd(head + 0, cnt.equal);
  if (cnt.opposite) atomicAdd(head + 1, cnt.opposite);
  if (cnt.at_infinity) atomicAdd(head + 2, cnt.at_infinity);
  if (cnt.to_infinity) atomicAdd(head + 3, cnt.to_infinity);
}
__global__ void __launch_bounds__(SP_THREADS) k_secp_affine(uint32_t n, Ws W) {
  const uint32_t i = blockIdx.x * SP_THREADS + threadIdx.x; if (i >= n) return;
  if (!ws_word(W, i, SW_FLAG)) return;
  if (ws_word(W, i, SW_QINF)) { ws_word(W, i, SW_FLAG) = 0u; return; }                             // Q at infinity: recoverPlain's "invalid public key"
  const Fe zi = fe_inv(ws_get(W, i, SW_QZ)), zi2 = fe_sqr(zi);
  ws_put(W, i, SW_QX, fe_mul(ws_get(W, i, SW_QX), zi2)); ws_put(W, i, SW_QY, fe_mul(fe_mul(ws_get(W, i, SW_QY), zi2), zi));
}
__global__ void __launch_bounds__(SP_THREADS) k_secp_address(uint32_t n, Ws W, uint8_t *__restrict__ ok, uint32_t *__restrict__ froms, uint32_t *__restrict__ pubs) {
  const uint32_t i = blockIdx.x * SP_THREADS + threadIdx.x; if (i >= n) return;
  const bool good = ws_word(W, i, SW_FLAG) != 0; uint32_t a[5] = {0, 0, 0, 0, 0}; Fe x = u256_zero(), y = u256_zero();
  if (good) { x = ws_get(W, i, SW_QX); y = ws_get(W, i, SW_QY); address_of(x, y, a); }
  ok[i] = good ? 1 : 0;
#pragma unroll
  for (int k = 0; k < 5; k++) froms[5 * (size_t)i + k] = a[k];
  if (pubs) { if (good) { store_be(pubs + 16 * (size_t)i, x); store_be(pubs + 16 * (size_t)i + 8, y); }
    else {
#pragma unroll
      for (int k = 0; k < 16; k++) pubs[16 * (size_t)i + k] = 0u; } }
}
// the resident table: lane k computes (k + 1) G by k + 1 additions of G — the first meets infinity, the second equal operands — and one inversion
__global__ void __launch_bounds__(64) k_secp_gtable(uint32_t *__restrict__ gtab) {
  const uint32_t k = threadIdx.x; if (k >= 15) return;
  Ge G; G.x = u256_of(GX); G.y = u256_of(GY); Gej J; J.x = u256_zero(); J.y = u256_zero(); J.z = u256_zero(); J.inf = true; AddCounters unused;
#pragma unroll 1
  for (uint32_t j = 0; j < 15; j++) if (j <= k) J = gej_add_ge(J, G, unused);
  const Fe zi = fe_inv(J.z), zi2 = fe_sqr(zi), x = fe_mul(J.x, zi2), y = fe_mul(fe_mul(J.y, zi2), zi);
#pragma unroll
  for (int j = 0; j < 8; j++) { gtab[16 * k + j] = x.l[j]; gtab[16 * k + 8 + j] = y.l[j]; }
}
// raw operations, one lane an operand pair, 32 big-endian bytes an operand (zkgpu_test_secp_ops)
__global__ void __launch_bounds__(SP_THREADS) k_secp_op(int op, const uint32_t *__restrict__ a, const uint32_t *__restrict__ b, uint32_t *__restrict__ out, uint32_t n) {
  const uint32_t i = blockIdx.x * SP_THREADS + threadIdx.x; if (i >= n) return;
  const U256 x = load_be(a + 8 * (size_t)i), y = load_be(b + 8 * (size_t)i); U256 r = u256_zero();
  switch (op) {
    case SO_FQ_MUL: r = fe_mul(x, y); break;
    case SO_FQ_SQR: r = fe_sqr(x); break;
    case SO_FQ_ADD: r = fe_add(x, y); break;
    case SO_FQ_SUB: r = fe_sub(x, y); break;
    case SO_FQ_NEG: r = fe_neg(x); break;
    case SO_FQ_INV: r = fe_inv(x); break;
    case SO_FQ_SQRT: r = fe_sqrt(x); break;
    case SO_FQ_REDUCE: r = mod_reduce<FqP>(x); break;
    case SO_N_MUL: r = sc_mul(x, y); break;
    case SO_N_INV: r = sc_inv(x); break;
    case SO_N_REDUCE: r = mod_reduce<FnP>(x); break;
  }
  store_be(out + 8 * (size_t)i, r);
}

// ---- the host side ------------------------------------------------------------------------------------------------------------------------------------------------
namespace {
static_assert(TXL_SP_HEAD == SP_HEAD, "txs_layout.hpp carves the output of these kernels");
struct Senders : PinnedStage {                       // one a process, every member under the device mutex
  DevBuf<uint32_t> gtab, work, io; size_t stride = 0; bool table_built = false;
  uint64_t counters[4] = {0, 0, 0, 0};
  // the workspace for n lanes (kept and grown; the stride a multiple of 64, so that a wave's 64 words start on a 256-byte line) and the table of G
  Ws prepare(size_t n, hipStream_t s) {
    if (!table_built) { gtab = DevBuf<uint32_t>(15 * 16); hipLaunchKernelGGL(k_secp_gtable, dim3(1), dim3(64), 0, s, gtab.get()); HIP_CHECK(hipGetLastError());
      HIP_CHECK(hipStreamSynchronize(s)); table_built = true; }
    if (stride < n) {                                                                              // (no workspace at all while the new one is not there: an allocation that throws leaves stride 0, and the next call grows again)
      const size_t want = (std::max(n, 2 * stride) + 63) / 64 * 64; stride = 0; work = DevBuf<uint32_t>(); work = DevBuf<uint32_t>(want * SW_WORDS); stride = want; }
    if (n && (!work.get() || stride < n)) throw GpuError("senders: no workspace");
    return Ws{work.get(), stride};
  }
  // rtable, walk, affine, address on lanes whose R, u1, u2 and flag are in the workspace; out: the head | ok n bytes (padded to words) | froms 5n | pubs 16n
  void tail(size_t n, const Ws &W, uint32_t *out, bool want_pubs, hipStream_t s) {
    const dim3 grid(cdiv(n, SP_THREADS)), block(SP_THREADS); const uint32_t nn = (uint32_t)n; const SendersOut o = senders_out(n, want_pubs);
    HIP_CHECK(hipMemsetAsync(out, 0, 4 * SP_HEAD, s));
    hipLaunchKernelGGL(k_secp_rtable, grid, block, 0, s, nn, W);
    hipLaunchKernelGGL(k_secp_walk, grid, block, 0, s, nn, W, (const uint32_t *)gtab.get(), out);
    hipLaunchKernelGGL(k_secp_affine, grid, block, 0, s, nn, W);
    hipLaunchKernelGGL(k_secp_address, grid, block, 0, s, nn, W, (uint8_t *)(out + o.ok), out + o.froms, want_pubs ? out + o.pubs : (uint32_t *)nullptr);
    HIP_CHECK(hipGetLastError());
  }
  // the recovery on records that lie on the device: hash 8 words a record, R || S 16 words, V one byte; lift, scalars, then the tail.  Queues only.
  void body(size_t n, const uint32_t *hash, const uint32_t *rs, const uint8_t *v, bool homestead, const Ws &W, uint32_t *out, bool want_pubs, hipStream_t s) {
    const dim3 grid(cdiv(n, SP_THREADS)), block(SP_THREADS);
    hipLaunchKernelGGL(k_secp_lift, grid, block, 0, s, rs, v, (uint32_t)n, homestead ? 1 : 0, W);
    hipLaunchKernelGGL(k_secp_scalars, grid, block, 0, s, hash, rs, (uint32_t)n, W);
    tail(n, W, out, want_pubs, s);
  }
  void keep_counters(const uint8_t *back) { uint32_t h[SP_HEAD]; memcpy(h, back, sizeof h); for (int k = 0; k < 4; k++) counters[k] = h[k]; }
};
Senders &senders() { static Senders *s = new Senders; return *s; }   // (never destroyed: the runtime may be gone when statics are)
}  // namespace

// n records: sighash n x 32, sigs n x 65 (R || S || V).  froms n x 20, pubs n x 64 or null, ok n.  Returns the number of records with ok = 1.  The caller has checked
// the pointers and holds nothing; one upload of 97 n bytes, six launches, one download of 85 n (21 n without pubs) bytes.
size_t recover_senders(const uint8_t *sighash, const uint8_t *sigs, size_t n, bool homestead, uint8_t *froms, uint8_t *pubs, uint8_t *ok) {
  if (!n) return 0;
  if (n > 0x7FFFFFFFu) throw GpuError("senders: more than 2^31 - 1 records");
  LaneScope lane(0); hipStream_t s = gpu().stream; Senders &d = senders();                          // (the C entry holds the device mutex, as for every routine below)
  // up, in words: hash 8n | r, s 16n | v n bytes.  Down: head | ok | froms | pubs.
  const SendersOut o = senders_out(n, pubs != nullptr); const size_t okw = Carve::bytes(n), up = 24 * n + okw, down = o.end;
  d.pinned(4 * (up + down)); uint8_t *const pu = d.pin, *const back = d.pin + 4 * up;
  memcpy(pu, sighash, 32 * n); uint8_t *prs = pu + 32 * n, *pv = pu + 96 * n; memset(pv, 0, 4 * okw);
  for (size_t i = 0; i < n; i++) { memcpy(prs + 64 * i, sigs + 65 * i, 64); pv[i] = sigs[65 * i + 64]; }
  grow_buf(d.io, up + down); uint32_t *in = d.io.get(), *out = in + up;
  SyncAtExit sync; const Ws W = d.prepare(n, s);
  HIP_CHECK(hipMemcpyAsync(in, pu, 4 * up, hipMemcpyHostToDevice, s));
  d.body(n, in, in + 8 * n, (const uint8_t *)(in + 24 * n), homestead, W, out, pubs != nullptr, s);
  HIP_CHECK(hipMemcpyAsync(back, out, 4 * down, hipMemcpyDeviceToHost, s)); HIP_CHECK(hipStreamSynchronize(s));
  d.keep_counters(back);
  memcpy(ok, back + 4 * o.ok, n); memcpy(froms, back + 4 * o.froms, 20 * n); if (pubs) memcpy(pubs, back + 4 * o.pubs, 64 * n);
  size_t good = 0; for (size_t i = 0; i < n; i++) good += ok[i] != 0;
  return good;
}
// The same six launches on records another routine left on the device (gpu_txs.hip): hash n x 8 words, rs n x 16 words, v n bytes, all big-endian bytes in memory
// order.  out: recover_senders_out_words(n) words: the head | ok n bytes (padded to words) | froms 5n.  Queues on s and returns; the caller holds the device mutex,
// synchronises, and hands the head to senders_keep_head.
size_t recover_senders_out_words(size_t n) { return senders_out(n, false).end; }
void recover_senders_queue(const uint32_t *hash, const uint32_t *rs, const uint8_t *v, size_t n, bool homestead, uint32_t *out, hipStream_t s) {
  if (!n) return;
  if (n > 0x7FFFFFFFu) throw GpuError("senders: more than 2^31 - 1 records");
  Senders &d = senders(); const Ws W = d.prepare(n, s); d.body(n, hash, rs, v, homestead, W, out, false, s);
}
void senders_keep_head(const uint32_t *head) { senders().keep_counters((const uint8_t *)head); }
// u1 G + u2 P through the launches of the recovery from k_secp_rtable on: 32 big-endian bytes a value; out_xy n x 64, zero where out_inf[i] = 1
void probe_secp_lincomb(const uint8_t *u1, const uint8_t *u2, const uint8_t *px, const uint8_t *py, size_t n, uint8_t *out_xy, uint8_t *out_inf) {
  if (!n) return;
  if (!u1 || !u2 || !px || !py || !out_xy || !out_inf) throw GpuError("probe_secp_lincomb: a null pointer");
  if (n > (1u << 24)) throw GpuError("probe_secp_lincomb: more than 2^24 lanes");
  LaneScope lane(0); hipStream_t s = gpu().stream; Senders &d = senders();                          // (the C entry holds the device mutex)
  const SendersOut o = senders_out(n, true); const size_t up = 32 * n, down = o.end;
  d.pinned(4 * (up + down)); uint8_t *const back = d.pin + 4 * up;
  memcpy(d.pin, u1, 32 * n); memcpy(d.pin + 32 * n, u2, 32 * n); memcpy(d.pin + 64 * n, px, 32 * n); memcpy(d.pin + 96 * n, py, 32 * n);
  grow_buf(d.io, up + down); uint32_t *in = d.io.get(), *out = in + up;
  SyncAtExit sync; const Ws W = d.prepare(n, s);
  HIP_CHECK(hipMemcpyAsync(in, d.pin, 4 * up, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_secp_load_lincomb, dim3(cdiv(n, SP_THREADS)), dim3(SP_THREADS), 0, s, (const uint32_t *)in, (uint32_t)n, W);
  d.tail(n, W, out, true, s);
  HIP_CHECK(hipMemcpyAsync(back, out, 4 * down, hipMemcpyDeviceToHost, s)); HIP_CHECK(hipStreamSynchronize(s));
  d.keep_counters(back);
  const uint8_t *bok = back + 4 * o.ok; for (size_t i = 0; i < n; i++) out_inf[i] = bok[i] ? 0 : 1;
  memcpy(out_xy, back + 4 * o.pubs, 64 * n);
}
void probe_secp_ops(int op, const uint8_t *a, const uint8_t *b, size_t n, uint8_t *out) {
  if (op < 0 || op >= SO_OPS) throw GpuError("probe_secp_ops: unknown operation");
  if (!n) return;
  if (!a || !out) throw GpuError("probe_secp_ops: a null pointer");
  LaneScope lane(0); hipStream_t s = gpu().stream; DevBuf<uint8_t> da(32 * n), db(32 * n), dout(32 * n);
  da.upload(a, 32 * n); db.upload(b ? b : a, 32 * n);
  hipLaunchKernelGGL(k_secp_op, dim3(cdiv(n, SP_THREADS)), dim3(SP_THREADS), 0, s, op, (const uint32_t *)da.get(), (const uint32_t *)db.get(), (uint32_t *)dout.get(), (uint32_t)n);
  HIP_CHECK(hipGetLastError()); dout.download(out, 32 * n);
}
// the resident table as it lies in device memory: entry k - 1 = k G, X || Y, big-endian, k = 1 .. 15
void probe_secp_gtable(uint8_t *out) {
  LaneScope lane(0); hipStream_t s = gpu().stream; Senders &d = senders(); d.prepare(0, s);
  uint32_t w[15 * 16]; d.gtab.download(w, 15 * 16);
  for (int k = 0; k < 15; k++) for (int c = 0; c < 2; c++) for (int j = 0; j < 8; j++) { const uint32_t v = w[16 * k + 8 * c + j]; uint8_t *o = out + 64 * k + 32 * c + 4 * (7 - j);
    o[0] = (uint8_t)(v >> 24); o[1] = (uint8_t)(v >> 16); o[2] = (uint8_t)(v >> 8); o[3] = (uint8_t)v; }
}
void senders_counters(uint64_t out[4]) { Senders &d = senders(); for (int k = 0; k < 4; k++) out[k] = d.counters[k]; }

}  // namespace zk
