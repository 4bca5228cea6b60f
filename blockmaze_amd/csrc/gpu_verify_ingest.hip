// Device ingest of the block check (DESIGN.md "Block verification", "From records"): from the records as a node holds them (include/zk_records.h: the proof as
// 512 hex characters, the statement as the bytes of its hashes) to the arrays k_block_records reads, and the integer sums of the equation's right-hand scalars.
// Nothing here is arithmetic worth the name: a byte gather, 8 + n_inputs field conversions and a sum per record — which is why it must not run on the host,
// 65,536 times a block, in front of 22 ms of kernels.
#include <algorithm>
#include <cstring>
#include "gpu_internal.hpp"
#include "pairing_types.cuh"

namespace zk {

// ---- k_ingest_records ------------------------------------------------------------------------------------------------------------------------------------------
// The statement of a kind is a bit string (capi_zk.cpp: public_bits): per argument the bytes of the blob — the common.Hash reversed —, the most significant bit of a
// byte first; value_s as eight little-endian bytes in the same bit order.  pack_public_bits cuts it into 253-bit little-endian chunks.  With every byte bit-reversed
// the string IS a little-endian integer W, input j = (W >> 253 j) mod 2^253; and 32-bit word i of an argument's share of W is __brev of the little-endian word at
// byte 28 - 4 i of the hash (pk, 20 bytes: at 16 - 4 i), so a word of W costs one LDS read and one v_bfrev.  Every argument is a whole number of words (8, 5 or 2).
constexpr uint32_t REC_BYTES = 720, REC_VEC = REC_BYTES / 16, REC_VALUE = 8, REC_PROOF = 16, REC_ARGS = 528;
constexpr uint32_t ING_RECORDS = 16, ING_THREADS = 256;   // records a workgroup takes: 128 lanes for their coordinates, up to 96 for their inputs

size_t record_num_inputs(int kind) { return kind == 0 || kind == 3 ? 4 : kind == 1 ? 5 : kind == 2 ? 6 : 0; }
static uint32_t record_words(int kind) { return kind == 1 ? 32 : kind == 2 ? 45 : 26; }   // 1,024 / 1,440 / 832 bits

__device__ __forceinline__ uint32_t stmt_word(const uint32_t *rec /* LDS, one record */, uint32_t kind, uint32_t n_words, uint32_t idx) {
  if (idx >= n_words) return 0;
  uint32_t arg, i;
  if (kind == 2) {                                                                       // deposit: RT, pk (five words), then four hashes
    if (idx < 8) { arg = 0; i = idx; }
    else if (idx < 13) return __brev(rec[(REC_ARGS + 32 + 16) / 4 - (idx - 8)]);
    else { arg = 2 + ((idx - 13) >> 3); i = (idx - 13) & 7; }
  } else if (kind != 1 && idx >= 24) return __brev(__builtin_bswap32(rec[REC_VALUE / 4 + (idx - 24)]));   // mint, redeem: value_s behind three hashes
  else { arg = idx >> 3; i = idx & 7; }
  return __brev(rec[(REC_ARGS + 32 * arg + 28) / 4 - i]);
}
// x -= m if x >= m; true if it did
__device__ __forceinline__ bool sub_if_geq(uint32_t x[8], const uint32_t m[8]) {
  uint32_t d[8]; uint64_t br = 0;
  for (int i = 0; i < 8; i++) { const uint64_t t = (uint64_t)x[i] - m[i] - br; d[i] = (uint32_t)t; br = (t >> 32) & 1; }
  if (br) return false;
  for (int i = 0; i < 8; i++) x[i] = d[i];
  return true;
}

static __global__ void __launch_bounds__(ING_THREADS) k_ingest_records(const uint4 *__restrict__ recs, uint32_t n, uint32_t kind, uint32_t n_inputs, uint32_t n_words,
    uint32_t strict, Fq *__restrict__ items /* n x 8 */, Fr *__restrict__ inputs /* n x n_inputs */, uint8_t *__restrict__ parsed) {
  __shared__ uint4 sh[ING_RECORDS * REC_VEC]; __shared__ uint32_t bad[ING_RECORDS];
  const uint32_t tid = threadIdx.x, r0 = blockIdx.x * ING_RECORDS, cnt = n - r0 < ING_RECORDS ? n - r0 : ING_RECORDS;
  for (uint32_t k = tid; k < cnt * REC_VEC; k += ING_THREADS) sh[k] = recs[(size_t)r0 * REC_VEC + k];
  if (tid < ING_RECORDS) bad[tid] = 0;
  __syncthreads();
  const uint32_t *sw = (const uint32_t *)sh;
  Fq v = Fq::zero(); const uint32_t prec = tid >> 3, coord = tid & 7; const bool proof_lane = tid < 8 * ING_RECORDS && prec < cnt;
  if (proof_lane) {
    // 64 digits, the most significant first: limb m is the eight characters at 56 - 8 m
    const uint32_t *hex = sw + (prec * REC_BYTES + REC_PROOF + 64 * coord) / 4; uint32_t x[8], fail = 0;
    for (int m = 0; m < 8; m++) {
      uint32_t limb = 0;
      for (int h = 0; h < 2; h++) { const uint32_t four = hex[14 - 2 * m + h];
        for (int k = 0; k < 4; k++) { const uint32_t ch = (four >> (8 * k)) & 0xffu, d = ch - '0', e = ch - 'a';
          fail |= (d > 9u) & (e > 5u); limb = (limb << 4) | (d <= 9u ? d : (e + 10u) & 15u); } }
      x[m] = limb;
    }
    // any 256-bit value is a coordinate (proof_from_hex): below q by conditional subtractions of 4q, 2q, q (4q < 2^256 < 6q) BEFORE the Montgomery product, whose
    // operands must be reduced; in strict mode a value that needed one is not a proof
    uint32_t q1[8], q2[8], q4[8];
    for (int i = 0; i < 8; i++) { q1[i] = FqParams::MOD[i]; q2[i] = (q1[i] << 1) | (i ? FqParams::MOD[i - 1] >> 31 : 0u); q4[i] = (q1[i] << 2) | (i ? FqParams::MOD[i - 1] >> 30 : 0u); }
    const bool s4 = sub_if_geq(x, q4), s2 = sub_if_geq(x, q2), s1 = sub_if_geq(x, q1);
    if (strict && (s4 || s2 || s1)) fail = 1;
    if (fail) atomicOr(&bad[prec], 1u);
    for (int i = 0; i < 8; i++) v.l[i] = x[i];
    v = v.to_mont();
  } else if (tid >= 8 * ING_RECORDS && tid - 8 * ING_RECORDS < cnt * n_inputs) {
    const uint32_t t = tid - 8 * ING_RECORDS, rec = t / n_inputs, j = t - rec * n_inputs; const uint32_t *rw = sw + rec * (REC_BYTES / 4);
    Fr out; uint32_t at = 253 * j, lo = stmt_word(rw, kind, n_words, at >> 5);
    for (int m = 0; m < 8; m++) {                                                          // bits [253 j + 32 m, + 32) of W: a funnel shift across two of its words
      const uint32_t hi = stmt_word(rw, kind, n_words, (at >> 5) + m + 1); out.l[m] = __funnelshift_r(lo, hi, at & 31); lo = hi; }
    out.l[7] &= 0x1fffffffu;                                                               // 253 = 7 x 32 + 29
    inputs[(size_t)(r0 + rec) * n_inputs + j] = out;
  }
  __syncthreads();
  if (proof_lane) {                                                                        // (an unparsed record's points are zeroed, as the host zeroes its Proof)
    const uint32_t slot = coord ^ (coord >= 2 && coord < 6 ? 1u : 0u);                     // hex order A.x A.y B.x.c1 B.x.c0 B.y.c1 B.y.c0 C.x C.y -> Proof's x0 x1 y0 y1
    items[(size_t)(r0 + prec) * 8 + slot] = bad[prec] ? Fq::zero() : v;
  }
  if (tid < cnt) parsed[r0 + tid] = bad[tid] ? 0 : 1;
}

struct RecordIngest::Impl { PinnedBuf<Fe32> stage; DevBuf<uint8_t> recs, items, inputs, parsed; size_t cap = 0, n = 0, ni = 0; };
RecordIngest::RecordIngest() : impl(new Impl) {}
RecordIngest::~RecordIngest() = default;
uint8_t *RecordIngest::stage(size_t n) {
  Impl &d = *impl; if (!n || n > (1u << 26)) throw GpuError("record ingest: record count");   // (64 M records: every size below stays far inside 64 bits, and cdiv's 32)
  if (n > d.cap) {
    const size_t cap = n + n / 4 + 64;
    d.stage = PinnedBuf<Fe32>((cap * REC_BYTES + sizeof(Fe32) - 1) / sizeof(Fe32)); d.recs = DevBuf<uint8_t>(cap * REC_BYTES); d.items = DevBuf<uint8_t>(cap * sizeof(VerifyItem));
    d.inputs = DevBuf<uint8_t>(cap * 6 * sizeof(Fe32) + 32); d.parsed = DevBuf<uint8_t>(cap); d.cap = cap;
  }
  return (uint8_t *)d.stage.get();
}
void RecordIngest::run(size_t n, int kind, bool strict) {
  Impl &d = *impl; const size_t ni = record_num_inputs(kind);
  if (!n || n > d.cap || !ni) throw GpuError("record ingest: record count or kind");
  static_assert(sizeof(VerifyItem) == 8 * sizeof(Fq) && sizeof(VerifyItem) == 256, "proof record");
  try {
    { Stage st("verify.upload"); upload_async(d.recs.get(), d.stage.get(), n * REC_BYTES); }
    Stage st("verify.ingest");
    hipLaunchKernelGGL(k_ingest_records, dim3(cdiv(n, ING_RECORDS)), dim3(ING_THREADS), 0, gpu().stream, (const uint4 *)d.recs.get(), (uint32_t)n, (uint32_t)kind,
        (uint32_t)ni, record_words(kind), strict ? 1u : 0u, (Fq *)d.items.get(), (Fr *)d.inputs.get(), d.parsed.get());
    HIP_CHECK(hipGetLastError());
  } catch (...) { (void)hipStreamSynchronize(gpu().stream); throw; }   // (no copy may still be reading the staging area when the next caller fills it)
  d.n = n; d.ni = ni;
}
const void *RecordIngest::items_dev() const { return impl->items.get(); }
const Fe32 *RecordIngest::inputs_dev() const { return (const Fe32 *)impl->inputs.get(); }
const uint8_t *RecordIngest::parsed_dev() const { return impl->parsed.get(); }
void RecordIngest::download(size_t first, size_t count, void *items, Fe32 *inputs, uint8_t *parsed) {
  Impl &d = *impl; if (first + count > d.n) throw GpuError("record ingest: download range"); hipStream_t s = gpu().stream; if (!count) return;
  if (items) HIP_CHECK(hipMemcpyAsync(items, d.items.get() + first * sizeof(VerifyItem), count * sizeof(VerifyItem), hipMemcpyDeviceToHost, s));
  if (inputs) HIP_CHECK(hipMemcpyAsync(inputs, d.inputs.get() + first * d.ni * sizeof(Fe32), count * d.ni * sizeof(Fe32), hipMemcpyDeviceToHost, s));
  if (parsed) HIP_CHECK(hipMemcpyAsync(parsed, d.parsed.get() + first, count, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
}

// ---- k_block_scalar_sums ---------------------------------------------------------------------------------------------------------------------------------------
// The integers s = sum r_i (row 0) and c_j = sum r_i x_ij (row j + 1) over the records flagged 1, exact, seven 64-bit limbs each as rlc_int_sums keeps them
// (groth16_verifier.cpp: 128 + 256 bits a product, fewer than 2^31 records).  Integer addition does not care for the order, so the result is the host loop's bit for
// bit.  blockIdx.y = the row; a lane sums a grid-stride range, a wave folds by cross-lane moves, the workgroup's four waves meet in LDS, and the workgroups'
// results (at most SUM_BLOCKS a row) are folded by one more launch of the same reduction.
constexpr uint32_t SUM_THREADS = 256, SUM_BLOCKS = 64;
struct U448 { uint64_t l[7]; };
__device__ __forceinline__ void add448(U448 &a, const U448 &b) {
  uint64_t carry = 0;
  for (int k = 0; k < 7; k++) { const uint64_t s = a.l[k] + b.l[k], c1 = s < b.l[k], s2 = s + carry, c2 = s2 < s; a.l[k] = s2; carry = c1 | c2; }
}
// the sum over the workgroup, valid in thread 0
__device__ __forceinline__ U448 block_sum448(U448 acc, uint64_t (*sh)[7]) {
  for (int off = 32; off; off >>= 1) { U448 o; for (int k = 0; k < 7; k++) o.l[k] = __shfl_down((unsigned long long)acc.l[k], off, 64); add448(acc, o); }
  const uint32_t wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
  if ((threadIdx.x & 63) == 0) for (int k = 0; k < 7; k++) sh[wave][k] = acc.l[k];
  __syncthreads();
  if (threadIdx.x == 0) for (uint32_t w = 1; w < waves; w++) { U448 o; for (int k = 0; k < 7; k++) o.l[k] = sh[w][k]; add448(acc, o); }
  return acc;
}
static __global__ void __launch_bounds__(SUM_THREADS) k_block_scalar_sums(const Fr *__restrict__ inputs, uint32_t n_inputs, const uint4 *__restrict__ weights,
    const uint8_t *__restrict__ flag, uint32_t n, uint64_t *__restrict__ partials /* rows x gridDim.x x 7 */) {
  __shared__ uint64_t sh[SUM_THREADS / 64][7];
  const uint32_t row = blockIdx.y; U448 acc; for (int k = 0; k < 7; k++) acc.l[k] = 0;
  for (uint32_t i = blockIdx.x * SUM_THREADS + threadIdx.x; i < n; i += gridDim.x * SUM_THREADS) {
    if (flag[i] != 1) continue;
    const uint4 wv = weights[i]; const uint64_t w[2] = {(uint64_t)wv.x | (uint64_t)wv.y << 32, (uint64_t)wv.z | (uint64_t)wv.w << 32};
    U448 p; for (int k = 0; k < 7; k++) p.l[k] = 0;
    if (row == 0) { p.l[0] = w[0]; p.l[1] = w[1]; }
    else {
      const Fr xv = inputs[(size_t)i * n_inputs + row - 1]; uint64_t x[4]; for (int b = 0; b < 4; b++) x[b] = (uint64_t)xv.l[2 * b] | (uint64_t)xv.l[2 * b + 1] << 32;
      for (int a = 0; a < 2; a++) { uint64_t carry = 0;                                     // schoolbook, 2 x 4 limbs: p + lo + carry never leaves 128 bits
        for (int b = 0; b < 4; b++) { const uint64_t lo = w[a] * x[b], hi = __umul64hi(w[a], x[b]), s = p.l[a + b] + lo, c1 = s < lo, s2 = s + carry, c2 = s2 < s;
          p.l[a + b] = s2; carry = hi + c1 + c2; }
        p.l[a + 4] = carry; }
    }
    add448(acc, p);
  }
  acc = block_sum448(acc, sh);
  if (threadIdx.x == 0) for (int k = 0; k < 7; k++) partials[((size_t)row * gridDim.x + blockIdx.x) * 7 + k] = acc.l[k];
}
static __global__ void __launch_bounds__(64) k_block_scalar_sums_fold(const uint64_t *__restrict__ partials, uint32_t nb, uint64_t *__restrict__ out /* rows x 7 */) {
  __shared__ uint64_t sh[1][7];
  const uint32_t row = blockIdx.x; U448 acc; for (int k = 0; k < 7; k++) acc.l[k] = 0;
  for (uint32_t b = threadIdx.x; b < nb; b += 64) { U448 o; for (int k = 0; k < 7; k++) o.l[k] = partials[((size_t)row * nb + b) * 7 + k]; add448(acc, o); }
  acc = block_sum448(acc, sh);
  if (threadIdx.x == 0) for (int k = 0; k < 7; k++) out[row * 7 + k] = acc.l[k];
}
size_t block_scalar_sums_scratch(size_t n_inputs) { return (n_inputs + 1) * SUM_BLOCKS * 7; }
void block_scalar_sums_dev(const Fe32 *inputs, size_t n_inputs, const uint8_t *weights, const uint8_t *flags, size_t n, uint64_t *partials, uint64_t *out) {
  if (!n || n > 0x7fffffffu) throw GpuError("block sums: record count");
  const uint32_t nb = std::min<uint32_t>(cdiv(n, SUM_THREADS), SUM_BLOCKS), rows = (uint32_t)n_inputs + 1; hipStream_t s = gpu().stream;
  hipLaunchKernelGGL(k_block_scalar_sums, dim3(nb, rows), dim3(SUM_THREADS), 0, s, (const Fr *)inputs, (uint32_t)n_inputs, (const uint4 *)weights, flags, (uint32_t)n, partials);
  hipLaunchKernelGGL(k_block_scalar_sums_fold, dim3(rows), dim3(64), 0, s, (const uint64_t *)partials, nb, out);
  HIP_CHECK(hipGetLastError());
}

}  // namespace zk
