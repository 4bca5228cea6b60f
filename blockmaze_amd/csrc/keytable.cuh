// The keyed table under the spent set (gpu_snset.hip) and the account table (gpu_accounts.hip): an append-only log of entries that begin with a 20-byte key, and an
// index over it.  State m is the first m log entries.
// Layout: the log holds a fixed number of 32-bit words an entry (the key is the first five) and doubles through copy_dev_async.  The index is an open-addressing
// table of 32-bit slots, a power of two of them, linear probing: a slot holds 0 (empty), 0xFFFFFFFF (a tombstone: an entry that a rewind removed) or log index + 1.
// The home slot of a key is kt_home() below.  During one call a slot may also hold a TENTATIVE value n_old + 1 + j: record j of the batch has claimed it; its key
// lies in the uploaded batch.
// Rules every kernel keeps (DESIGN.md "Spent serial numbers" has the arguments):
//   - no lane waits for another lane, wave or workgroup, and every probe loop ends after `slots` steps at the latest (running out sets the call's error word);
//   - inside one launch the only words one workgroup writes and another reads are table slots (and the account table's heads): read by agent-scope relaxed atomic
//     loads, written by atomicCAS / atomicMin / atomicMax / atomicExch / an atomic store, and "empty" is never acted on from a load — a slot is claimed by CAS alone;
//   - key bytes, in the log or in the batch, and every other plain store are read only in launches after the one that wrote them;
//   - an insert goes into an empty slot only, never into a tombstone, so a slot that is not empty stays so for the whole launch.
// Everything runs in order on the library's main stream (lane 0) under the device mutex, each entry of a table under that table's own mutex (taken first).
#pragma once
#include <sys/random.h>
#include <mutex>
#include <string>
#include <vector>
#include "gpu_internal.hpp"

extern std::mutex g_gpu_mutex;

namespace zk {

constexpr uint32_t KT_TOMB = 0xFFFFFFFFu, KT_NONE = 0xFFFFFFFFu;   // a slot's tombstone; "this record probed nothing" in a per-record slot array
constexpr int KT_THREADS = 256, KEY_WORDS = 5;
constexpr uint32_t KT_MIN_SLOTS_LOG = 10, KT_MAX_SLOTS_LOG = 31;
constexpr uint64_t KT_MAX_LOG = 0xFFFFFFFEull;                     // the log never reaches 2^32 - 2 entries: n_old + 1 + j stays below the tombstone

struct Key20 { uint32_t w[KEY_WORDS]; };
struct KeyTable { uint32_t *slots; uint32_t mask; uint64_t seed; };
// The mix (restated by include/zkgpu.h and by the tests): w0..w4 are the key's bytes as five little-endian 32-bit words; in 64-bit arithmetic
//   h = seed;  for k = 0..4: h = (h ^ w_k) * 0x9E3779B97F4A7C15, h ^= h >> 32;  h = h * 0xD6E8FEB86659FD93, h ^= h >> 32;  home = h & (slots - 1)
__device__ __forceinline__ uint32_t kt_home(const Key20 &k, const KeyTable &T) {
  uint64_t h = T.seed;
#pragma unroll
  for (int i = 0; i < KEY_WORDS; i++) { h = (h ^ (uint64_t)k.w[i]) * 0x9E3779B97F4A7C15ull; h ^= h >> 32; }
  h *= 0xD6E8FEB86659FD93ull; h ^= h >> 32;
  return (uint32_t)h & T.mask;
}
__device__ __forceinline__ Key20 key_load(const uint32_t *p) { Key20 k;
#pragma unroll
  for (int i = 0; i < KEY_WORDS; i++) k.w[i] = p[i];
  return k; }
__device__ __forceinline__ void key_store(uint32_t *p, const Key20 &k) {
#pragma unroll
  for (int i = 0; i < KEY_WORDS; i++) p[i] = k.w[i]; }
__device__ __forceinline__ bool key_equal(const Key20 &a, const Key20 &b) { uint32_t d = 0;
#pragma unroll
  for (int i = 0; i < KEY_WORDS; i++) d |= a.w[i] ^ b.w[i];
  return d == 0; }
__device__ __forceinline__ uint32_t slot_load(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void slot_store(uint32_t *p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The find-or-claim walk of record i of a batch of n keys (5 words each, at `keys`) on a table whose log holds n_old entries of STRIDE words: the slot the record
// ends at, or KT_NONE where the probe went round the table or met a value that is neither the table's nor the call's.  The lane walks the chain from its home slot:
// a resident value (<= n_old) is compared with the log, a tentative one with the batch; on its own key it stops — LOWER: lowering a tentative value to its own
// n_old + 1 + i if that is smaller, so the slot ends at the lowest of its claimants —; on empty it claims the slot by CAS and, if the CAS fails, looks at what the
// CAS returned — which is not empty, so a slot is looked at twice at most.  All records of one key end at one slot: every lane sees the same final value of every
// slot on its way.
template <int STRIDE, bool LOWER>
__device__ __forceinline__ uint32_t kt_find_or_claim(const KeyTable &T, const uint32_t *__restrict__ log, uint32_t n_old, const uint32_t *__restrict__ keys, uint32_t n, uint32_t i) {
  const Key20 k = key_load(keys + KEY_WORDS * (size_t)i); const uint32_t mine = n_old + 1 + i; uint32_t s = kt_home(k, T);
  for (uint32_t step = 0; step <= T.mask; step++, s = (s + 1) & T.mask) {
    uint32_t v = slot_load(T.slots + s);
    if (v == 0) { v = atomicCAS(T.slots + s, 0u, mine); if (v == 0) return s; }
    if (v == KT_TOMB) continue;
    if (v > n_old && v - n_old - 1 >= n) break;                                                     // no value of this call or of the table: the table is damaged
    const Key20 o = key_load(v <= n_old ? log + STRIDE * (size_t)(v - 1) : keys + KEY_WORDS * (size_t)(v - n_old - 1));
    if (key_equal(k, o)) { if (LOWER && v > mine) atomicMin(T.slots + s, mine); return s; }
  }
  return KT_NONE;
}

// Ranks in record order over a grid of KT_THREADS-wide workgroups, each of which has left its number of flagged items in counts[blockIdx.x] in an earlier launch.
// kt_ranks_before: the items of the earlier workgroups (LDS word `before`; two barriers).  kt_rank_step: a lane flags up to two items, a0 before a1; returned is the
// number of flagged items of the workgroup's lower lanes (ballot and popcount a wave, LDS across the waves; one barrier), `all` the workgroup's total.  Neither has
// an early exit: every lane of the workgroup calls them, and puts a barrier between two steps (wave_sum is written again).
__device__ __forceinline__ uint32_t kt_ranks_before(uint32_t *before, const uint32_t *__restrict__ counts) {
  if (threadIdx.x == 0) *before = 0;
  __syncthreads();
  uint32_t part = 0; for (uint32_t t = threadIdx.x; t < blockIdx.x; t += KT_THREADS) part += counts[t];
  if (part) atomicAdd(before, part);
  __syncthreads();
  return *before;
}
__device__ __forceinline__ uint32_t kt_rank_step(bool a0, bool a1, uint32_t *wave_sum, uint32_t &all) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6; const unsigned long long b0 = __ballot(a0), b1 = __ballot(a1), below = (1ull << lane) - 1;
  if (lane == 0) wave_sum[wave] = (uint32_t)(__popcll(b0) + __popcll(b1));
  __syncthreads();
  uint32_t rank = (uint32_t)(__popcll(b0 & below) + __popcll(b1 & below)); all = 0;
#pragma unroll
  for (uint32_t w = 0; w < KT_THREADS / 64; w++) { const uint32_t c = wave_sum[w]; if (w < wave) rank += c; all += c; }
  return rank;
}

// ---- the host side: what SpentSet::Impl and AccountTable::Impl share.  `name` begins every message ("spent set", "account table"); `stride` is the log's words an
// entry.  The pinned staging carries the gathered batch on the way up and the answer on the way down.
struct LogTableState : PinnedStage {
  const char *const name; const size_t stride;
  std::mutex mu; uint64_t n = 0, tombs = 0, seed = 0, cap = 0; uint32_t slots_log = 0, min_log = KT_MIN_SLOTS_LOG; bool damaged = false;
  DevBuf<uint32_t> log, slots, work /* a call's arrays, kept and grown */;
  LogTableState(const char *name_, size_t stride_, int log2_slots, const uint64_t *seed_) : name(name_), stride(stride_) {   // (no HIP call: the owner allocates the slots)
    if (log2_slots && (log2_slots < 4 || log2_slots > (int)KT_MAX_SLOTS_LOG)) throw GpuError(std::string(name) + ": a table has 2^4 to 2^31 slots");
    if (seed_) seed = *seed_; else if (getrandom(&seed, 8, 0) != 8) throw GpuError(std::string(name) + ": getrandom gave no seed");
    min_log = slots_log = log2_slots ? (uint32_t)log2_slots : KT_MIN_SLOTS_LOG;
  }
  KeyTable handle(uint32_t *s, uint32_t lg) const { return KeyTable{s, (uint32_t)((1ull << lg) - 1), seed}; }
  // A call that writes the table marks it damaged until it has come through: whatever ends it early — a HIP error, an error word — leaves a table that may hold
  // tentative values or entries beyond n, and the table is made anew from the log before its next use (slots_log_for, the owner's repair).
  struct Writing { bool &flag; explicit Writing(bool &f) : flag(f) { flag = true; } void done() { flag = false; } };
  // slots for `incoming` more entries: live entries + tombstones + the batch at or below half of the table (the account table's addresses take one slot however many
  // entries they have, so its load factor stays at or below one half too); otherwise (or after damage) the smallest sufficient table
  uint32_t slots_log_for(uint64_t incoming) const {
    if (!damaged && 2 * (n + tombs + incoming) <= (1ull << slots_log)) return 0;
    uint32_t lg = min_log; while ((1ull << lg) < 2 * (n + incoming)) lg++;
    if (lg > KT_MAX_SLOTS_LOG) throw GpuError(std::string(name) + ": the table would need more than 2^31 slots");
    return lg;
  }
  void adopt_slots(DevBuf<uint32_t> &fresh, uint32_t lg) { slots = std::move(fresh); slots_log = lg; tombs = 0; damaged = false; }   // a rebuilt table becomes the table's own
  void reserve_log(uint64_t entries) {
    if (entries <= cap) return;
    uint64_t c = std::max<uint64_t>(cap, 1024); while (c < entries) c *= 2;
    DevBuf<uint32_t> fresh(stride * (size_t)c); if (n) copy_dev_async(fresh.get(), log.get(), 4 * stride * (size_t)n);
    HIP_CHECK(hipGetLastError()); HIP_CHECK(hipStreamSynchronize(gpu().stream));                  // (the old allocation is let go below)
    log = std::move(fresh); cap = c;
  }
  bool read_log(uint64_t first, uint64_t count, uint8_t *out) {
    std::lock_guard<std::mutex> lk(mu);
    if (first > n || count > n - first || (count && !out)) return false;
    if (!count) return true;
    LaneScope lane(0); std::lock_guard<std::mutex> gl(g_gpu_mutex); hipStream_t s = gpu().stream; SyncAtExit sync;
    HIP_CHECK(hipMemcpyAsync(out, log.get() + stride * (size_t)first, 4 * stride * (size_t)count, hipMemcpyDeviceToHost, s)); HIP_CHECK(hipStreamSynchronize(s));
    return true;
  }
  void read_slots(std::vector<uint32_t> &out, uint64_t &seed_out, uint64_t &tombstones) {
    std::lock_guard<std::mutex> lk(mu); LaneScope lane(0); std::lock_guard<std::mutex> gl(g_gpu_mutex);
    out.resize((size_t)1 << slots_log); slots.download(out.data(), out.size()); seed_out = seed; tombstones = tombs;
  }
};

}  // namespace zk
