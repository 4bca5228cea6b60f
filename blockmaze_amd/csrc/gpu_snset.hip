// The set of spent serial numbers resident in HBM (DESIGN.md "Spent serial numbers"; include/zk_spent.h): what core/state_processor.go:106-163 keeps in the state
// trie — statedb.Exist(BytesToAddress(sn)), "sn is already used", CreateAccount — as an append-only log of distinct 20-byte keys in insertion order and an index over it.
// State m is the first m log entries.
// Layout: the log holds 5 words an entry and doubles through copy_dev_async.  The index is an open-addressing table of 32-bit slots, a power of two of them, linear
// probing: a slot holds 0 (empty), 0xFFFFFFFF (a tombstone: an entry that a rewind removed) or log index + 1.  The home slot of a key is snset_home() below.
// During one spend call a slot may also hold a TENTATIVE value n_old + 1 + j: record j of the batch has claimed it; its key lies in the uploaded batch.
// Rules every kernel keeps (DESIGN.md has the arguments):
//   - no lane waits for another lane, wave or workgroup, and every probe loop ends after `slots` steps at the latest (running out sets the error word);
//   - inside one launch the only words one workgroup writes and another reads are table slots: read by agent-scope relaxed atomic loads, written by atomicCAS /
//     atomicMin / an atomic store, and "empty" is never acted on from a load — a slot is claimed by CAS alone;
//   - key bytes, in the log or in the batch, are read only in launches after the one that wrote them;
//   - an insert goes into an empty slot only, never into a tombstone, so a slot that is not empty stays so for the whole launch.
// Everything runs in order on the library's main stream (lane 0) under the device mutex, each entry of a set under that set's own mutex (taken first).
#include <sys/random.h>
#include <algorithm>
#include <atomic>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>
#include "gpu_internal.hpp"

extern std::mutex g_gpu_mutex;

namespace zk {

constexpr uint32_t SN_TOMB = 0xFFFFFFFFu, SN_NONE = 0xFFFFFFFFu;   // a slot's tombstone; "this record probed nothing" in the per-record slot array
constexpr int SN_THREADS = 256, SN_WORDS = 5;
constexpr uint32_t SN_MIN_SLOTS_LOG = 10, SN_MAX_SLOTS_LOG = 31, SN_MAX_TILES = 1024;
constexpr uint64_t SN_MAX_LOG = 0xFFFFFFFEull;                     // the log never reaches 2^32 - 2 entries: n_old + 1 + j stays below the tombstone
constexpr uint32_t SN_ROUND_CAP = 8;                               // spend_pairs: rounds on the device before the host finishes the live records.  A bound on what an adversary can cost a call, not a tuned number

struct SnKey { uint32_t w[SN_WORDS]; };
struct SnTable { uint32_t *slots; uint32_t mask; uint64_t seed; };
// The mix (restated by include/zkgpu.h and by the tests): w0..w4 are the key's bytes as five little-endian 32-bit words; in 64-bit arithmetic
//   h = seed;  for k = 0..4: h = (h ^ w_k) * 0x9E3779B97F4A7C15, h ^= h >> 32;  h = h * 0xD6E8FEB86659FD93, h ^= h >> 32;  home = h & (slots - 1)
__device__ __forceinline__ uint32_t snset_home(const SnKey &k, const SnTable &T) {
  uint64_t h = T.seed;
#pragma unroll
  for (int i = 0; i < SN_WORDS; i++) { h = (h ^ (uint64_t)k.w[i]) * 0x9E3779B97F4A7C15ull; h ^= h >> 32; }
  h *= 0xD6E8FEB86659FD93ull; h ^= h >> 32;
  return (uint32_t)h & T.mask;
}
__device__ __forceinline__ SnKey sn_load(const uint32_t *p) { SnKey k;
#pragma unroll
  for (int i = 0; i < SN_WORDS; i++) k.w[i] = p[i];
  return k; }
__device__ __forceinline__ bool sn_equal(const SnKey &a, const SnKey &b) { uint32_t d = 0;
#pragma unroll
  for (int i = 0; i < SN_WORDS; i++) d |= a.w[i] ^ b.w[i];
  return d == 0; }
__device__ __forceinline__ uint32_t slot_load(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void slot_store(uint32_t *p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// One lane per record of the batch; where[i] = the slot record i ended at, SN_NONE for a record that is masked out or exempt (active[i] = 0).  A lane walks the chain
// from its home slot: a resident value (<= n_old) is compared with the log, a tentative one with the batch; on its own key it stops (lowering a tentative value to its
// own record number if that is smaller); on empty it claims the slot by CAS and, if the CAS fails, looks at what the CAS returned — which is not empty, so a slot is
// looked at twice at most.
__global__ void __launch_bounds__(SN_THREADS) k_snset_probe(SnTable T, const uint32_t *__restrict__ log, uint32_t n_old, const uint32_t *__restrict__ keys,
                                                             const uint8_t *__restrict__ active, uint32_t n, uint32_t *__restrict__ where, uint32_t *__restrict__ err) {
  const uint32_t i = blockIdx.x * SN_THREADS + threadIdx.x; if (i >= n) return;
  if (!active[i]) { where[i] = SN_NONE; return; }
  const SnKey k = sn_load(keys + SN_WORDS * (size_t)i); const uint32_t mine = n_old + 1 + i; uint32_t s = snset_home(k, T), at = SN_NONE;
  for (uint32_t step = 0; step <= T.mask; step++, s = (s + 1) & T.mask) {
    uint32_t v = slot_load(T.slots + s);
    if (v == 0) { v = atomicCAS(T.slots + s, 0u, mine); if (v == 0) { at = s; break; } }
    if (v == SN_TOMB) continue;
    if (v > n_old && v - n_old - 1 >= n) break;                                                   // no value of this call or of the set: the table is damaged
    const SnKey o = sn_load(v <= n_old ? log + SN_WORDS * (size_t)(v - 1) : keys + SN_WORDS * (size_t)(v - n_old - 1));
    if (sn_equal(k, o)) { if (v > mine) atomicMin(T.slots + s, mine); at = s; break; }
  }
  if (at == SN_NONE) *err = 1;
  where[i] = at;
}
// A later launch: every record reads its slot's final value.  Workgroup b takes the records [b, b + 1) * per * SN_THREADS and leaves its number of winners in counts[b].
__global__ void __launch_bounds__(SN_THREADS) k_snset_classify(const uint32_t *__restrict__ slots, const uint32_t *__restrict__ where, uint32_t n, uint32_t n_old, uint32_t per,
                                                                uint8_t *__restrict__ conflict, uint8_t *__restrict__ winner, uint32_t *__restrict__ counts) {
  __shared__ uint32_t total; if (threadIdx.x == 0) total = 0;
  __syncthreads();
  uint32_t mine = 0;
  for (uint32_t it = 0; it < per; it++) {
    const uint64_t i = ((uint64_t)blockIdx.x * per + it) * SN_THREADS + threadIdx.x; if (i >= n) break;
    const uint32_t w = where[i]; uint8_t c = 0, win = 0;
    if (w != SN_NONE) { const uint32_t v = slot_load(slots + w); if (v <= n_old) c = 1; else if (v == n_old + 1 + (uint32_t)i) win = 1; else c = 2; }
    conflict[i] = c; winner[i] = win; mine += win;
  }
  if (mine) atomicAdd(&total, mine);
  __syncthreads();
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}
// A later launch again, for the winners: rank = winners of the earlier workgroups + rank inside the workgroup (ballot and popcount a wave, LDS across the waves), so
// committed keys enter the log in record order.  commit: the key goes to log[n_old + rank] and the slot gets n_old + rank + 1; otherwise the slot is emptied, and as
// every tentative slot has exactly one winner the table is what it was before the call.  The last workgroup leaves the number of winners in n_won.
__global__ void __launch_bounds__(SN_THREADS) k_snset_finalize(uint32_t *__restrict__ slots, uint32_t *__restrict__ log, const uint32_t *__restrict__ where, const uint8_t *__restrict__ winner,
                                                                const uint32_t *__restrict__ keys, uint32_t n, uint32_t n_old, uint32_t per, const uint32_t *__restrict__ counts, int commit,
                                                                uint32_t *__restrict__ n_won) {
  __shared__ uint32_t before, wave_sum[SN_THREADS / 64];
  if (threadIdx.x == 0) before = 0;
  __syncthreads();
  uint32_t part = 0; for (uint32_t t = threadIdx.x; t < blockIdx.x; t += SN_THREADS) part += counts[t];
  if (part) atomicAdd(&before, part);
  __syncthreads();
  uint32_t running = before; const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (uint32_t it = 0; it < per; it++) {                                                          // (uniform: every lane of the workgroup takes every barrier)
    const uint64_t i = ((uint64_t)blockIdx.x * per + it) * SN_THREADS + threadIdx.x; const bool win = i < n && winner[i];
    const unsigned long long b = __ballot(win);
    if (lane == 0) wave_sum[wave] = (uint32_t)__popcll(b);
    __syncthreads();
    uint32_t rank = running + (uint32_t)__popcll(b & ((1ull << lane) - 1)), all = 0;
#pragma unroll
    for (uint32_t w = 0; w < SN_THREADS / 64; w++) { const uint32_t c = wave_sum[w]; if (w < wave) rank += c; all += c; }
    if (win) {
      const uint32_t s = where[i];
      if (commit) { const SnKey k = sn_load(keys + SN_WORDS * i); uint32_t *dst = log + SN_WORDS * (size_t)(n_old + rank);
#pragma unroll
        for (int j = 0; j < SN_WORDS; j++) dst[j] = k.w[j];
        slot_store(slots + s, n_old + rank + 1); }
      else slot_store(slots + s, 0u);
    }
    running += all;
    __syncthreads();
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) *n_won = running;
}
// a fresh table from the log: one lane per live entry; the keys are distinct, so CAS into empty is all there is
__global__ void __launch_bounds__(SN_THREADS) k_snset_rebuild(SnTable T, const uint32_t *__restrict__ log, uint32_t n_live, uint32_t *__restrict__ err) {
  const uint32_t i = blockIdx.x * SN_THREADS + threadIdx.x; if (i >= n_live) return;
  uint32_t s = snset_home(sn_load(log + SN_WORDS * (size_t)i), T); bool done = false;
  for (uint32_t step = 0; step <= T.mask && !done; step++, s = (s + 1) & T.mask) done = atomicCAS(T.slots + s, 0u, i + 1) == 0;
  if (!done) *err = 2;
}
// rewind from n to m: one lane per entry m .. n - 1 walks to the slot that holds its own index + 1 and leaves the tombstone there
__global__ void __launch_bounds__(SN_THREADS) k_snset_unlink(SnTable T, const uint32_t *__restrict__ log, uint32_t m, uint32_t n, uint32_t *__restrict__ err) {
  const uint32_t i = m + blockIdx.x * SN_THREADS + threadIdx.x; if (i >= n) return;
  uint32_t s = snset_home(sn_load(log + SN_WORDS * (size_t)i), T); bool done = false;
  for (uint32_t step = 0; step <= T.mask; step++, s = (s + 1) & T.mask) {
    const uint32_t v = slot_load(T.slots + s);
    if (v == i + 1) { slot_store(T.slots + s, SN_TOMB); done = true; break; }
    if (v == 0) break;
  }
  if (!done) *err = 3;
}
// read-only: index[t] = the position of key t in the log if it is below `size`, else 2^64 - 1.  An entry at `size` or beyond does not match and the walk goes on.
__global__ void __launch_bounds__(SN_THREADS) k_snset_query(SnTable T, const uint32_t *__restrict__ log, uint32_t size, const uint32_t *__restrict__ keys, uint32_t q,
                                                             unsigned long long *__restrict__ index) {
  const uint32_t t = blockIdx.x * SN_THREADS + threadIdx.x; if (t >= q) return;
  const SnKey k = sn_load(keys + SN_WORDS * (size_t)t); uint32_t s = snset_home(k, T); unsigned long long found = ~0ull;
  for (uint32_t step = 0; step <= T.mask; step++, s = (s + 1) & T.mask) {
    const uint32_t v = slot_load(T.slots + s);
    if (v == 0) break;
    if (v == SN_TOMB || v - 1 >= size) continue;
    if (sn_equal(k, sn_load(log + SN_WORDS * (size_t)(v - 1)))) { found = v - 1; break; }
  }
  index[t] = found;
}

// ---- two keys a record (DESIGN.md "Two keys a record"; SpentSet::spend_pairs) -----------------------------------------------------------------------------------
// Entry e = 2 i + j is key j of record i, its tentative slot value n_old + 1 + e; active[e] = 0 for a key that is not there or is the exempt first key.  A record is
// live, accepted or rejected (status[i]); code[i] is its conflict code.  A round is the three launches probe, wins, decide; the fourth, finish, either releases the
// round's slots (records are still live) or finalises the call.  Each launch reads only table slots and flags that earlier launches wrote.
constexpr uint8_t SP_LIVE = 0, SP_ACCEPTED = 1, SP_REJECTED = 2;
constexpr uint32_t SP_ERR = 0, SP_LIVE_N = 1, SP_WON = 2, SP_TOMBS = 3, SP_HEAD = 4;              // the call's head words: error, live records, keys committed, tombstones left
// k_snset_probe with one lane per entry of every record that is not rejected: afterwards a slot holds the lowest entry among those claimants
__global__ void __launch_bounds__(SN_THREADS) k_snset_pairs_probe(SnTable T, const uint32_t *__restrict__ log, uint32_t n_old, const uint32_t *__restrict__ keys,
                                                                   const uint8_t *__restrict__ active, const uint8_t *__restrict__ status, uint32_t n2, uint32_t *__restrict__ where,
                                                                   uint32_t *__restrict__ head) {
  const uint32_t e = blockIdx.x * SN_THREADS + threadIdx.x; if (e >= n2) return;
  if (!active[e] || status[e >> 1] == SP_REJECTED) { where[e] = SN_NONE; return; }
  const SnKey k = sn_load(keys + SN_WORDS * (size_t)e); const uint32_t mine = n_old + 1 + e; uint32_t s = snset_home(k, T), at = SN_NONE;
  for (uint32_t step = 0; step <= T.mask; step++, s = (s + 1) & T.mask) {
    uint32_t v = slot_load(T.slots + s);
    if (v == 0) { v = atomicCAS(T.slots + s, 0u, mine); if (v == 0) { at = s; break; } }
    if (v == SN_TOMB) continue;
    if (v > n_old && v - n_old - 1 >= n2) break;                                                  // no value of this call or of the set: the table is damaged
    const SnKey o = sn_load(v <= n_old ? log + SN_WORDS * (size_t)(v - 1) : keys + SN_WORDS * (size_t)(v - n_old - 1));
    if (sn_equal(k, o)) { if (v > mine) atomicMin(T.slots + s, mine); at = s; break; }
  }
  if (at == SN_NONE) head[SP_ERR] = 1;
  where[e] = at;
}
// A later launch, one lane per record that is not rejected: hold[e] = entry e holds its slot.  A live record with a key that was in the set before the call is
// rejected with code 1; one that holds every slot of its own has won and is accepted for good — its lower-indexed competitors can only leave.  win[i] = record i is
// accepted; counts[b] = the entries of the accepted records of workgroup b's tile, for finish's ranks.  Lane 0 zeroes the live count that decide adds to.
__global__ void __launch_bounds__(SN_THREADS) k_snset_pairs_wins(const uint32_t *__restrict__ slots, const uint32_t *__restrict__ where, const uint8_t *__restrict__ active, uint32_t n,
                                                                  uint32_t n_old, uint32_t per, uint8_t *__restrict__ status, uint8_t *__restrict__ code, uint8_t *__restrict__ win,
                                                                  uint8_t *__restrict__ hold, uint32_t *__restrict__ counts, uint32_t *__restrict__ head) {
  __shared__ uint32_t total; if (threadIdx.x == 0) { total = 0; if (blockIdx.x == 0) head[SP_LIVE_N] = 0; }
  __syncthreads();
  uint32_t mine = 0;
  for (uint32_t it = 0; it < per; it++) {
    const uint64_t i = ((uint64_t)blockIdx.x * per + it) * SN_THREADS + threadIdx.x; if (i >= n) break;
    uint8_t st = status[i]; uint32_t held = 0; bool all = true, resident = false;
#pragma unroll
    for (uint32_t j = 0; j < 2; j++) {
      const uint64_t e = 2 * i + j; uint8_t h = 0;
      if (st != SP_REJECTED && active[e]) {
        const uint32_t w = where[e], v = w == SN_NONE ? 0u : slot_load(slots + w);
        if (w != SN_NONE && v <= n_old) resident = true;
        h = w != SN_NONE && v == n_old + 1 + (uint32_t)e; held += h; all = all && h;
      }
      hold[e] = h;
    }
    if (st == SP_LIVE) { if (resident) { st = SP_REJECTED; code[i] = 1; } else if (all) st = SP_ACCEPTED; status[i] = st; }
    else if (st == SP_ACCEPTED && !all) head[SP_ERR] = 4;
    const uint8_t w = st == SP_ACCEPTED; win[i] = w; if (w) mine += held;
  }
  if (mine) atomicAdd(&total, mine);
  __syncthreads();
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}
// A later launch again, as it reads the win flags of other workgroups' records: a live record that lost a slot to an accepted record, or to its own other entry, is
// rejected with code 2; one that lost only to records that did not win stays live, and is counted.
__global__ void __launch_bounds__(SN_THREADS) k_snset_pairs_decide(const uint32_t *__restrict__ slots, const uint32_t *__restrict__ where, const uint8_t *__restrict__ active,
                                                                    const uint8_t *__restrict__ hold, const uint8_t *__restrict__ win, uint32_t n, uint32_t n_old,
                                                                    uint8_t *__restrict__ status, uint8_t *__restrict__ code, uint32_t *__restrict__ head) {
  const uint32_t i = blockIdx.x * SN_THREADS + threadIdx.x; bool live = false;
  if (i < n && status[i] == SP_LIVE) {
    bool lost = false;
#pragma unroll
    for (uint32_t j = 0; j < 2; j++) {
      const uint64_t e = 2 * (uint64_t)i + j; if (!active[e] || hold[e]) continue;
      const uint32_t w = where[e]; if (w == SN_NONE) continue;                                     // (the probe has set the error word)
      const uint32_t v = slot_load(slots + w), h = v - n_old - 1;
      if (v <= n_old || h >= 2 * (uint64_t)n) { head[SP_ERR] = 4; continue; }
      if ((h >> 1) == i || win[h >> 1]) lost = true;
    }
    if (lost) { status[i] = SP_REJECTED; code[i] = 2; } else live = true;
  }
  const unsigned long long b = __ballot(live);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(head + SP_LIVE_N, (uint32_t)__popcll(b));
}
// The last launch of a round.  Records are still live: every holder empties its slot, and the table is what it was before the call.  None is: k_snset_finalize over
// entries — the rank of an accepted record's entry = the accepted entries before it (counts of the earlier workgroups, ballot and popcount inside this one), so the
// log receives the accepted records' keys in record order, k1 before k2.  A slot held by a rejected record is emptied without commit; with commit it becomes a
// tombstone (emptied, it could cut the chain of a key that went past it) and is counted.
__global__ void __launch_bounds__(SN_THREADS) k_snset_pairs_finish(uint32_t *__restrict__ slots, uint32_t *__restrict__ log, const uint32_t *__restrict__ where, const uint8_t *__restrict__ active,
                                                                    const uint8_t *__restrict__ hold, const uint8_t *__restrict__ win, const uint32_t *__restrict__ keys, uint32_t n,
                                                                    uint32_t n_old, uint32_t per, const uint32_t *__restrict__ counts, int commit, uint32_t *__restrict__ head) {
  __shared__ uint32_t before, wave_sum[SN_THREADS / 64];
  if (head[SP_LIVE_N]) {                                                                           // (uniform over the grid: decide, an earlier launch, wrote it)
    for (uint32_t it = 0; it < per; it++) {
      const uint64_t i = ((uint64_t)blockIdx.x * per + it) * SN_THREADS + threadIdx.x; if (i >= n) break;
#pragma unroll
      for (uint32_t j = 0; j < 2; j++) if (hold[2 * i + j]) slot_store(slots + where[2 * i + j], 0u);
    }
    return;
  }
  if (threadIdx.x == 0) before = 0;
  __syncthreads();
  uint32_t part = 0, tombs = 0; for (uint32_t t = threadIdx.x; t < blockIdx.x; t += SN_THREADS) part += counts[t];
  if (part) atomicAdd(&before, part);
  __syncthreads();
  uint32_t running = before; const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (uint32_t it = 0; it < per; it++) {                                                          // (uniform: every lane of the workgroup takes every barrier)
    const uint64_t i = ((uint64_t)blockIdx.x * per + it) * SN_THREADS + threadIdx.x; const bool won = i < n && win[i];
    const bool a0 = won && hold[2 * i], a1 = won && hold[2 * i + 1];
    const unsigned long long b0 = __ballot(a0), b1 = __ballot(a1), below = (1ull << lane) - 1;
    if (lane == 0) wave_sum[wave] = (uint32_t)(__popcll(b0) + __popcll(b1));
    __syncthreads();
    uint32_t rank = running + (uint32_t)(__popcll(b0 & below) + __popcll(b1 & below)), all = 0;
#pragma unroll
    for (uint32_t w = 0; w < SN_THREADS / 64; w++) { const uint32_t c = wave_sum[w]; if (w < wave) rank += c; all += c; }
    if (i < n) {
#pragma unroll
      for (uint32_t j = 0; j < 2; j++) {
        const uint64_t e = 2 * i + j; if (!hold[e]) continue;
        const uint32_t s = where[e];
        if (won && commit) { const SnKey k = sn_load(keys + SN_WORDS * e); uint32_t *dst = log + SN_WORDS * (size_t)(n_old + rank);
#pragma unroll
          for (int c = 0; c < SN_WORDS; c++) dst[c] = k.w[c];
          slot_store(slots + s, n_old + rank + 1); rank++; }
        else if (commit) { slot_store(slots + s, SN_TOMB); tombs++; }
        else slot_store(slots + s, 0u);
      }
    }
    running += all;
    __syncthreads();
  }
  if (tombs) atomicAdd(head + SP_TOMBS, tombs);
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) head[SP_WON] = running;
}

static std::atomic<uint64_t> g_snset_launches{0}, g_snset_rounds{0}, g_snset_host_finishes{0};
uint64_t SpentSet::launches() { return g_snset_launches.load(); }
void SpentSet::rounds(uint64_t &rounds, uint64_t &host_finishes) { rounds = g_snset_rounds.load(); host_finishes = g_snset_host_finishes.load(); }

struct SpentSet::Impl {
  std::mutex mu; uint64_t n = 0, tombs = 0, seed = 0, cap = 0; uint32_t slots_log = 0, min_log = SN_MIN_SLOTS_LOG, round_cap = SN_ROUND_CAP; bool has_exempt = false, damaged = false; uint8_t exempt[20];
  DevBuf<uint32_t> log, slots, err /* one word for rebuild and rewind outside a spend call, zero between calls */, work /* a call's arrays, kept and grown */;
  uint8_t *pin = nullptr; size_t pin_bytes = 0;                     // pinned staging: the gathered batch on the way up, the answer on the way down
  ~Impl() { if (pin) (void)hipHostFree(pin); }
  struct SyncAtExit { ~SyncAtExit() { (void)hipStreamSynchronize(gpu().stream); } };   // nothing reads pinned or caller memory once an entry has returned or thrown
  void pinned(size_t bytes) { if (pin_bytes >= bytes) return; if (pin) { (void)hipHostFree(pin); pin = nullptr; pin_bytes = 0; }
    HIP_CHECK(hipHostMalloc((void **)&pin, 2 * bytes)); pin_bytes = 2 * bytes; }
  static void grow(DevBuf<uint32_t> &b, size_t words) { if (b.size() < words) b = DevBuf<uint32_t>(std::max(words, 2 * b.size())); }
  SnTable table(uint32_t *s, uint32_t lg) const { return SnTable{s, (uint32_t)((1ull << lg) - 1), seed}; }
  SnTable table() const { return table(slots.get(), slots_log); }
  static void launched() { g_snset_launches.fetch_add(1); }
  // A call that writes the set's own table marks it damaged until it has come through: whatever ends it early — a HIP error, an error word — leaves a table that may
  // hold tentative values or entries beyond n, and the table is made anew from the log before its next use (slots_log_for, repair).
  struct Writing { bool &flag; explicit Writing(bool &f) : flag(f) { flag = true; } void done() { flag = false; } };
  // An error word read after a synchronise.  No load factor at or below one half produces one.
  void check_err(uint32_t e, const char *what, bool own_word) {
    if (!e) return;
    if (own_word) { (void)hipMemsetAsync(err.get(), 0, 4, gpu().stream); (void)hipStreamSynchronize(gpu().stream); }
    throw GpuError(std::string("spent set: ") + what + (e == 1 ? ": a probe went round the whole table" : e == 2 ? ": no empty slot while rebuilding" : e == 4 ? ": a slot holds no value of this call" : ": an entry of the log is not in the table"));
  }
  // slots for `incoming` more keys: live entries + tombstones + the batch at or below half of the table; otherwise (or after damage) the smallest sufficient table
  uint32_t slots_log_for(uint64_t incoming) const {
    if (!damaged && 2 * (n + tombs + incoming) <= (1ull << slots_log)) return 0;
    uint32_t lg = min_log; while ((1ull << lg) < 2 * (n + incoming)) lg++;
    if (lg > SN_MAX_SLOTS_LOG) throw GpuError("spent set: the table would need more than 2^31 slots");
    return lg;
  }
  DevBuf<uint32_t> rebuilt(uint32_t lg, uint32_t *err_word) {        // one memset and one launch on the main stream, not synchronised
    DevBuf<uint32_t> fresh((size_t)1 << lg); hipStream_t s = gpu().stream; HIP_CHECK(hipMemsetAsync(fresh.get(), 0, 4ull << lg, s));
    if (n) { hipLaunchKernelGGL(k_snset_rebuild, dim3(cdiv(n, SN_THREADS)), dim3(SN_THREADS), 0, s, table(fresh.get(), lg), (const uint32_t *)log.get(), (uint32_t)n, err_word); launched(); HIP_CHECK(hipGetLastError()); }
    return fresh;
  }
  uint32_t own_err() { uint32_t e = 0; HIP_CHECK(hipMemcpyAsync(&e, err.get(), 4, hipMemcpyDeviceToHost, gpu().stream)); HIP_CHECK(hipStreamSynchronize(gpu().stream)); return e; }
  void repair() {                                                     // query and rewind read the set's own table: after damage it is made anew first
    if (!damaged) return;
    const uint32_t lg = slots_log_for(0); DevBuf<uint32_t> fresh = rebuilt(lg, err.get()); check_err(own_err(), "rebuild", true);
    slots = std::move(fresh); slots_log = lg; tombs = 0; damaged = false;
  }
  void reserve_log(uint64_t entries) {
    if (entries <= cap) return;
    uint64_t c = std::max<uint64_t>(cap, 1024); while (c < entries) c *= 2;
    DevBuf<uint32_t> fresh(SN_WORDS * (size_t)c); if (n) copy_dev_async(fresh.get(), log.get(), 4 * SN_WORDS * (size_t)n);
    HIP_CHECK(hipGetLastError()); HIP_CHECK(hipStreamSynchronize(gpu().stream));                  // (the old allocation is let go below)
    log = std::move(fresh); cap = c;
  }
};

SpentSet::SpentSet(const uint8_t *exempt, int log2_slots, const uint64_t *seed) : impl(new Impl) {
  Impl &d = *impl;
  if (log2_slots && (log2_slots < 4 || log2_slots > (int)SN_MAX_SLOTS_LOG)) throw GpuError("spent set: a table has 2^4 to 2^31 slots");
  if (exempt) { d.has_exempt = true; memcpy(d.exempt, exempt, 20); }
  if (seed) d.seed = *seed; else if (getrandom(&d.seed, 8, 0) != 8) throw GpuError("spent set: getrandom gave no seed");
  LaneScope lane(0); std::lock_guard<std::mutex> gl(g_gpu_mutex);
  d.min_log = d.slots_log = log2_slots ? (uint32_t)log2_slots : SN_MIN_SLOTS_LOG;
  d.slots = DevBuf<uint32_t>((size_t)1 << d.slots_log); d.err = DevBuf<uint32_t>(1); d.slots.zero(); d.err.zero(); HIP_CHECK(hipStreamSynchronize(gpu().stream));
}
SpentSet::~SpentSet() { try { LaneScope lane(0); std::lock_guard<std::mutex> gl(g_gpu_mutex); impl.reset(); } catch (...) {} }
uint64_t SpentSet::size() const { std::lock_guard<std::mutex> lk(impl->mu); return impl->n; }
bool SpentSet::exempt_key(uint8_t out[20]) const { if (impl->has_exempt) memcpy(out, impl->exempt, 20); return impl->has_exempt; }   // (set once, by the constructor)

// One upload, at most one rebuild, three launches and one download, whatever n is.
bool SpentSet::spend(const uint8_t *keys, const uint8_t *mask, size_t n, bool commit, uint8_t *conflict, uint64_t *size_out) {
  Impl &d = *impl; std::lock_guard<std::mutex> lk(d.mu);
  if ((n && (!keys || !conflict)) || n >= SN_MAX_LOG || d.n + n >= SN_MAX_LOG) return false;
  if (!n) { if (size_out) *size_out = d.n; return true; }
  LaneScope lane(0); std::lock_guard<std::mutex> gl(g_gpu_mutex); hipStream_t s = gpu().stream;
  // a call's arrays, in words (byte arrays padded to words): keys 5n | active | err | won | conflict | winner | where n | counts.  Up: keys .. err (the word arrives
  // as zero).  Down: err .. conflict.
  const uint32_t per = cdiv(n, (size_t)SN_THREADS * SN_MAX_TILES), tiles = cdiv(n, (size_t)SN_THREADS * per); const size_t nw = (n + 3) / 4;
  const size_t o_active = SN_WORDS * n, o_err = o_active + nw, o_won = o_err + 1, o_conf = o_won + 1, o_winner = o_conf + nw, o_where = o_winner + nw, o_counts = o_where + n, words = o_counts + tiles;
  d.pinned(4 * (o_err + 1)); uint8_t *act = d.pin + 4 * o_active; memset(act, 0, 4 * (nw + 1));
  for (size_t i = 0; i < n; i++) { const uint8_t *k = keys + 20 * i; memcpy(d.pin + 20 * i, k, 20); act[i] = (!mask || mask[i]) && !(d.has_exempt && !memcmp(k, d.exempt, 20)); }
  const uint32_t lg = d.slots_log_for(n); if (commit) d.reserve_log(d.n + n);
  Impl::grow(d.work, words); uint32_t *W = d.work.get(); const uint32_t n_old = (uint32_t)d.n;
  DevBuf<uint32_t> fresh; Impl::SyncAtExit sync;                                                  // (declared before the guard: the stream is idle when `fresh` is let go)
  HIP_CHECK(hipMemcpyAsync(W, d.pin, 4 * (o_err + 1), hipMemcpyHostToDevice, s));
  // the table the call runs on: the set's own, or a rebuilt one — which replaces the set's only if the call commits: a check-only call leaves the set's table bit for bit
  if (lg) fresh = d.rebuilt(lg, W + o_err);
  const SnTable T = lg ? d.table(fresh.get(), lg) : d.table(); bool scratch_flag = false; Impl::Writing w(lg ? scratch_flag : d.damaged);
  hipLaunchKernelGGL(k_snset_probe, dim3(cdiv(n, SN_THREADS)), dim3(SN_THREADS), 0, s, T, (const uint32_t *)d.log.get(), n_old, (const uint32_t *)W, (const uint8_t *)(W + o_active), (uint32_t)n, W + o_where, W + o_err); Impl::launched();
  hipLaunchKernelGGL(k_snset_classify, dim3(tiles), dim3(SN_THREADS), 0, s, (const uint32_t *)T.slots, (const uint32_t *)(W + o_where), (uint32_t)n, n_old, per, (uint8_t *)(W + o_conf), (uint8_t *)(W + o_winner), W + o_counts); Impl::launched();
  hipLaunchKernelGGL(k_snset_finalize, dim3(tiles), dim3(SN_THREADS), 0, s, T.slots, d.log.get(), (const uint32_t *)(W + o_where), (const uint8_t *)(W + o_winner), (const uint32_t *)W, (uint32_t)n, n_old, per,
                     (const uint32_t *)(W + o_counts), commit ? 1 : 0, W + o_won); Impl::launched();
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpyAsync(d.pin, W + o_err, 4 * (2 + nw), hipMemcpyDeviceToHost, s)); HIP_CHECK(hipStreamSynchronize(s));
  uint32_t head[2]; memcpy(head, d.pin, 8); d.check_err(head[0], "spend", false);
  if (commit) { if (lg) { d.slots = std::move(fresh); d.slots_log = lg; d.tombs = 0; d.damaged = false; } d.n += head[1]; }
  w.done();
  memcpy(conflict, d.pin + 8, n); if (size_out) *size_out = d.n;
  return true;
}
void SpentSet::set_round_cap(uint32_t rounds) { std::lock_guard<std::mutex> lk(impl->mu); impl->round_cap = rounds ? rounds : SN_ROUND_CAP; }
// One upload, at most one rebuild, and four launches and one download a round, whatever n is: probe, wins, decide, finish.  A batch without conflicts among its own
// keys takes one round.  After round_cap rounds with records still live the host decides those (snset_pairs_finish_host) and one more pass — probe, wins, finish —
// finalises on the device.
bool SpentSet::spend_pairs(const uint8_t *keys, const uint8_t *nkeys, size_t n, bool commit, uint8_t *conflict, uint64_t *size_out) {
  Impl &d = *impl; std::lock_guard<std::mutex> lk(d.mu);
  if ((n && (!keys || !nkeys || !conflict)) || n >= SN_MAX_LOG / 2 || d.n + 2 * n >= SN_MAX_LOG) return false;   // n_old + 1 + e stays below the tombstone for every entry e < 2n
  for (size_t i = 0; i < n; i++) if (nkeys[i] > 2) return false;
  if (!n) { if (size_out) *size_out = d.n; return true; }
  LaneScope lane(0); std::lock_guard<std::mutex> gl(g_gpu_mutex); hipStream_t s = gpu().stream;
  // a call's arrays, in words (byte arrays padded to words): keys 10n | active 2n | status | code | head | win | hold 2n | where 2n | counts.  Up: keys .. head (the
  // head arrives as zero).  Down, after every round: status .. head.
  const uint32_t per = cdiv(n, (size_t)SN_THREADS * SN_MAX_TILES), tiles = cdiv(n, (size_t)SN_THREADS * per); const size_t nw = (n + 3) / 4, nw2 = (2 * n + 3) / 4;
  const size_t o_active = 2 * SN_WORDS * n, o_status = o_active + nw2, o_code = o_status + nw, o_head = o_code + nw, o_win = o_head + SP_HEAD, o_hold = o_win + nw, o_where = o_hold + nw2,
               o_counts = o_where + 2 * n, words = o_counts + tiles;
  d.pinned(4 * o_win); uint8_t *act = d.pin + 4 * o_active, *status = d.pin + 4 * o_status, *code = d.pin + 4 * o_code; memset(act, 0, 4 * (o_win - o_active)); memcpy(d.pin, keys, 40 * n);
  for (size_t i = 0; i < n; i++) {
    const uint8_t *k = keys + 40 * i;
    act[2 * i] = nkeys[i] >= 1 && !(d.has_exempt && !memcmp(k, d.exempt, 20)); act[2 * i + 1] = nkeys[i] == 2;
    if (nkeys[i] == 2 && d.has_exempt && !memcmp(k + 20, d.exempt, 20)) { status[i] = SP_REJECTED; code[i] = 1; }   // the exempt key is never inserted, so as a second key it counts as spent
  }
  const uint32_t lg = d.slots_log_for(2 * n); if (commit) d.reserve_log(d.n + 2 * n);
  Impl::grow(d.work, words); uint32_t *W = d.work.get(); const uint32_t n_old = (uint32_t)d.n;
  DevBuf<uint32_t> fresh; Impl::SyncAtExit sync;                                                  // (declared before the guard: the stream is idle when `fresh` is let go)
  HIP_CHECK(hipMemcpyAsync(W, d.pin, 4 * o_win, hipMemcpyHostToDevice, s));
  if (lg) fresh = d.rebuilt(lg, W + o_head + SP_ERR);                                               // as in spend: a rebuilt table replaces the set's only if the call commits
  const SnTable T = lg ? d.table(fresh.get(), lg) : d.table(); bool scratch_flag = false; Impl::Writing w(lg ? scratch_flag : d.damaged);
  const uint8_t *A = (const uint8_t *)(W + o_active), *H = (const uint8_t *)(W + o_hold), *WIN = (const uint8_t *)(W + o_win); uint8_t *ST = (uint8_t *)(W + o_status), *CO = (uint8_t *)(W + o_code);
  uint32_t head[SP_HEAD], rounds = 0; bool host_pass = false;
  for (;;) {
    hipLaunchKernelGGL(k_snset_pairs_probe, dim3(cdiv(2 * n, SN_THREADS)), dim3(SN_THREADS), 0, s, T, (const uint32_t *)d.log.get(), n_old, (const uint32_t *)W, A, (const uint8_t *)ST, (uint32_t)(2 * n), W + o_where, W + o_head); Impl::launched();
    hipLaunchKernelGGL(k_snset_pairs_wins, dim3(tiles), dim3(SN_THREADS), 0, s, (const uint32_t *)T.slots, (const uint32_t *)(W + o_where), A, (uint32_t)n, n_old, per, ST, CO, (uint8_t *)(W + o_win), (uint8_t *)(W + o_hold), W + o_counts, W + o_head); Impl::launched();
    if (!host_pass) { hipLaunchKernelGGL(k_snset_pairs_decide, dim3(cdiv(n, SN_THREADS)), dim3(SN_THREADS), 0, s, (const uint32_t *)T.slots, (const uint32_t *)(W + o_where), A, H, WIN, (uint32_t)n, n_old, ST, CO, W + o_head); Impl::launched(); }
    hipLaunchKernelGGL(k_snset_pairs_finish, dim3(tiles), dim3(SN_THREADS), 0, s, T.slots, d.log.get(), (const uint32_t *)(W + o_where), A, H, WIN, (const uint32_t *)W, (uint32_t)n, n_old, per, (const uint32_t *)(W + o_counts), commit ? 1 : 0, W + o_head); Impl::launched();
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(status, ST, 4 * (o_win - o_status), hipMemcpyDeviceToHost, s)); HIP_CHECK(hipStreamSynchronize(s));
    memcpy(head, d.pin + 4 * o_head, sizeof head); d.check_err(head[SP_ERR], "spend_pairs", false);
    if (!host_pass) g_snset_rounds.fetch_add(1);
    if (!head[SP_LIVE_N]) break;
    if (host_pass) throw GpuError("spent set: spend_pairs: records live after the host has decided them");
    if (++rounds < d.round_cap) continue;
    snset_pairs_finish_host(d.pin, act, n, status, code); g_snset_host_finishes.fetch_add(1); host_pass = true;   // the round's slots are released: the table is what it was
    HIP_CHECK(hipMemcpyAsync(ST, status, 4 * (o_head - o_status), hipMemcpyHostToDevice, s));
  }
  if (commit) { if (lg) { d.slots = std::move(fresh); d.slots_log = lg; d.tombs = 0; d.damaged = false; } d.n += head[SP_WON]; d.tombs += head[SP_TOMBS]; }
  w.done();
  memcpy(conflict, code, n); if (size_out) *size_out = d.n;
  return true;
}
bool SpentSet::query(uint64_t size, const uint8_t *keys, size_t q, uint64_t *index, bool current) {
  Impl &d = *impl; std::lock_guard<std::mutex> lk(d.mu); if (current) size = d.n;
  if (size > d.n || (q && (!keys || !index)) || q >= SN_MAX_LOG) return false;
  if (!q) return true;
  LaneScope lane(0); std::lock_guard<std::mutex> gl(g_gpu_mutex); hipStream_t s = gpu().stream; d.repair();
  const size_t o_out = (SN_WORDS * q + 1) & ~(size_t)1;                                            // (the answers are 64-bit words)
  d.pinned(std::max<size_t>(20 * q, 8 * q)); Impl::grow(d.work, o_out + 2 * q); uint32_t *W = d.work.get(); memcpy(d.pin, keys, 20 * q);
  Impl::SyncAtExit sync;
  HIP_CHECK(hipMemcpyAsync(W, d.pin, 20 * q, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_snset_query, dim3(cdiv(q, SN_THREADS)), dim3(SN_THREADS), 0, s, d.table(), (const uint32_t *)d.log.get(), (uint32_t)size, (const uint32_t *)W, (uint32_t)q, (unsigned long long *)(W + o_out)); Impl::launched();
  HIP_CHECK(hipGetLastError()); HIP_CHECK(hipMemcpyAsync(d.pin, W + o_out, 8 * q, hipMemcpyDeviceToHost, s)); HIP_CHECK(hipStreamSynchronize(s));
  memcpy(index, d.pin, 8 * q); return true;
}
bool SpentSet::rewind(uint64_t size) {
  Impl &d = *impl; std::lock_guard<std::mutex> lk(d.mu); if (size > d.n) return false;
  if (size == d.n) return true;
  LaneScope lane(0); std::lock_guard<std::mutex> gl(g_gpu_mutex); hipStream_t s = gpu().stream;
  if (!size) {                                                                                     // the empty set: an empty table, and no tombstone
    HIP_CHECK(hipMemsetAsync(d.slots.get(), 0, 4ull << d.slots_log, s)); HIP_CHECK(hipStreamSynchronize(s)); d.n = 0; d.tombs = 0; d.damaged = false; return true;
  }
  d.repair(); Impl::Writing w(d.damaged);
  hipLaunchKernelGGL(k_snset_unlink, dim3(cdiv(d.n - size, SN_THREADS)), dim3(SN_THREADS), 0, s, d.table(), (const uint32_t *)d.log.get(), (uint32_t)size, (uint32_t)d.n, d.err.get()); Impl::launched();
  HIP_CHECK(hipGetLastError()); d.check_err(d.own_err(), "rewind", true);
  d.tombs += d.n - size; d.n = size; w.done(); return true;
}
bool SpentSet::read_log(uint64_t first, uint64_t count, uint8_t *out) {
  Impl &d = *impl; std::lock_guard<std::mutex> lk(d.mu);
  if (first > d.n || count > d.n - first || (count && !out)) return false;
  if (!count) return true;
  LaneScope lane(0); std::lock_guard<std::mutex> gl(g_gpu_mutex); hipStream_t s = gpu().stream; Impl::SyncAtExit sync;
  HIP_CHECK(hipMemcpyAsync(out, d.log.get() + SN_WORDS * (size_t)first, 20 * (size_t)count, hipMemcpyDeviceToHost, s)); HIP_CHECK(hipStreamSynchronize(s));
  return true;
}
void SpentSet::table(std::vector<uint32_t> &slots, uint64_t &seed, uint64_t &tombstones) {
  Impl &d = *impl; std::lock_guard<std::mutex> lk(d.mu); LaneScope lane(0); std::lock_guard<std::mutex> gl(g_gpu_mutex);
  slots.resize((size_t)1 << d.slots_log); d.slots.download(slots.data(), slots.size()); seed = d.seed; tombstones = d.tombs;
}

}  // namespace zk
