// The account table resident in HBM (DESIGN.md "Account table"; include/zk_accounts.h): what the reference keeps per account as statedb.GetCMTBalance / SetCMT
// (core/state_processor.go:112-157, core/state_transition.go:221-223) — a map from a 20-byte address to a 32-byte balance commitment — as an append-only log of
// (address, value, prev) entries and an index over it.  State m is the first m log entries; the value of an address at state m is the value of its latest entry
// below m, or 32 zero bytes.
// Layout: the log holds 14 words an entry (address 5, value 8, prev 1: log index + 1 of the address's previous entry, or 0).  The index is the keyed table
// (keytable.cuh: slot values, the mix, the find-or-claim walk, the rules every kernel keeps), a slot holding log index + 1 of the address's LATEST entry; a tentative
// value n_old + 1 + j means record j of the batch has claimed the slot for an address the table did not hold.  Beside the slots lies one side word a slot, `heads`:
// all zero between calls; during a call the head (record + 1) of the list of the batch's records that ended at the slot — on the segment road, of the first such
// record of each tile of 256.  To the table's rules this file adds:
//   - the one barrier, in k_acct_probe_tiled, is reached by every lane of its workgroup unconditionally, each after a bounded probe of its own, and nothing spins on
//     memory;
//   - every list walk ends after the chain cap or the log's length, and running out sets a word of the call's head;
//   - heads are touched by atomics only, like slots; values, prev words and list links, which are plain stores, are read only in launches after the one that wrote
//     them.
#include <algorithm>
#include <atomic>
#include <cstring>
#include "keytable.cuh"
#include "acct_pred_host.hpp"

namespace zk {

constexpr int AC_VAL = 8, AC_ENTRY = 14, AC_PREV = 13;
// Steps one lane walks along a slot's list before the call hands the predecessor search to the host.  A list holds the batch's records of ONE sender, and a lane of
// that sender walks all of it, so a sender with L records costs L^2 dependent loads: 256 keeps every sender with up to 256 transactions in a call on the device (the
// reference's pool admits 16 to 64 an account by default), and bounds what an adversary who fills a call with one sender can cost it to 256 loads a lane.
constexpr uint32_t ACCT_CHAIN_CAP = 256;
constexpr uint32_t AH_ERR = 0, AH_OVER = 1, AH_TOMBS = 2, AH_HEAD = 4;   // the call's head words: error, a list longer than the cap, tombstones left by a rewind

struct AcTable : KeyTable { uint32_t *heads; };

// Launch 1 of a batch, one lane per record: where[i] = the slot of record i's address (kt_find_or_claim: the resident one, one that a record of the batch has claimed,
// or the empty one this lane claims; a tentative value stays its first claimant's).  Then the record pushes itself on that slot's list: link[i] = the head it replaced.
__global__ void __launch_bounds__(KT_THREADS) k_acct_probe(AcTable T, const uint32_t *__restrict__ log, uint32_t n_old, const uint32_t *__restrict__ addrs, uint32_t n,
                                                            uint32_t *__restrict__ where, uint32_t *__restrict__ link, uint32_t *__restrict__ head) {
  const uint32_t i = blockIdx.x * KT_THREADS + threadIdx.x; if (i >= n) return;
  const uint32_t at = kt_find_or_claim<AC_ENTRY, false>(T, log, n_old, addrs, n, i);
  where[i] = at;
  if (at == KT_NONE) { head[AH_ERR] = 1; link[i] = 0; return; }
  link[i] = atomicExch(T.heads + at, i + 1);
}
// Launch 2, one lane per record: it walks its slot's list (in no order: the exchanges landed as they came) and keeps pred[i] = 1 + the highest record below its own,
// succ[i] = a record above its own exists, base[i] = the slot's resident value (log index + 1 of the address's latest entry) or 0 where the slot is a claimed one.
// A walk of more than `cap` steps raises AH_OVER: launch 3 then does nothing and the host finishes the search (acct_pred_host).
__global__ void __launch_bounds__(KT_THREADS) k_acct_pred(const uint32_t *__restrict__ slots, const uint32_t *__restrict__ heads, const uint32_t *__restrict__ where,
                                                           const uint32_t *__restrict__ link, uint32_t n, uint32_t n_old, uint32_t cap, uint32_t *__restrict__ pred,
                                                           uint32_t *__restrict__ succ, uint32_t *__restrict__ base, uint32_t *__restrict__ head) {
  const uint32_t i = blockIdx.x * KT_THREADS + threadIdx.x; if (i >= n) return;
  const uint32_t w = where[i]; uint32_t best = 0, later = 0, b = 0;
  if (w != KT_NONE) {
    const uint32_t v = slot_load(slots + w); b = v <= n_old ? v : 0u;
    uint32_t node = slot_load(heads + w), steps = 0;
    while (node) {
      if (node > n) { head[AH_ERR] = 4; break; }
      if (steps++ == cap) { head[AH_OVER] = 1; break; }
      const uint32_t j = node - 1;
      if (j < i) best = max(best, node); else if (j > i) later = 1;
      node = link[j];
    }
  }
  pred[i] = best; succ[i] = later; base[i] = b;
}
// ---- the tiled search (DESIGN.md "A stretch of the chain with accounts"): launches 1 and 2 of a SEGMENT batch.  A tile is a workgroup's KT_THREADS consecutive
// records.  Inside a tile the records of one slot find each other through LDS; a slot's list holds ONE node for each tile the slot occurs in — the tile's first
// record of it — so a walk visits at most ceil(n / KT_THREADS) nodes whatever a sender's share of the batch is.
// Launch 1: where[i] as k_acct_probe finds it (same walk, same claim, same tentative values, same error word).  No lane returns before the barrier — the one place a
// lane waits, which every lane of the workgroup reaches after its own bounded probe —; lanes at or beyond n take part with KT_NONE.  Then one pass over the tile's
// 256 where words, every lane reading the same word (a broadcast): the closest lower lane with the lane's slot — pred[i], written at once — and the highest one
// above it — the tile-last.  A lane with a higher one writes succ[i] = 1; the tile-last's succ word is left to launch 2.  A lane without a lower one is the
// tile-first: it writes pred[i] = 0 (launch 2 knows it by that), tlast[i], and pushes itself, and only itself, on the slot's list.
__global__ void __launch_bounds__(KT_THREADS) k_acct_probe_tiled(AcTable T, const uint32_t *__restrict__ log, uint32_t n_old, const uint32_t *__restrict__ addrs, uint32_t n,
                                                                  uint32_t *__restrict__ where, uint32_t *__restrict__ link, uint32_t *__restrict__ pred, uint32_t *__restrict__ succ,
                                                                  uint32_t *__restrict__ tlast, uint32_t *__restrict__ head) {
  __shared__ __align__(16) uint32_t tile[KT_THREADS];
  const uint32_t t = threadIdx.x, first = blockIdx.x * KT_THREADS, i = first + t; uint32_t at = KT_NONE;
  if (i < n) {
    at = kt_find_or_claim<AC_ENTRY, false>(T, log, n_old, addrs, n, i);
    if (at == KT_NONE) head[AH_ERR] = 1;
  }
  tile[t] = at;
  __syncthreads();
  if (i >= n) return;
  where[i] = at;
  if (at == KT_NONE) { link[i] = 0; pred[i] = 0; succ[i] = 0; tlast[i] = i; return; }
  uint32_t lower = 0, last = t;                                                                     // lower: lane + 1 of the closest lower lane of the slot
  const uint4 *tile4 = reinterpret_cast<const uint4 *>(tile);                                      // four words a read: 64 LDS reads a lane, without a branch
#pragma unroll 4
  for (uint32_t q = 0; q < KT_THREADS / 4; q++) {
    const uint4 v = tile4[q]; const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (uint32_t c = 0; c < 4; c++) { const uint32_t j = 4 * q + c; const bool same = w4[c] == at; lower = same && j < t ? j + 1 : lower; last = same && j > t ? j : last; }
  }
  if (last != t) succ[i] = 1;
  if (lower) { pred[i] = first + lower; return; }
  pred[i] = 0; tlast[i] = first + last;
  link[i] = atomicExch(T.heads + at, i + 1);
}
// Launch 2: base[i] as k_acct_pred reads it.  Only a tile-first (pred[i] == 0 and a slot) walks the slot's list — the tile-firsts of the slot, in no order — and keeps
// the highest node below its own and whether one above exists.  Its predecessor is the LAST record of the slot in that earlier tile, tlast[node]; and it stores "a
// later tile holds the slot" into the succ word of its own tile's last record, which launch 1 left alone: a plain store to another record's word, read by launch 3.
// A walk of more than `cap` nodes raises AH_OVER, as in k_acct_pred.
__global__ void __launch_bounds__(KT_THREADS) k_acct_pred_tiled(const uint32_t *__restrict__ slots, const uint32_t *__restrict__ heads, const uint32_t *__restrict__ where,
                                                                 const uint32_t *__restrict__ link, const uint32_t *__restrict__ tlast, uint32_t n, uint32_t n_old, uint32_t cap,
                                                                 uint32_t *pred, uint32_t *succ, uint32_t *__restrict__ base, uint32_t *__restrict__ head) {
  const uint32_t i = blockIdx.x * KT_THREADS + threadIdx.x; if (i >= n) return;
  const uint32_t w = where[i]; uint32_t b = 0;
  if (w != KT_NONE) {
    const uint32_t v = slot_load(slots + w); b = v <= n_old ? v : 0u;
    if (pred[i] == 0) {
      uint32_t node = slot_load(heads + w), steps = 0, best = 0, later = 0; bool sound = true;
      while (node) {
        if (node > n) { head[AH_ERR] = 4; sound = false; break; }
        if (steps++ == cap) { head[AH_OVER] = 1; sound = false; break; }
        const uint32_t j = node - 1;
        if (j < i) best = max(best, node); else if (j > i) later = 1;
        node = link[j];
      }
      const uint32_t mine = tlast[i], theirs = best ? tlast[best - 1] : 0u;
      if (sound && (mine >= n || theirs >= n)) head[AH_ERR] = 4;
      else if (sound) { pred[i] = best ? theirs + 1 : 0u; succ[mine] = later; }                       // (not sound: launch 3 does nothing, or the call fails)
    }
  }
  base[i] = b;
}
// Launch 3, one lane per record.  The value the address has before record i: the batch value of its predecessor (chained), else the value of the resident entry,
// else zero.  fill (append = 0): that value goes to old[i]; the one record of a slot without a successor zeroes the slot's head and, where the slot was a claimed
// one, empties it: the table is what it was before the call.  append = 1: record i becomes log entry n_old + i — address, value, prev = the predecessor's entry or
// the resident one — and the record without a successor leaves its own entry in the slot.  With AH_OVER raised and `forced` not set the launch does nothing.
__global__ void __launch_bounds__(KT_THREADS) k_acct_write(AcTable T, uint32_t *__restrict__ log, uint32_t n_old, const uint32_t *__restrict__ addrs, const uint32_t *__restrict__ vals,
                                                            uint32_t n, const uint32_t *__restrict__ where, const uint32_t *__restrict__ pred, const uint32_t *__restrict__ succ,
                                                            const uint32_t *__restrict__ base, int append, int chained, int forced, uint32_t *__restrict__ old,
                                                            const uint32_t *__restrict__ head) {
  if (head[AH_OVER] && !forced) return;                                                            // (uniform over the grid: an earlier launch wrote it)
  const uint32_t i = blockIdx.x * KT_THREADS + threadIdx.x; if (i >= n) return;
  const uint32_t w = where[i]; if (w == KT_NONE) return;                                           // (the probe has set the error word)
  const uint32_t p = pred[i], b = base[i];
  if (append) {
    uint32_t *dst = log + AC_ENTRY * (size_t)(n_old + i); const uint32_t *a = addrs + KEY_WORDS * (size_t)i, *v = vals + AC_VAL * (size_t)i;
#pragma unroll
    for (int c = 0; c < KEY_WORDS; c++) dst[c] = a[c];
#pragma unroll
    for (int c = 0; c < AC_VAL; c++) dst[KEY_WORDS + c] = v[c];
    dst[AC_PREV] = p ? n_old + p : b;
    if (!succ[i]) { slot_store(T.slots + w, n_old + i + 1); slot_store(T.heads + w, 0u); }
    return;
  }
  const uint32_t *src = (chained && p) ? vals + AC_VAL * (size_t)(p - 1) : b ? log + AC_ENTRY * (size_t)(b - 1) + KEY_WORDS : nullptr;
#pragma unroll
  for (int c = 0; c < AC_VAL; c++) old[AC_VAL * (size_t)i + c] = src ? src[c] : 0u;
  if (!succ[i]) { slot_store(T.heads + w, 0u); if (!b) slot_store(T.slots + w, 0u); }
}
// read-only, one lane per query: the value of address t at state `size` — it finds the address's slot, then walks prev down to an entry below `size`
__global__ void __launch_bounds__(KT_THREADS) k_acct_get(AcTable T, const uint32_t *__restrict__ log, uint32_t n_log, uint32_t size, const uint32_t *__restrict__ addrs, uint32_t q,
                                                          uint32_t *__restrict__ out, uint32_t *__restrict__ head) {
  const uint32_t t = blockIdx.x * KT_THREADS + threadIdx.x; if (t >= q) return;
  const Key20 k = key_load(addrs + KEY_WORDS * (size_t)t); uint32_t s = kt_home(k, T), e = 0;
  for (uint32_t step = 0; step <= T.mask; step++, s = (s + 1) & T.mask) {
    const uint32_t v = slot_load(T.slots + s);
    if (v == 0) break;
    if (v == KT_TOMB) continue;
    if (v > n_log) { head[AH_ERR] = 4; break; }
    if (key_equal(k, key_load(log + AC_ENTRY * (size_t)(v - 1)))) { e = v; break; }
  }
  for (uint32_t step = 0; e > size; step++) {                                                      // prev falls strictly, so the walk ends after n_log steps at the latest
    const uint32_t p = log[AC_ENTRY * (size_t)(e - 1) + AC_PREV];
    if (p >= e || step >= n_log) { head[AH_ERR] = 5; e = 0; break; }
    e = p;
  }
#pragma unroll
  for (int c = 0; c < AC_VAL; c++) out[AC_VAL * (size_t)t + c] = e ? log[AC_ENTRY * (size_t)(e - 1) + KEY_WORDS + c] : 0u;
}
// a fresh table from the log, one lane per live entry: the first entry of an address to arrive claims an empty slot by CAS, every other raises the slot to its own
// index + 1 by atomicMax — whatever the slot holds meanwhile is an entry of the same address — so the slot ends at the address's latest entry
__global__ void __launch_bounds__(KT_THREADS) k_acct_rebuild(AcTable T, const uint32_t *__restrict__ log, uint32_t n_live, uint32_t *__restrict__ err) {
  const uint32_t i = blockIdx.x * KT_THREADS + threadIdx.x; if (i >= n_live) return;
  const Key20 k = key_load(log + AC_ENTRY * (size_t)i); uint32_t s = kt_home(k, T); bool done = false;
  for (uint32_t step = 0; step <= T.mask && !done; step++, s = (s + 1) & T.mask) {
    uint32_t v = slot_load(T.slots + s);
    if (v == 0) { v = atomicCAS(T.slots + s, 0u, i + 1); if (v == 0) { done = true; break; } }
    if (v > n_live) break;
    if (key_equal(k, key_load(log + AC_ENTRY * (size_t)(v - 1)))) { atomicMax(T.slots + s, i + 1); done = true; }
  }
  if (!done) *err = 2;
}
// rewind from n to m, one lane per entry m .. n - 1: the entry whose prev lies below m is the first of its address at or beyond m — one such lane an address — and
// it walks to the address's slot and leaves prev there, or the tombstone (counted) where the address has no entry below m.  A slot another lane has already
// rewritten holds the tombstone or an entry of that lane's address: no match either way.
__global__ void __launch_bounds__(KT_THREADS) k_acct_rewind(AcTable T, const uint32_t *__restrict__ log, uint32_t m, uint32_t n, uint32_t *__restrict__ head) {
  const uint32_t i = m + blockIdx.x * KT_THREADS + threadIdx.x; if (i >= n) return;
  const uint32_t p = log[AC_ENTRY * (size_t)i + AC_PREV]; if (p > m) return;
  const Key20 k = key_load(log + AC_ENTRY * (size_t)i); uint32_t s = kt_home(k, T); bool done = false;
  for (uint32_t step = 0; step <= T.mask; step++, s = (s + 1) & T.mask) {
    const uint32_t v = slot_load(T.slots + s);
    if (v == 0) break;
    if (v == KT_TOMB) continue;
    if (v > n) break;
    if (key_equal(k, key_load(log + AC_ENTRY * (size_t)(v - 1)))) { slot_store(T.slots + s, p ? p : KT_TOMB); if (!p) atomicAdd(head + AH_TOMBS, 1u); done = true; break; }
  }
  if (!done) head[AH_ERR] = 3;
}

static std::atomic<uint64_t> g_acct_launches{0}, g_acct_host_finishes{0};
void AccountTable::launches(uint64_t &launches, uint64_t &host_finishes) { launches = g_acct_launches.load(); host_finishes = g_acct_host_finishes.load(); }

struct AccountTable::Impl : LogTableState {
  uint32_t chain_cap = ACCT_CHAIN_CAP; DevBuf<uint32_t> heads;
  Impl(int log2_slots, const uint64_t *seed) : LogTableState("account table", AC_ENTRY, log2_slots, seed) {}
  AcTable table(uint32_t *s, uint32_t *h, uint32_t lg) const { return AcTable{handle(s, lg), h}; }
  AcTable table() const { return table(slots.get(), heads.get(), slots_log); }
  static void launched() { g_acct_launches.fetch_add(1); }
  static void check_err(uint32_t e, const char *what) {
    if (!e) return;
    throw GpuError(std::string("account table: ") + what + (e == 1 ? ": a probe went round the whole table" : e == 2 ? ": no empty slot while rebuilding" : e == 3 ? ": an entry of the log is not in the table"
                   : e == 5 ? ": a prev link does not fall" : ": a slot or a list holds no value of this call"));
  }
  struct Fresh { DevBuf<uint32_t> slots, heads; };
  Fresh rebuilt(uint32_t lg, uint32_t *err_word) {                   // two memsets and one launch on the main stream, not synchronised
    Fresh f; f.slots = DevBuf<uint32_t>((size_t)1 << lg); f.heads = DevBuf<uint32_t>((size_t)1 << lg); hipStream_t s = gpu().stream;
    HIP_CHECK(hipMemsetAsync(f.slots.get(), 0, 4ull << lg, s)); HIP_CHECK(hipMemsetAsync(f.heads.get(), 0, 4ull << lg, s));
    if (n) { hipLaunchKernelGGL(k_acct_rebuild, dim3(cdiv(n, KT_THREADS)), dim3(KT_THREADS), 0, s, table(f.slots.get(), f.heads.get(), lg), (const uint32_t *)log.get(), (uint32_t)n, err_word); launched(); HIP_CHECK(hipGetLastError()); }
    return f;
  }
  void adopt(Fresh &f, uint32_t lg) { adopt_slots(f.slots, lg); heads = std::move(f.heads); }   // a damaged table is made anew slots and heads
  // a head of its own for the entries that are no batch: zeroed on the stream, in the call's workspace
  uint32_t *own_head() { grow_buf(work, AH_HEAD); HIP_CHECK(hipMemsetAsync(work.get(), 0, 4 * AH_HEAD, gpu().stream)); return work.get(); }
  void read_head(const uint32_t *dev, uint32_t out[AH_HEAD]) { HIP_CHECK(hipMemcpyAsync(out, dev, 4 * AH_HEAD, hipMemcpyDeviceToHost, gpu().stream)); HIP_CHECK(hipStreamSynchronize(gpu().stream)); }
  void repair() {                                                     // get and rewind read the table's own index: after damage it is made anew first
    if (!damaged) return;
    const uint32_t lg = slots_log_for(0); uint32_t *h = own_head(); Fresh f = rebuilt(lg, h + AH_ERR); uint32_t head[AH_HEAD]; read_head(h, head); check_err(head[AH_ERR], "rebuild");
    adopt(f, lg);
  }
  template <class Gather> const uint8_t *batch(size_t m, bool append, bool chained, bool tiled, Gather gather);
  // Read-only, one launch: the values of q addresses at state `size`.  gather(dst) writes the q x 20 address bytes into the pinned staging buffer; the return value
  // points at q x 32 bytes in pinned memory, valid until the table's next call.  The caller holds the table's mutex and has checked the arguments.
  template <class Gather> const uint8_t *values_at(size_t q, uint64_t size, const char *what, Gather gather) {
    LaneScope lane(0); std::lock_guard<std::mutex> gl(g_gpu_mutex); hipStream_t s = gpu().stream; repair();
    const size_t o_head = KEY_WORDS * q, o_out = o_head + AH_HEAD; pinned(4 * (o_out + AC_VAL * q)); grow_buf(work, o_out + AC_VAL * q); uint32_t *W = work.get();
    gather(pin); memset(pin + 4 * o_head, 0, 4 * AH_HEAD); SyncAtExit sync;
    HIP_CHECK(hipMemcpyAsync(W, pin, 4 * o_out, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_acct_get, dim3(cdiv(q, KT_THREADS)), dim3(KT_THREADS), 0, s, table(), (const uint32_t *)log.get(), (uint32_t)n, (uint32_t)size, (const uint32_t *)W, (uint32_t)q, W + o_out, W + o_head); launched();
    HIP_CHECK(hipGetLastError()); HIP_CHECK(hipMemcpyAsync(pin, W + o_head, 4 * (AH_HEAD + AC_VAL * q), hipMemcpyDeviceToHost, s)); HIP_CHECK(hipStreamSynchronize(s));
    uint32_t head[AH_HEAD]; memcpy(head, pin, sizeof head); check_err(head[AH_ERR], what);
    return pin + 4 * AH_HEAD;
  }
};

AccountTable::AccountTable(int log2_slots, const uint64_t *seed) : impl(new Impl(log2_slots, seed)) {
  Impl &d = *impl; LaneScope lane(0); std::lock_guard<std::mutex> gl(g_gpu_mutex);
  d.slots = DevBuf<uint32_t>((size_t)1 << d.slots_log); d.heads = DevBuf<uint32_t>((size_t)1 << d.slots_log); d.slots.zero(); d.heads.zero(); HIP_CHECK(hipStreamSynchronize(gpu().stream));
}
AccountTable::~AccountTable() { try { LaneScope lane(0); std::lock_guard<std::mutex> gl(g_gpu_mutex); impl.reset(); } catch (...) {} }
uint64_t AccountTable::size() const { std::lock_guard<std::mutex> lk(impl->mu); return impl->n; }
void AccountTable::set_chain_cap(uint32_t cap) { std::lock_guard<std::mutex> lk(impl->mu); impl->chain_cap = cap ? cap : ACCT_CHAIN_CAP; }

// One batch of m records that all take part (the callers leave out the others): gather(addrs, vals) writes their m x 20 address bytes and m x 32 value bytes straight
// into the pinned staging buffer, the one pass the host makes over the batch.  append: the records become log entries n .. n + m - 1; otherwise the return value
// points at m x 32 bytes in pinned memory, each record's value before it — chained: after the earlier records of the batch —, valid until the table's next call.
// One upload, at most one rebuild, three launches and one download whatever m is; a list beyond the chain cap adds the host's search, one upload, the third launch
// again and one download.  tiled: launches 1 and 2 are the tiled search's (the segment entries), with one more array, tlast m, at the end of the call's arrays; the
// third launch, the host finish and everything else are the same.  The caller holds the table's mutex and has checked the arguments.
template <class Gather> const uint8_t *AccountTable::Impl::batch(size_t m, bool append, bool chained, bool tiled, Gather gather) {
  Impl &d = *this;
  LaneScope lane(0); std::lock_guard<std::mutex> gl(g_gpu_mutex); hipStream_t s = gpu().stream;
  // a call's arrays, in words: addrs 5m | vals 8m | head | old 8m | pred m | succ m | where m | link m | base m.  Up: addrs .. head (the head arrives as zero).  Down:
  // head .. old (append: the head alone).  Pinned memory, in words: the upload | the download | pred m, succ m of a host finish — the addresses stay where they are.
  const size_t o_vals = KEY_WORDS * m, o_head = o_vals + AC_VAL * m, o_old = o_head + AH_HEAD, o_pred = o_old + AC_VAL * m, o_succ = o_pred + m, o_where = o_succ + m, o_link = o_where + m, o_base = o_link + m,
               o_tlast = o_base + m, words = o_tlast + (tiled ? m : 0), down = AH_HEAD + (append ? 0 : AC_VAL * m);
  const size_t up = o_head + AH_HEAD, p_down = up, p_ps = p_down + down;
  d.pinned(4 * (p_ps + 2 * m)); uint8_t *const back = d.pin + 4 * p_down;
  gather(d.pin, d.pin + 4 * o_vals); memset(d.pin + 4 * o_head, 0, 4 * AH_HEAD);
  const uint32_t lg = d.slots_log_for(m); if (append) d.reserve_log(d.n + m);
  grow_buf(d.work, words); uint32_t *W = d.work.get(); const uint32_t n_old = (uint32_t)d.n, mm = (uint32_t)m;
  Fresh fresh; SyncAtExit sync;                                                                     // (declared before the guard: the stream is idle when `fresh` is let go)
  HIP_CHECK(hipMemcpyAsync(W, d.pin, 4 * up, hipMemcpyHostToDevice, s));
  // the table the call runs on: the table's own, or a rebuilt one — which replaces the table's only if the call appends: a fill leaves the index bit for bit
  if (lg) fresh = d.rebuilt(lg, W + o_head + AH_ERR);
  const AcTable T = lg ? d.table(fresh.slots.get(), fresh.heads.get(), lg) : d.table(); bool scratch_flag = false; Writing w(lg ? scratch_flag : d.damaged);
  const dim3 grid(cdiv(m, KT_THREADS)), block(KT_THREADS); const uint32_t *A = W, *V = W + o_vals;
  if (tiled) {
    hipLaunchKernelGGL(k_acct_probe_tiled, grid, block, 0, s, T, (const uint32_t *)d.log.get(), n_old, A, mm, W + o_where, W + o_link, W + o_pred, W + o_succ, W + o_tlast, W + o_head); launched();
    hipLaunchKernelGGL(k_acct_pred_tiled, grid, block, 0, s, (const uint32_t *)T.slots, (const uint32_t *)T.heads, (const uint32_t *)(W + o_where), (const uint32_t *)(W + o_link), (const uint32_t *)(W + o_tlast), mm, n_old,
                       d.chain_cap, W + o_pred, W + o_succ, W + o_base, W + o_head); launched();
  } else {
    hipLaunchKernelGGL(k_acct_probe, grid, block, 0, s, T, (const uint32_t *)d.log.get(), n_old, A, mm, W + o_where, W + o_link, W + o_head); launched();
    hipLaunchKernelGGL(k_acct_pred, grid, block, 0, s, (const uint32_t *)T.slots, (const uint32_t *)T.heads, (const uint32_t *)(W + o_where), (const uint32_t *)(W + o_link), mm, n_old, d.chain_cap, W + o_pred, W + o_succ,
                       W + o_base, W + o_head); launched();
  }
  auto write = [&](int forced) {
    hipLaunchKernelGGL(k_acct_write, grid, block, 0, s, T, d.log.get(), n_old, A, V, mm, (const uint32_t *)(W + o_where), (const uint32_t *)(W + o_pred), (const uint32_t *)(W + o_succ), (const uint32_t *)(W + o_base),
                       append ? 1 : 0, chained ? 1 : 0, forced, W + o_old, (const uint32_t *)(W + o_head)); launched();
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(back, W + o_head, 4 * down, hipMemcpyDeviceToHost, s)); HIP_CHECK(hipStreamSynchronize(s));
  };
  write(0);
  uint32_t head[AH_HEAD]; memcpy(head, back, sizeof head); check_err(head[AH_ERR], append ? "append" : "fill");
  if (head[AH_OVER]) {                                                                              // the third launch did nothing: the host finishes the search
    uint32_t *ps = (uint32_t *)(d.pin + 4 * p_ps); acct_pred_host(d.pin, m, ps, ps + m); g_acct_host_finishes.fetch_add(1);
    HIP_CHECK(hipMemcpyAsync(W + o_pred, ps, 8 * m, hipMemcpyHostToDevice, s));
    write(1); memcpy(head, back, sizeof head); check_err(head[AH_ERR], append ? "append" : "fill");
  }
  if (append) { if (lg) d.adopt(fresh, lg); d.n += m; }
  w.done();
  return back + 4 * AH_HEAD;
}

bool AccountTable::set(const uint8_t *addrs, const uint8_t *values, size_t n, uint64_t *size_out) {
  Impl &d = *impl; std::lock_guard<std::mutex> lk(d.mu);
  if ((n && (!addrs || !values)) || n >= KT_MAX_LOG || d.n + n >= KT_MAX_LOG) return false;
  if (n) d.batch(n, true, true, false, [&](uint8_t *a, uint8_t *v) { memcpy(a, addrs, 20 * n); memcpy(v, values, 32 * n); });
  if (size_out) *size_out = d.n;
  return true;
}
// the slots of a record (include/zk_records.h: kind at byte 0, args[k] at byte 528 + 32 k): its old and its new balance commitment
static inline int acct_old_arg(uint8_t kind) { return kind == 2 ? 2 : 0; }
static inline int acct_new_arg(uint8_t kind) { return kind == 2 ? 4 : kind == 1 ? 3 : 2; }
constexpr size_t REC_BYTES = 720, REC_ARGS = 528;
static size_t acct_taking_part(const uint8_t *recs, size_t n) { size_t m = 0; for (size_t i = 0; i < n; i++) m += recs[REC_BYTES * i] <= 3; return m; }
// the senders (and, unless v is null, the new slots) of the records with kind <= 3, packed in record order
static void acct_gather(const uint8_t *addrs, const uint8_t *recs, size_t n, uint8_t *a, uint8_t *v) {
  for (size_t i = 0, j = 0; i < n; i++) { const uint8_t *r = recs + REC_BYTES * i; if (r[0] > 3) continue;
    memcpy(a + 20 * j, addrs + 20 * i, 20); if (v) memcpy(v + 32 * j, r + REC_ARGS + 32 * acct_new_arg(r[0]), 32); j++; }
}
bool AccountTable::fill(const uint8_t *addrs, uint8_t *recs, size_t n, bool chained, bool tiled) {
  Impl &d = *impl; std::lock_guard<std::mutex> lk(d.mu);
  if ((n && (!addrs || !recs)) || n >= KT_MAX_LOG || d.n + n >= KT_MAX_LOG) return false;
  const size_t m = acct_taking_part(recs, n); if (!m) return true;
  const uint8_t *olds = nullptr;
  if (chained) olds = d.batch(m, false, true, tiled, [&](uint8_t *a, uint8_t *v) { acct_gather(addrs, recs, n, a, v); });
  else olds = d.values_at(m, d.n, "fill", [&](uint8_t *a) { acct_gather(addrs, recs, n, a, nullptr); });   // the pool's rule: every record against the current state
  for (size_t i = 0, j = 0; i < n; i++) { uint8_t *r = recs + REC_BYTES * i; if (r[0] <= 3) memcpy(r + REC_ARGS + 32 * acct_old_arg(r[0]), olds + 32 * j++, 32); }
  return true;
}
bool AccountTable::commit_chain(const uint8_t *addrs, const uint8_t *recs, size_t n, uint64_t *size_out, bool tiled) {
  Impl &d = *impl; std::lock_guard<std::mutex> lk(d.mu);
  if ((n && (!addrs || !recs)) || n >= KT_MAX_LOG || d.n + n >= KT_MAX_LOG) return false;
  const size_t m = acct_taking_part(recs, n);
  if (m) d.batch(m, true, true, tiled, [&](uint8_t *a, uint8_t *v) { acct_gather(addrs, recs, n, a, v); });
  if (size_out) *size_out = d.n;
  return true;
}
bool AccountTable::get(const uint8_t *addrs, size_t q, int64_t at_size, uint8_t *out) {
  Impl &d = *impl; std::lock_guard<std::mutex> lk(d.mu); const uint64_t size = at_size < 0 ? d.n : (uint64_t)at_size;
  if (at_size < -1 || size > d.n || (q && (!addrs || !out)) || q >= KT_MAX_LOG) return false;
  if (!q) return true;
  memcpy(out, d.values_at(q, size, "get", [&](uint8_t *a) { memcpy(a, addrs, 20 * q); }), 32 * q);
  return true;
}
bool AccountTable::rewind(uint64_t size) {
  Impl &d = *impl; std::lock_guard<std::mutex> lk(d.mu); if (size > d.n) return false;
  if (size == d.n) return true;
  LaneScope lane(0); std::lock_guard<std::mutex> gl(g_gpu_mutex); hipStream_t s = gpu().stream;
  if (!size) {                                                                                     // the empty table: no entry, no tombstone
    HIP_CHECK(hipMemsetAsync(d.slots.get(), 0, 4ull << d.slots_log, s)); HIP_CHECK(hipMemsetAsync(d.heads.get(), 0, 4ull << d.slots_log, s)); HIP_CHECK(hipStreamSynchronize(s));
    d.n = 0; d.tombs = 0; d.damaged = false; return true;
  }
  d.repair(); Impl::Writing w(d.damaged); SyncAtExit sync; uint32_t *h = d.own_head();
  hipLaunchKernelGGL(k_acct_rewind, dim3(cdiv(d.n - size, KT_THREADS)), dim3(KT_THREADS), 0, s, d.table(), (const uint32_t *)d.log.get(), (uint32_t)size, (uint32_t)d.n, h); Impl::launched();
  HIP_CHECK(hipGetLastError()); uint32_t head[AH_HEAD]; d.read_head(h, head); Impl::check_err(head[AH_ERR], "rewind");
  d.tombs += head[AH_TOMBS]; d.n = size; w.done(); return true;
}
bool AccountTable::read_log(uint64_t first, uint64_t count, uint8_t *out) { return impl->read_log(first, count, out); }
void AccountTable::table(std::vector<uint32_t> &slots, uint64_t &seed, uint64_t &tombstones) { impl->read_slots(slots, seed, tombstones); }

}  // namespace zk
