// The set of spent serial numbers resident in HBM (DESIGN.md "Spent serial numbers"; include/zk_spent.h): what core/state_processor.go:106-163 keeps in the state
// trie — statedb.Exist(BytesToAddress(sn)), "sn is already used", CreateAccount — as an append-only log of distinct 20-byte keys in insertion order and an index over it.
// State m is the first m log entries.
// Layout: the log holds 5 words an entry, the key.  The index, its slot values, the mix, the find-or-claim walk and the rules every kernel keeps are the keyed table's
// (keytable.cuh); this file holds what the set does with them.
#include <algorithm>
#include <atomic>
#include <cstring>
#include "keytable.cuh"

namespace zk {

constexpr uint32_t SN_MAX_TILES = 1024;
constexpr uint32_t SN_ROUND_CAP = 8;                               // spend_pairs: rounds on the device before the host finishes the live records.  A bound on what an adversary can cost a call, not a tuned number

// One lane per record of the batch; where[i] = the slot record i ended at (kt_find_or_claim, a tentative value lowered to the lowest record of the key), KT_NONE for a
// record that is masked out or exempt (active[i] = 0).
__global__ void __launch_bounds__(KT_THREADS) k_snset_probe(KeyTable T, const uint32_t *__restrict__ log, uint32_t n_old, const uint32_t *__restrict__ keys,
                                                             const uint8_t *__restrict__ active, uint32_t n, uint32_t *__restrict__ where, uint32_t *__restrict__ err) {
  const uint32_t i = blockIdx.x * KT_THREADS + threadIdx.x; if (i >= n) return;
  if (!active[i]) { where[i] = KT_NONE; return; }
  const uint32_t at = kt_find_or_claim<KEY_WORDS, true>(T, log, n_old, keys, n, i);
  if (at == KT_NONE) *err = 1;
  where[i] = at;
}
// A later launch: every record reads its slot's final value.  Workgroup b takes the records [b, b + 1) * per * KT_THREADS and leaves its number of winners in counts[b].
__global__ void __launch_bounds__(KT_THREADS) k_snset_classify(const uint32_t *__restrict__ slots, const uint32_t *__restrict__ where, uint32_t n, uint32_t n_old, uint32_t per,
                                                                uint8_t *__restrict__ conflict, uint8_t *__restrict__ winner, uint32_t *__restrict__ counts) {
  __shared__ uint32_t total; if (threadIdx.x == 0) total = 0;
  __syncthreads();
  uint32_t mine = 0;
  for (uint32_t it = 0; it < per; it++) {
    const uint64_t i = ((uint64_t)blockIdx.x * per + it) * KT_THREADS + threadIdx.x; if (i >= n) break;
    const uint32_t w = where[i]; uint8_t c = 0, win = 0;
    if (w != KT_NONE) { const uint32_t v = slot_load(slots + w); if (v <= n_old) c = 1; else if (v == n_old + 1 + (uint32_t)i) win = 1; else c = 2; }
    conflict[i] = c; winner[i] = win; mine += win;
  }
  if (mine) atomicAdd(&total, mine);
  __syncthreads();
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}
// A later launch again, for the winners: rank = winners of the earlier workgroups + rank inside the workgroup (ballot and popcount a wave, LDS across the waves), so
// committed keys enter the log in record order.  commit: the key goes to log[n_old + rank] and the slot gets n_old + rank + 1; otherwise the slot is emptied, and as
// every tentative slot has exactly one winner the table is what it was before the call.  The last workgroup leaves the number of winners in n_won.
__global__ void __launch_bounds__(KT_THREADS) k_snset_finalize(uint32_t *__restrict__ slots, uint32_t *__restrict__ log, const uint32_t *__restrict__ where, const uint8_t *__restrict__ winner,
                                                                const uint32_t *__restrict__ keys, uint32_t n, uint32_t n_old, uint32_t per, const uint32_t *__restrict__ counts, int commit,
                                                                uint32_t *__restrict__ n_won) {
  __shared__ uint32_t before, wave_sum[KT_THREADS / 64];
  uint32_t running = kt_ranks_before(&before, counts);
  for (uint32_t it = 0; it < per; it++) {                                                          // (uniform: every lane of the workgroup takes every barrier)
    const uint64_t i = ((uint64_t)blockIdx.x * per + it) * KT_THREADS + threadIdx.x; const bool win = i < n && winner[i];
    uint32_t all; const uint32_t rank = running + kt_rank_step(win, false, wave_sum, all);
    if (win) {
      const uint32_t s = where[i];
      if (commit) { key_store(log + KEY_WORDS * (size_t)(n_old + rank), key_load(keys + KEY_WORDS * i)); slot_store(slots + s, n_old + rank + 1); }
      else slot_store(slots + s, 0u);
    }
    running += all;
    __syncthreads();
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) *n_won = running;
}
// a fresh table from the log: one lane per live entry; the keys are distinct, so CAS into empty is all there is
__global__ void __launch_bounds__(KT_THREADS) k_snset_rebuild(KeyTable T, const uint32_t *__restrict__ log, uint32_t n_live, uint32_t *__restrict__ err) {
  const uint32_t i = blockIdx.x * KT_THREADS + threadIdx.x; if (i >= n_live) return;
  uint32_t s = kt_home(key_load(log + KEY_WORDS * (size_t)i), T); bool done = false;
  for (uint32_t step = 0; step <= T.mask && !done; step++, s = (s + 1) & T.mask) done = atomicCAS(T.slots + s, 0u, i + 1) == 0;
  if (!done) *err = 2;
}
// rewind from n to m: one lane per entry m .. n - 1 walks to the slot that holds its own index + 1 and leaves the tombstone there
__global__ void __launch_bounds__(KT_THREADS) k_snset_unlink(KeyTable T, const uint32_t *__restrict__ log, uint32_t m, uint32_t n, uint32_t *__restrict__ err) {
  const uint32_t i = m + blockIdx.x * KT_THREADS + threadIdx.x; if (i >= n) return;
  uint32_t s = kt_home(key_load(log + KEY_WORDS * (size_t)i), T); bool done = false;
  for (uint32_t step = 0; step <= T.mask; step++, s = (s + 1) & T.mask) {
    const uint32_t v = slot_load(T.slots + s);
    if (v == i + 1) { slot_store(T.slots + s, KT_TOMB); done = true; break; }
    if (v == 0) break;
  }
  if (!done) *err = 3;
}
// read-only: index[t] = the position of key t in the log if it is below `size`, else 2^64 - 1.  An entry at `size` or beyond does not match and the walk goes on.
__global__ void __launch_bounds__(KT_THREADS) k_snset_query(KeyTable T, const uint32_t *__restrict__ log, uint32_t size, const uint32_t *__restrict__ keys, uint32_t q,
                                                             unsigned long long *__restrict__ index) {
  const uint32_t t = blockIdx.x * KT_THREADS + threadIdx.x; if (t >= q) return;
  const Key20 k = key_load(keys + KEY_WORDS * (size_t)t); uint32_t s = kt_home(k, T); unsigned long long found = ~0ull;
  for (uint32_t step = 0; step <= T.mask; step++, s = (s + 1) & T.mask) {
    const uint32_t v = slot_load(T.slots + s);
    if (v == 0) break;
    if (v == KT_TOMB || v - 1 >= size) continue;
    if (key_equal(k, key_load(log + KEY_WORDS * (size_t)(v - 1)))) { found = v - 1; break; }
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
__global__ void __launch_bounds__(KT_THREADS) k_snset_pairs_probe(KeyTable T, const uint32_t *__restrict__ log, uint32_t n_old, const uint32_t *__restrict__ keys,
                                                                   const uint8_t *__restrict__ active, const uint8_t *__restrict__ status, uint32_t n2, uint32_t *__restrict__ where,
                                                                   uint32_t *__restrict__ head) {
  const uint32_t e = blockIdx.x * KT_THREADS + threadIdx.x; if (e >= n2) return;
  if (!active[e] || status[e >> 1] == SP_REJECTED) { where[e] = KT_NONE; return; }
  const uint32_t at = kt_find_or_claim<KEY_WORDS, true>(T, log, n_old, keys, n2, e);
  if (at == KT_NONE) head[SP_ERR] = 1;
  where[e] = at;
}
// A later launch, one lane per record that is not rejected: hold[e] = entry e holds its slot.  A live record with a key that was in the set before the call is
// rejected with code 1; one that holds every slot of its own has won and is accepted for good — its lower-indexed competitors can only leave.  win[i] = record i is
// accepted; counts[b] = the entries of the accepted records of workgroup b's tile, for finish's ranks.  Lane 0 zeroes the live count that decide adds to.
__global__ void __launch_bounds__(KT_THREADS) k_snset_pairs_wins(const uint32_t *__restrict__ slots, const uint32_t *__restrict__ where, const uint8_t *__restrict__ active, uint32_t n,
                                                                  uint32_t n_old, uint32_t per, uint8_t *__restrict__ status, uint8_t *__restrict__ code, uint8_t *__restrict__ win,
                                                                  uint8_t *__restrict__ hold, uint32_t *__restrict__ counts, uint32_t *__restrict__ head) {
  __shared__ uint32_t total; if (threadIdx.x == 0) { total = 0; if (blockIdx.x == 0) head[SP_LIVE_N] = 0; }
  __syncthreads();
  uint32_t mine = 0;
  for (uint32_t it = 0; it < per; it++) {
    const uint64_t i = ((uint64_t)blockIdx.x * per + it) * KT_THREADS + threadIdx.x; if (i >= n) break;
    uint8_t st = status[i]; uint32_t held = 0; bool all = true, resident = false;
#pragma unroll
    for (uint32_t j = 0; j < 2; j++) {
      const uint64_t e = 2 * i + j; uint8_t h = 0;
      if (st != SP_REJECTED && active[e]) {
        const uint32_t w = where[e], v = w == KT_NONE ? 0u : slot_load(slots + w);
        if (w != KT_NONE && v <= n_old) resident = true;
        h = w != KT_NONE && v == n_old + 1 + (uint32_t)e; held += h; all = all && h;
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
__global__ void __launch_bounds__(KT_THREADS) k_snset_pairs_decide(const uint32_t *__restrict__ slots, const uint32_t *__restrict__ where, const uint8_t *__restrict__ active,
                                                                    const uint8_t *__restrict__ hold, const uint8_t *__restrict__ win, uint32_t n, uint32_t n_old,
                                                                    uint8_t *__restrict__ status, uint8_t *__restrict__ code, uint32_t *__restrict__ head) {
  const uint32_t i = blockIdx.x * KT_THREADS + threadIdx.x; bool live = false;
  if (i < n && status[i] == SP_LIVE) {
    bool lost = false;
#pragma unroll
    for (uint32_t j = 0; j < 2; j++) {
      const uint64_t e = 2 * (uint64_t)i + j; if (!active[e] || hold[e]) continue;
      const uint32_t w = where[e]; if (w == KT_NONE) continue;                                     // (the probe has set the error word)
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
__global__ void __launch_bounds__(KT_THREADS) k_snset_pairs_finish(uint32_t *__restrict__ slots, uint32_t *__restrict__ log, const uint32_t *__restrict__ where, const uint8_t *__restrict__ active,
                                                                    const uint8_t *__restrict__ hold, const uint8_t *__restrict__ win, const uint32_t *__restrict__ keys, uint32_t n,
                                                                    uint32_t n_old, uint32_t per, const uint32_t *__restrict__ counts, int commit, uint32_t *__restrict__ head) {
  __shared__ uint32_t before, wave_sum[KT_THREADS / 64];
  if (head[SP_LIVE_N]) {                                                                           // (uniform over the grid: decide, an earlier launch, wrote it)
    for (uint32_t it = 0; it < per; it++) {
      const uint64_t i = ((uint64_t)blockIdx.x * per + it) * KT_THREADS + threadIdx.x; if (i >= n) break;
#pragma unroll
      for (uint32_t j = 0; j < 2; j++) if (hold[2 * i + j]) slot_store(slots + where[2 * i + j], 0u);
    }
    return;
  }
  uint32_t running = kt_ranks_before(&before, counts), tombs = 0;
  for (uint32_t it = 0; it < per; it++) {                                                          // (uniform: every lane of the workgroup takes every barrier)
    const uint64_t i = ((uint64_t)blockIdx.x * per + it) * KT_THREADS + threadIdx.x; const bool won = i < n && win[i];
    uint32_t all, rank = running + kt_rank_step(won && hold[2 * i], won && hold[2 * i + 1], wave_sum, all);
    if (i < n) {
#pragma unroll
      for (uint32_t j = 0; j < 2; j++) {
        const uint64_t e = 2 * i + j; if (!hold[e]) continue;
        const uint32_t s = where[e];
        if (won && commit) { key_store(log + KEY_WORDS * (size_t)(n_old + rank), key_load(keys + KEY_WORDS * e)); slot_store(slots + s, n_old + rank + 1); rank++; }
        else if (commit) { slot_store(slots + s, KT_TOMB); tombs++; }
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

struct SpentSet::Impl : LogTableState {
  uint32_t round_cap = SN_ROUND_CAP; bool has_exempt = false; uint8_t exempt[20];
  DevBuf<uint32_t> err /* one word for rebuild and rewind outside a spend call, zero between calls */;
  Impl(int log2_slots, const uint64_t *seed) : LogTableState("spent set", KEY_WORDS, log2_slots, seed) {}
  KeyTable table() const { return handle(slots.get(), slots_log); }
  static void launched() { g_snset_launches.fetch_add(1); }
  // An error word read after a synchronise.  No load factor at or below one half produces one.
  void check_err(uint32_t e, const char *what, bool own_word) {
    if (!e) return;
    if (own_word) { (void)hipMemsetAsync(err.get(), 0, 4, gpu().stream); (void)hipStreamSynchronize(gpu().stream); }
    throw GpuError(std::string(name) + ": " + what + (e == 1 ? ": a probe went round the whole table" : e == 2 ? ": no empty slot while rebuilding" : e == 4 ? ": a slot holds no value of this call" : ": an entry of the log is not in the table"));
  }
  DevBuf<uint32_t> rebuilt(uint32_t lg, uint32_t *err_word) {        // one memset and one launch on the main stream, not synchronised
    DevBuf<uint32_t> fresh((size_t)1 << lg); hipStream_t s = gpu().stream; HIP_CHECK(hipMemsetAsync(fresh.get(), 0, 4ull << lg, s));
    if (n) { hipLaunchKernelGGL(k_snset_rebuild, dim3(cdiv(n, KT_THREADS)), dim3(KT_THREADS), 0, s, handle(fresh.get(), lg), (const uint32_t *)log.get(), (uint32_t)n, err_word); launched(); HIP_CHECK(hipGetLastError()); }
    return fresh;
  }
  uint32_t own_err() { uint32_t e = 0; HIP_CHECK(hipMemcpyAsync(&e, err.get(), 4, hipMemcpyDeviceToHost, gpu().stream)); HIP_CHECK(hipStreamSynchronize(gpu().stream)); return e; }
  void repair() {                                                     // query and rewind read the set's own table: after damage it is made anew first
    if (!damaged) return;
    const uint32_t lg = slots_log_for(0); DevBuf<uint32_t> fresh = rebuilt(lg, err.get()); check_err(own_err(), "rebuild", true);
    adopt_slots(fresh, lg);
  }
};

SpentSet::SpentSet(const uint8_t *exempt, int log2_slots, const uint64_t *seed) : impl(new Impl(log2_slots, seed)) {
  Impl &d = *impl;
  if (exempt) { d.has_exempt = true; memcpy(d.exempt, exempt, 20); }
  LaneScope lane(0); std::lock_guard<std::mutex> gl(g_gpu_mutex);
  d.slots = DevBuf<uint32_t>((size_t)1 << d.slots_log); d.err = DevBuf<uint32_t>(1); d.slots.zero(); d.err.zero(); HIP_CHECK(hipStreamSynchronize(gpu().stream));
}
SpentSet::~SpentSet() { try { LaneScope lane(0); std::lock_guard<std::mutex> gl(g_gpu_mutex); impl.reset(); } catch (...) {} }
uint64_t SpentSet::size() const { std::lock_guard<std::mutex> lk(impl->mu); return impl->n; }
bool SpentSet::exempt_key(uint8_t out[20]) const { if (impl->has_exempt) memcpy(out, impl->exempt, 20); return impl->has_exempt; }   // (set once, by the constructor)

// One upload, at most one rebuild, three launches and one download, whatever n is.
bool SpentSet::spend(const uint8_t *keys, const uint8_t *mask, size_t n, bool commit, uint8_t *conflict, uint64_t *size_out) {
  Impl &d = *impl; std::lock_guard<std::mutex> lk(d.mu);
  if ((n && (!keys || !conflict)) || n >= KT_MAX_LOG || d.n + n >= KT_MAX_LOG) return false;
  if (!n) { if (size_out) *size_out = d.n; return true; }
  LaneScope lane(0); std::lock_guard<std::mutex> gl(g_gpu_mutex); hipStream_t s = gpu().stream;
  // a call's arrays, in words (byte arrays padded to words): keys 5n | active | err | won | conflict | winner | where n | counts.  Up: keys .. err (the word arrives
  // as zero).  Down: err .. conflict.
  const uint32_t per = cdiv(n, (size_t)KT_THREADS * SN_MAX_TILES), tiles = cdiv(n, (size_t)KT_THREADS * per); const size_t nw = (n + 3) / 4;
  const size_t o_active = KEY_WORDS * n, o_err = o_active + nw, o_won = o_err + 1, o_conf = o_won + 1, o_winner = o_conf + nw, o_where = o_winner + nw, o_counts = o_where + n, words = o_counts + tiles;
  d.pinned(4 * (o_err + 1)); uint8_t *act = d.pin + 4 * o_active; memset(act, 0, 4 * (nw + 1));
  for (size_t i = 0; i < n; i++) { const uint8_t *k = keys + 20 * i; memcpy(d.pin + 20 * i, k, 20); act[i] = (!mask || mask[i]) && !(d.has_exempt && !memcmp(k, d.exempt, 20)); }
  const uint32_t lg = d.slots_log_for(n); if (commit) d.reserve_log(d.n + n);
  grow_buf(d.work, words); uint32_t *W = d.work.get(); const uint32_t n_old = (uint32_t)d.n;
  DevBuf<uint32_t> fresh; SyncAtExit sync;                                                  // (declared before the guard: the stream is idle when `fresh` is let go)
  HIP_CHECK(hipMemcpyAsync(W, d.pin, 4 * (o_err + 1), hipMemcpyHostToDevice, s));
  // the table the call runs on: the set's own, or a rebuilt one — which replaces the set's only if the call commits: a check-only call leaves the set's table bit for bit
  if (lg) fresh = d.rebuilt(lg, W + o_err);
  const KeyTable T = lg ? d.handle(fresh.get(), lg) : d.table(); bool scratch_flag = false; Impl::Writing w(lg ? scratch_flag : d.damaged);
  hipLaunchKernelGGL(k_snset_probe, dim3(cdiv(n, KT_THREADS)), dim3(KT_THREADS), 0, s, T, (const uint32_t *)d.log.get(), n_old, (const uint32_t *)W, (const uint8_t *)(W + o_active), (uint32_t)n, W + o_where, W + o_err); Impl::launched();
  hipLaunchKernelGGL(k_snset_classify, dim3(tiles), dim3(KT_THREADS), 0, s, (const uint32_t *)T.slots, (const uint32_t *)(W + o_where), (uint32_t)n, n_old, per, (uint8_t *)(W + o_conf), (uint8_t *)(W + o_winner), W + o_counts); Impl::launched();
  hipLaunchKernelGGL(k_snset_finalize, dim3(tiles), dim3(KT_THREADS), 0, s, T.slots, d.log.get(), (const uint32_t *)(W + o_where), (const uint8_t *)(W + o_winner), (const uint32_t *)W, (uint32_t)n, n_old, per,
                     (const uint32_t *)(W + o_counts), commit ? 1 : 0, W + o_won); Impl::launched();
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpyAsync(d.pin, W + o_err, 4 * (2 + nw), hipMemcpyDeviceToHost, s)); HIP_CHECK(hipStreamSynchronize(s));
  uint32_t head[2]; memcpy(head, d.pin, 8); d.check_err(head[0], "spend", false);
  if (commit) { if (lg) d.adopt_slots(fresh, lg); d.n += head[1]; }
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
  if ((n && (!keys || !nkeys || !conflict)) || n >= KT_MAX_LOG / 2 || d.n + 2 * n >= KT_MAX_LOG) return false;   // n_old + 1 + e stays below the tombstone for every entry e < 2n
  for (size_t i = 0; i < n; i++) if (nkeys[i] > 2) return false;
  if (!n) { if (size_out) *size_out = d.n; return true; }
  LaneScope lane(0); std::lock_guard<std::mutex> gl(g_gpu_mutex); hipStream_t s = gpu().stream;
  // a call's arrays, in words (byte arrays padded to words): keys 10n | active 2n | status | code | head | win | hold 2n | where 2n | counts.  Up: keys .. head (the
  // head arrives as zero).  Down, after every round: status .. head.
  const uint32_t per = cdiv(n, (size_t)KT_THREADS * SN_MAX_TILES), tiles = cdiv(n, (size_t)KT_THREADS * per); const size_t nw = (n + 3) / 4, nw2 = (2 * n + 3) / 4;
  const size_t o_active = 2 * KEY_WORDS * n, o_status = o_active + nw2, o_code = o_status + nw, o_head = o_code + nw, o_win = o_head + SP_HEAD, o_hold = o_win + nw, o_where = o_hold + nw2,
               o_counts = o_where + 2 * n, words = o_counts + tiles;
  d.pinned(4 * o_win); uint8_t *act = d.pin + 4 * o_active, *status = d.pin + 4 * o_status, *code = d.pin + 4 * o_code; memset(act, 0, 4 * (o_win - o_active)); memcpy(d.pin, keys, 40 * n);
  for (size_t i = 0; i < n; i++) {
    const uint8_t *k = keys + 40 * i;
    act[2 * i] = nkeys[i] >= 1 && !(d.has_exempt && !memcmp(k, d.exempt, 20)); act[2 * i + 1] = nkeys[i] == 2;
    if (nkeys[i] == 2 && d.has_exempt && !memcmp(k + 20, d.exempt, 20)) { status[i] = SP_REJECTED; code[i] = 1; }   // the exempt key is never inserted, so as a second key it counts as spent
  }
  const uint32_t lg = d.slots_log_for(2 * n); if (commit) d.reserve_log(d.n + 2 * n);
  grow_buf(d.work, words); uint32_t *W = d.work.get(); const uint32_t n_old = (uint32_t)d.n;
  DevBuf<uint32_t> fresh; SyncAtExit sync;                                                  // (declared before the guard: the stream is idle when `fresh` is let go)
  HIP_CHECK(hipMemcpyAsync(W, d.pin, 4 * o_win, hipMemcpyHostToDevice, s));
  if (lg) fresh = d.rebuilt(lg, W + o_head + SP_ERR);                                               // as in spend: a rebuilt table replaces the set's only if the call commits
  const KeyTable T = lg ? d.handle(fresh.get(), lg) : d.table(); bool scratch_flag = false; Impl::Writing w(lg ? scratch_flag : d.damaged);
  const uint8_t *A = (const uint8_t *)(W + o_active), *H = (const uint8_t *)(W + o_hold), *WIN = (const uint8_t *)(W + o_win); uint8_t *ST = (uint8_t *)(W + o_status), *CO = (uint8_t *)(W + o_code);
  uint32_t head[SP_HEAD], rounds = 0; bool host_pass = false;
  for (;;) {
    hipLaunchKernelGGL(k_snset_pairs_probe, dim3(cdiv(2 * n, KT_THREADS)), dim3(KT_THREADS), 0, s, T, (const uint32_t *)d.log.get(), n_old, (const uint32_t *)W, A, (const uint8_t *)ST, (uint32_t)(2 * n), W + o_where, W + o_head); Impl::launched();
    hipLaunchKernelGGL(k_snset_pairs_wins, dim3(tiles), dim3(KT_THREADS), 0, s, (const uint32_t *)T.slots, (const uint32_t *)(W + o_where), A, (uint32_t)n, n_old, per, ST, CO, (uint8_t *)(W + o_win), (uint8_t *)(W + o_hold), W + o_counts, W + o_head); Impl::launched();
    if (!host_pass) { hipLaunchKernelGGL(k_snset_pairs_decide, dim3(cdiv(n, KT_THREADS)), dim3(KT_THREADS), 0, s, (const uint32_t *)T.slots, (const uint32_t *)(W + o_where), A, H, WIN, (uint32_t)n, n_old, ST, CO, W + o_head); Impl::launched(); }
    hipLaunchKernelGGL(k_snset_pairs_finish, dim3(tiles), dim3(KT_THREADS), 0, s, T.slots, d.log.get(), (const uint32_t *)(W + o_where), A, H, WIN, (const uint32_t *)W, (uint32_t)n, n_old, per, (const uint32_t *)(W + o_counts), commit ? 1 : 0, W + o_head); Impl::launched();
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
  if (commit) { if (lg) d.adopt_slots(fresh, lg); d.n += head[SP_WON]; d.tombs += head[SP_TOMBS]; }
  w.done();
  memcpy(conflict, code, n); if (size_out) *size_out = d.n;
  return true;
}
bool SpentSet::query(uint64_t size, const uint8_t *keys, size_t q, uint64_t *index, bool current) {
  Impl &d = *impl; std::lock_guard<std::mutex> lk(d.mu); if (current) size = d.n;
  if (size > d.n || (q && (!keys || !index)) || q >= KT_MAX_LOG) return false;
  if (!q) return true;
  LaneScope lane(0); std::lock_guard<std::mutex> gl(g_gpu_mutex); hipStream_t s = gpu().stream; d.repair();
  const size_t o_out = (KEY_WORDS * q + 1) & ~(size_t)1;                                            // (the answers are 64-bit words)
  d.pinned(std::max<size_t>(20 * q, 8 * q)); grow_buf(d.work, o_out + 2 * q); uint32_t *W = d.work.get(); memcpy(d.pin, keys, 20 * q);
  SyncAtExit sync;
  HIP_CHECK(hipMemcpyAsync(W, d.pin, 20 * q, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_snset_query, dim3(cdiv(q, KT_THREADS)), dim3(KT_THREADS), 0, s, d.table(), (const uint32_t *)d.log.get(), (uint32_t)size, (const uint32_t *)W, (uint32_t)q, (unsigned long long *)(W + o_out)); Impl::launched();
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
  hipLaunchKernelGGL(k_snset_unlink, dim3(cdiv(d.n - size, KT_THREADS)), dim3(KT_THREADS), 0, s, d.table(), (const uint32_t *)d.log.get(), (uint32_t)size, (uint32_t)d.n, d.err.get()); Impl::launched();
  HIP_CHECK(hipGetLastError()); d.check_err(d.own_err(), "rewind", true);
  d.tombs += d.n - size; d.n = size; w.done(); return true;
}
bool SpentSet::read_log(uint64_t first, uint64_t count, uint8_t *out) { return impl->read_log(first, count, out); }
void SpentSet::table(std::vector<uint32_t> &slots, uint64_t &seed, uint64_t &tombstones) { impl->read_slots(slots, seed, tombstones); }

}  // namespace zk
