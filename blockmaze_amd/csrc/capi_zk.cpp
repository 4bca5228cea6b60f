// The drop-in layer: the C symbols go-ethereum/zktx binds through cgo (include/zk_{common,mint,send,deposit,redeem}.h).
// Behavioural contract restated from libsnark-vnt/src/{mint,send,deposit,redeem}/*cgo.cpp:
//   * hex strings in, freshly allocated NUL-terminated hex strings out (the Go side never frees them);
//   * a witness that violates the circuit yields the hex of the default proof (G1::one, G2::one, G1::one), whose first
//     characters are "000000..." — the failure sentinel go-ethereum checks (internal/ethapi/api.go:1690);
//   * keys are looked up under /usr/local/prfKey/ (override: ZK_PRFKEY_DIR); unlike the reference they are parsed once
//     and kept resident in HBM, re-read only when the file's size or mtime changes;
//   * no exception, abort or signal handler ever crosses this boundary; calls may arrive concurrently on any thread.
#include <sys/random.h>
#include <sys/stat.h>
#include <unistd.h>
#include <cerrno>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <array>
#include <map>
#include <set>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include "../../include/zk_deposit.h"
#include "../../include/zk_mint.h"
#include "../../include/zk_redeem.h"
#include "../../include/zk_send.h"
#include "../../include/zk_batch.h"
#include "../../include/zk_block.h"
#include "../../include/zk_records.h"
#include "../../include/zk_tree.h"
#include "../../include/zk_tree_states.h"
#include "../../include/zk_roots.h"
#include "../../include/zk_spent.h"
#include "../../include/zk_proof_cache.h"
#include "../../include/zk_spent_pk.h"
#include "../../include/zk_tree_block.h"
#include "../../include/zk_tree_chain.h"
#include "../../include/zk_accounts.h"
#include "../../include/zk_accounts_chain.h"
#include "../../include/zkgpu.h"
#include "blockmaze_circuits.hpp"
#include "capi_accounts.hpp"
#include "groth16.hpp"

using namespace zk;
extern std::mutex g_gpu_mutex;
extern void zkgpu_set_error(const std::string &s);

namespace {
char *dup_string(const std::string &s) { char *p = (char *)malloc(s.size() + 1); if (p) memcpy(p, s.c_str(), s.size() + 1); return p; }
char *hash_out(const Blob256 &h) { return dup_string(blob_to_hex(h.b, 32)); }
std::string key_dir() { const char *e = getenv("ZK_PRFKEY_DIR"); return e && *e ? e : "/usr/local/prfKey"; }
// (the deposit circuit at a Merkle depth other than the reference's 8 has keys of its own: deposit<depth>pk.txt / deposit<depth>vk.txt)
std::string key_path(CircuitKind k, bool pk, size_t depth = 8) {
  return key_dir() + "/" + circuit_name(k) + (k == CircuitKind::Deposit && depth != 8 ? std::to_string(depth) : "") + (pk ? "pk.txt" : "vk.txt"); }

struct FileStamp { off_t size = -1; time_t mtime = 0; long mtime_ns = 0; bool operator==(const FileStamp &o) const {
    return size == o.size && mtime == o.mtime && mtime_ns == o.mtime_ns; } };
bool stamp_of(const std::string &p, FileStamp &s) {
  struct stat st;
  if (stat(p.c_str(), &st)) return false;
  s.size = st.st_size;
  s.mtime = st.st_mtim.tv_sec;
  s.mtime_ns = st.st_mtim.tv_nsec;
  return true;
}

// One proving key = a small pool of provers (ZK_PROVERS_PER_KEY, default 6), each with its own circuit board, device buffers and stream set: cgo calls
// that arrive concurrently (tx pool, RPC goroutines, block processing) overlap on the GPU instead of queueing behind one mutex.
// (tag_dev / wide_dev: the device's addresses of the board's two arrays, pinned and mapped once per unit — the hand-over's kernel reads them in place; null: staged)
struct ProverUnit { std::shared_ptr<Prover> prover; std::unique_ptr<Circuit> circuit; std::mutex busy; const uint8_t *tag_dev = nullptr; const Fe32 *wide_dev = nullptr;
  void map_board() { static const bool on = [] { const char *e = getenv("ZK_HANDOVER_MAPPED"); return !e || atoi(e) != 0; }(); if (!on) return;
    circuit::Board &b = circuit->board; tag_dev = (const uint8_t *)gpu_host_register(b.tag.data(), b.tag.size());
    wide_dev = tag_dev ? (const Fe32 *)gpu_host_register(b.wide.data(), b.wide.size() * sizeof(b.wide[0])) : nullptr;
    if (tag_dev && !wide_dev) { gpu_host_unregister(b.tag.data()); tag_dev = nullptr; } }
  ~ProverUnit() { if (circuit && tag_dev) { gpu_host_unregister(circuit->board.tag.data()); gpu_host_unregister(circuit->board.wide.data()); } } };
typedef std::vector<std::shared_ptr<ProverUnit>> UnitList;
// A reload (the key file's size or mtime changed) never touches the old list: it publishes a NEW one, and the old units die when the last proof running on them
// lets go of its reference — a caller can therefore never see a destroyed unit or mutex, however the reload interleaves with proofs in flight.
struct ProverSlot { FileStamp stamp; std::vector<std::shared_ptr<const UnitList>> units /* one list per device slot, built on first use */;
    std::vector<uint8_t> building /* a caller is loading this device's pool */; std::atomic<unsigned> next{0}; };
struct VkSlot { FileStamp stamp; std::shared_ptr<PreparedVerifyingKey> vk; std::shared_ptr<BatchVerifier> gpu;
  std::shared_ptr<BlockVerifier> block; int rlc_ok = -1 /* the key's check for the block equation (rlc_key_ok): -1 not made yet */;
  uint8_t tag[32] = {0} /* SHA-256 of the bytes `vk` was parsed from: the proof cache's name for this key */; };
std::mutex g_cache_mutex; std::map<std::string, ProverSlot> g_provers; std::map<std::string, VkSlot> g_vks;

std::unique_ptr<Circuit> make_circuit(CircuitKind k, bool emit, size_t depth = 8) {
  switch (k) {
    case CircuitKind::Mint: return make_mint_circuit(emit);
    case CircuitKind::Send: return make_send_circuit(emit);
    case CircuitKind::Redeem: return make_redeem_circuit(emit);
    default: return make_deposit_circuit(emit, depth);
  }
}

// after the first load from text: leave the container behind for the next process start (a read-only key directory simply goes without). `before` is the key
// file's stamp taken BEFORE it was read: the container is written under that stamp, and only if the file still carries it — a key replaced while it was being
// parsed must not leave the old key's tables behind under the new file's size and mtime.
void write_container_quietly(const std::string &pk_path, const ProvingKeyHost &pk, const FileStamp &before) {
  std::string cp = key_container_path(pk_path);
  FileStamp now;
  if (cp.empty() || pk.H_lagrange.empty() || pk.L_star.empty() || !stamp_of(pk_path, now) || !(now == before)) return;
  KeyStamp ks; ks.size = before.size; ks.mtime_s = before.mtime; ks.mtime_ns = before.mtime_ns;
  try { save_key_container(cp, pk, ks); } catch (const std::exception &) {} }
// A unit of the key's pool, locked for the caller (the reference keeps the unit alive, the lock is released first: members are destroyed in reverse order)
struct HeldUnit { std::shared_ptr<ProverUnit> unit; std::unique_lock<std::mutex> lock; };
}  // namespace
// Which device of the list (ZK_DEVICES) a gen*proof call goes to — pure logic, driven by the CPU tests through zkgpu_test_pool_plan. loaded[d]: device d holds
// a pool of this key; building[d]: some caller is loading one there right now; busy[d]: proofs running on it. Policy: the least busy loaded device; but as soon
// as every loaded device already runs `spill` proofs (default 1) and a device without a pool is left, that one is taken (the caller builds its pool: 0.1 s from
// the key's container) — a process that never has two proofs in flight keeps one copy of one key on one GPU, one with many concurrent callers spreads over all
// GPUs of the node before two proofs share a device. A pool that somebody else is building is never waited for while a loaded device exists. Returns the
// device; -1 = wait for a build to finish.
int zk_pool_pick_device(const uint8_t *loaded, const uint8_t *building, const int *busy, int D, int spill, unsigned turn) {
  int best = -1, fresh = -1; bool any_building = false;
  for (int i = 0; i < D; i++) {
    const int d = (int)((turn + (unsigned)i) % (unsigned)D);                            // ties go round by turn
    if (loaded[d]) { if (best < 0 || busy[d] < busy[best]) best = d; }
    else if (building[d]) any_building = true;
  }
  for (int d = 0; d < D && fresh < 0; d++) if (!loaded[d] && !building[d]) fresh = d;   // pools appear in list order
  if (best < 0) return fresh >= 0 && !any_building ? fresh : -1;                         // nothing loaded yet: the first caller builds, the others wait for it
  if (busy[best] >= spill && fresh >= 0) return fresh;
  return best;
}
namespace {
std::condition_variable g_pool_cv;   // signalled under g_cache_mutex whenever a pool build ends
// Loads the key on first use or when the file changed. g_cache_mutex guards the slot table only; a pool is BUILT outside it (under g_gpu_mutex, which
// serialises key loads and the other set-up work of the device), so callers that can be served by a loaded device never queue behind a key load. A prover's
// helper threads start with its first proof (groth16_prover.cpp).
HeldUnit acquire_prover(CircuitKind k, size_t depth = 8) {
  std::string path = key_path(k, true, depth); FileStamp st; if (!stamp_of(path, st)) throw std::runtime_error("proving key not found: " + path);
  const int D = std::max(1, gpu_device_slots());
  static const int spill = [] { const char *e = getenv("ZK_SPILL_BUSY"); int v = e ? atoi(e) : 1; return v < 1 ? 1 : v; }();
  std::shared_ptr<const UnitList> list; unsigned turn = 0;
  { std::unique_lock<std::mutex> lk(g_cache_mutex); ProverSlot &slot = g_provers[path];
    // (a changed key file: new lists; the old provers die with the last proof running on them)
    if ((int)slot.units.size() != D || !(slot.stamp == st)) {
      slot.units.assign(D, nullptr);
      slot.building.assign(D, 0);
      slot.stamp = st;
    }
    turn = slot.next.fetch_add(1);
    for (;;) {
      std::vector<uint8_t> loaded(D, 0); std::vector<int> busy(D, 0);
      for (int d = 0; d < D; d++) if (slot.units[d]) {
        loaded[d] = 1;
        for (auto &u : *slot.units[d]) {
          std::unique_lock<std::mutex> t(u->busy, std::try_to_lock);
          if (!t.owns_lock()) busy[d]++;
        }
      }
      const int dev = zk_pool_pick_device(loaded.data(), slot.building.data(), busy.data(), D, spill, turn);
      if (dev < 0) {
        g_pool_cv.wait(lk);
        if (!(slot.stamp == st)) throw std::runtime_error("proving key changed while it was being loaded: " + path);
        continue;
      }
      if (slot.units[dev]) { list = slot.units[dev]; break; }
      slot.building[dev] = 1; lk.unlock();
      std::shared_ptr<UnitList> fresh; std::exception_ptr err;
      try { std::lock_guard<std::mutex> gl(g_gpu_mutex);
        bool cached = false;
        ProvingKeyHost pk = load_proving_key_fast(path, cached);
        const char *e = getenv("ZK_PROVERS_PER_KEY");
        int n = e ? atoi(e) : 6;
        if (n < 1) n = 1;
        if (n > 7) n = 7;
        fresh = std::make_shared<UnitList>(); std::shared_ptr<Prover> first;
        for (int i = 0; i < n; i++) { auto u = std::make_shared<ProverUnit>();
          // the pool's members share the first one's device tables
          if (i == 0) {
            u->prover.reset(new Prover(pk, 0, 1, dev));
            first = u->prover;
          } else u->prover.reset(new Prover(*first));
          u->circuit = make_circuit(k, false, depth); u->map_board();
          if (u->circuit->board.num_variables() != u->prover->num_variables() ||
              u->circuit->num_inputs() != u->prover->num_inputs()) throw std::runtime_error("proving key does not belong to the " +
              std::string(circuit_name(k)) + " circuit: " + path);
          fresh->push_back(std::move(u)); }
        if (!cached) write_container_quietly(path, pk, st);
      } catch (...) { err = std::current_exception(); fresh.reset(); }
      lk.lock(); ProverSlot &again = g_provers[path];                                    // (std::map: the reference stays valid, looked up again for clarity)
      if (again.stamp == st && (int)again.building.size() == D) { again.building[dev] = 0; if (fresh) again.units[dev] = fresh; }
      g_pool_cv.notify_all();
      if (err) std::rethrow_exception(err);
      list = fresh; break;
    } }
  // first free member; otherwise wait for one (by turn)
  for (const auto &u : *list) { std::unique_lock<std::mutex> lk(u->busy, std::try_to_lock); if (lk.owns_lock()) return HeldUnit{u, std::move(lk)}; }
  const std::shared_ptr<ProverUnit> &u = (*list)[(turn / (unsigned)D) % list->size()]; return HeldUnit{u, std::unique_lock<std::mutex>(u->busy)};
}
// tag_out (may be null): the tag of the key that is returned, read under the same lock
std::shared_ptr<PreparedVerifyingKey> vk_for_path(const std::string &path, uint8_t *tag_out = nullptr) {
  FileStamp st; if (!stamp_of(path, st)) throw std::runtime_error("verification key not found: " + path);
  std::lock_guard<std::mutex> lk(g_cache_mutex); VkSlot &slot = g_vks[path];
  if (!slot.vk || !(slot.stamp == st)) {
    std::vector<uint8_t> bytes; std::shared_ptr<PreparedVerifyingKey> vk = prepare_verifying_key(load_verifying_key(path, &bytes));
    sha256(bytes.data(), bytes.size(), slot.tag); slot.vk = vk; slot.gpu.reset(); slot.block.reset(); slot.rlc_ok = -1; slot.stamp = st;
  }
  if (tag_out) memcpy(tag_out, slot.tag, 32);
  return slot.vk;
}
std::shared_ptr<PreparedVerifyingKey> vk_for(CircuitKind k) { return vk_for_path(key_path(k, false)); }
// the key's batched GPU verifier (kernel K9), built on first use; the caller holds g_gpu_mutex
std::shared_ptr<BatchVerifier> gpu_verifier_for_path(const std::string &path) {
  std::shared_ptr<PreparedVerifyingKey> vk = vk_for_path(path); std::lock_guard<std::mutex> lk(g_cache_mutex); VkSlot &slot = g_vks[path];
  if (!slot.gpu) slot.gpu = std::shared_ptr<BatchVerifier>(make_batch_verifier(vk->vk).release());
  return slot.gpu;
}
#ifdef ZKGPU_TEST_HOOKS
// test builds only (make TEST_HOOKS=1): ZK_FIXED_RS="<r hex>:<s hex>" makes proofs reproducible. The release library does not contain this code: an environment
// variable must never be able to remove the zero-knowledge property (the reference draws r, s from std::random_device, r1cs_gg_ppzksnark.tcc:418-419).
bool parse_fixed_rs(Fe32 &r, Fe32 &s) {
  const char *e = getenv("ZK_FIXED_RS"); if (!e) return false; const char *colon = strchr(e, ':'); if (!colon) return false;
  auto parse = [](const char *b, const char *en, Fe32 &o) {
    memset(&o, 0, sizeof o);
    int n = 0;
    for (const char *p = en; p-- > b;) {
      char ch = *p;
      int d = ch >= '0' && ch <= '9' ? ch - '0' : ch >= 'a' && ch <= 'f' ? ch - 'a' + 10 : -1;
      if (d < 0 || n >= 64) return false;
      o.l[n / 8] |= (uint32_t)d << (4 * (n % 8));
      n++;
    }
    return n > 0;
  };
  return parse(e, colon, r) && parse(colon + 1, e + strlen(e), s);
}
#else
inline bool parse_fixed_rs(Fe32 &, Fe32 &) { return false; }
#endif

// ---- one proof's MSMs cut over several GPUs behind the cgo symbols (kernel K7; round 5) --------------------------------------------------------------
// ZK_SHARD_DEVICES=k: every gen*proof call of the process runs on k shard provers — shard j holds the contiguous slice j of every query of the key on device slot
// j mod (number of device slots, ZK_DEVICES) —, each on a thread of its own: the assignment goes to every shard, each runs the replicated row / transform pipeline
// and its slice of the five MSMs (Prover::prove_partial: five partial sums, 384 bytes, written by the kernels into pinned host memory), the calling thread adds the
// k records and assembles the proof (finish_from_partials: host work only).  No collective, no torch: what a go-ethereum process can use.  It pays where one MSM is
// much longer than the latency floor of its tails (the deposit circuit at depth 32); for the four deployed circuits proof-level spreading (ZK_DEVICES) is faster.
// One proof at a time per key (the shard set is locked for the call).  On a box with one GPU all shards share it: the same code path, testable
// (tests/test_gpu_groth16.py::test_cgo_symbols_with_sharded_msms).
struct ShardSet { FileStamp stamp; std::vector<std::unique_ptr<Prover>> shards; std::unique_ptr<Circuit> circuit; std::mutex busy; };
std::mutex g_shard_mutex; std::map<std::string, std::shared_ptr<ShardSet>> g_shard_sets;
static size_t shard_count() { static const size_t k = [] { const char *e = getenv("ZK_SHARD_DEVICES"); long v = e ? atol(e) : 0; return (size_t)(v < 2 ? 0 : v > 64 ? 64 : v); }(); return k; }
static std::shared_ptr<ShardSet> shard_set_for(CircuitKind k, size_t depth = 8) {
  const std::string path = key_path(k, true, depth); FileStamp st; if (!stamp_of(path, st)) throw std::runtime_error("proving key not found: " + path);
  std::lock_guard<std::mutex> lk(g_shard_mutex); std::shared_ptr<ShardSet> &slot = g_shard_sets[path];
  if (!slot || !(slot->stamp == st)) {
    std::lock_guard<std::mutex> gl(g_gpu_mutex);
    bool cached = false; ProvingKeyHost pk = load_proving_key_fast(path, cached); const size_t K = shard_count(), D = (size_t)std::max(1, gpu_device_slots());
    auto fresh = std::make_shared<ShardSet>(); fresh->stamp = st; fresh->circuit = make_circuit(k, false, depth);
    for (size_t j = 0; j < K; j++) fresh->shards.emplace_back(new Prover(pk, j, K, (int)(j % D)));
    if (fresh->circuit->board.num_variables() != fresh->shards[0]->num_variables() || fresh->circuit->num_inputs() != fresh->shards[0]->num_inputs())
      throw std::runtime_error("proving key does not belong to the " + std::string(circuit_name(k)) + " circuit: " + path);
    if (!cached) write_container_quietly(path, pk, st);
    slot = fresh;
  }
  return slot;
}
// false: the assignment does not satisfy the constraint system
static bool prove_sharded(ShardSet &set, const Fe32 *r, const Fe32 *s, Proof &proof) {
  const size_t K = set.shards.size(); std::vector<uint8_t> rec(K * Prover::PARTIAL_BYTES); std::vector<uint8_t> ok(K, 0); std::vector<std::string> errs(K); std::vector<std::thread> th;
  const uint8_t *tag = set.circuit->board.tag.data(); const Fe32 *wide = reinterpret_cast<const Fe32 *>(set.circuit->board.wide.data());
  auto work = [&](size_t j) {
    try { set.shards[j]->set_witness_tagged(tag, wide); ok[j] = set.shards[j]->prove_partial(rec.data() + j * Prover::PARTIAL_BYTES) ? 1 : 0; }
    catch (const std::exception &e) { errs[j] = e.what(); } catch (...) { errs[j] = "unknown error"; } };
  // (a thread that cannot be started — the process is out of threads — must not leave its started siblings joinable when the vector dies: that would end the host
  // process; they are joined, then the error travels up like any other)
  try { for (size_t j = 1; j < K; j++) th.emplace_back(work, j); }
  catch (...) { for (auto &t : th) t.join(); throw; }
  work(0); for (auto &t : th) t.join();
  for (auto &e : errs) if (!e.empty()) throw std::runtime_error(e);
  for (size_t j = 0; j < K; j++) if (!ok[j]) return false;
  set.shards[0]->finish_from_partials(rec.data(), K, r, s, proof); return true;   // (r, s null: fresh randomness, drawn inside)
}

static std::atomic<int> g_proofs_in_flight{0};   // genXproof calls of this process that are between acquiring a prover and returning
// shared tail of the gen*proof functions: assign() has filled the circuit's board
template <class AssignFn> char *generate(CircuitKind k, AssignFn assign, size_t depth = 8) {
  try {
    if (!gpu_available()) {
      zkgpu_set_error("no HIP device visible; libzkgpu has no CPU fallback");
      fprintf(stderr, "libzkgpu: no HIP device visible, cannot generate %s proof\n", circuit_name(k));
      return dup_string(proof_to_hex(default_proof()));
    }
    static const bool trace = getenv("ZK_TRACE_TIMES") != nullptr;
    auto now = [] {
      return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
    };
    struct InFlight { InFlight() { g_proofs_in_flight.fetch_add(1, std::memory_order_relaxed); } ~InFlight() {
        g_proofs_in_flight.fetch_sub(1, std::memory_order_relaxed); } } in_flight;
    if (shard_count()) {
      std::shared_ptr<ShardSet> set = shard_set_for(k, depth); std::lock_guard<std::mutex> one(set->busy); assign(*set->circuit);
      printf("Trying to generate %s proof...\n", circuit_name(k)); fflush(stdout);
      Fe32 r, s; const bool fixed = parse_fixed_rs(r, s); Proof proof;
      if (!prove_sharded(*set, fixed ? &r : nullptr, fixed ? &s : nullptr, proof)) { printf("can not generate %s proof\n", circuit_name(k)); fflush(stdout); proof = default_proof(); }
      return dup_string(proof_to_hex(proof));
    }
    double t0 = now(); HeldUnit held = acquire_prover(k, depth); ProverUnit &slot = *held.unit; double t1 = now(); assign(*slot.circuit); double t2 = now();
    printf("Trying to generate %s proof...\n", circuit_name(k)); fflush(stdout);
    Fe32 r, s; bool fixed = parse_fixed_rs(r, s); Proof proof;
    // the board's own form (one byte per 0 / 1, Montgomery values for the rest): no conversion, no scan
    { const circuit::Board &bd = slot.circuit->board;
      slot.prover->set_witness_board(bd.tag.data(), reinterpret_cast<const Fe32 *>(bd.wide.data()), bd.ever_wide.data(), bd.wide_marks, slot.tag_dev, slot.wide_dev); }
    double t3 = now();
    if (!slot.prover->prove_resident(fixed ? &r : nullptr, fixed ? &s : nullptr, proof)) {
      fprintf(stderr, "libzkgpu: %s: the statement's assignment violates the constraint system (constraint %ld among others): no proof\n", circuit_name(k), slot.prover->last_failed_row);
      printf("can not generate %s proof\n", circuit_name(k));
      fflush(stdout);
      proof = default_proof();
    }
    double t4 = now(); char *out = dup_string(proof_to_hex(proof));
    if (trace) fprintf(stderr, "trace-abi: acquire %.3f witness %.3f upload %.3f prove %.3f hex %.3f ms\n", t1 - t0, t2 - t1, t3 - t2, t4 - t3, now() - t4);
    return out;
  }
  catch (const std::exception &e) {
    zkgpu_set_error(e.what());
    fprintf(stderr, "libzkgpu: %s\n", e.what());
    return dup_string(proof_to_hex(default_proof()));
  }
  catch (...) { zkgpu_set_error("unknown error"); return dup_string(proof_to_hex(default_proof())); }
}
// The verdicts for m proofs of ONE circuit kind — where every verification of the cgo layer ends up, the single-proof verifyXproof symbols (m = 1) and
// verifyBatch alike. From ZK_VERIFY_GPU_MIN proofs on (default 1: since kernel K9 keeps its values on 29-bit limbs a proof takes 2.1 ms on ONE compute unit of
// the device, 2.5 ms on a host core) the records go to the device in one launch — one workgroup per proof, concurrent callers on separate streams
// (gpu_verify.hip) —, otherwise, or when the process sees no device, to the prepared host verifier. res[j]: 1 accept, 0 reject. A record the device hands back
// (input accumulator at infinity) is decided by the host verifier.
#ifndef ZK_VERIFY_WHILE_PROVING_DEFAULT
#define ZK_VERIFY_WHILE_PROVING_DEFAULT true
#endif
void verify_group(CircuitKind kind, const Proof *ps, const uint8_t *parsed, const Fe32 *inputs, size_t ni, size_t m, uint8_t *res, size_t depth = 8) {
  static const size_t gpu_min = [] { const char *e = getenv("ZK_VERIFY_GPU_MIN"); long v = e ? atol(e) : 1; return (size_t)(v < 1 ? 1 : v); }();
  const std::string path = key_path(kind, false, depth);
  // A single proof also goes to the device while provers of this process are at work (round 6; rounds 3-5 sent it to the host verifier then: K9 took 2.1 ms idle and
  // 2.8 ms beside four provers, the host 1.87).  K9 now takes 0.74 ms and its waves run at priority 3: verifySendproof 0.85 ms on an idle GPU, 0.92 ms (median; p90 1.09)
  // beside one busy prover, 1.01 ms (p90 2.1) beside four, against 1.87-1.90 ms on a host core (profiles/r06_verify_under_load.txt).  ZK_VERIFY_WHILE_PROVING=0: the
  // host verifier while a proof is in flight, as before.
  bool decided = false;
  // (ZK_VERIFY_WHILE_PROVING: 1 = the device also while provers are at work, 0 = the host verifier then; measured again in round 6, profiles/r06_verify_under_load.txt)
  static const bool while_proving = [] { const char *e = getenv("ZK_VERIFY_WHILE_PROVING"); return e ? atoi(e) != 0 : ZK_VERIFY_WHILE_PROVING_DEFAULT; }();
  if (m >= gpu_min && (m >= 2 || while_proving || g_proofs_in_flight.load(std::memory_order_relaxed) == 0) && gpu_available()) {
    // The device may only ever be FASTER than the host verifier, never a different judge: anything that goes wrong on this branch — building the key's
    // verifier, an allocation, a launch or stream error, the test hook below — is logged and the whole group is decided by the prepared host verifier instead.
    // A transient GPU fault must not reject a valid transaction (the reference's verifier is pure host code, r1cs_gg_ppzksnark.tcc:584-590).
    try {
      // (tests: makes this branch throw, so that the fallback below is exercised on a healthy GPU)
      static const bool fail_hook = getenv("ZK_TEST_FAIL_GPU_VERIFY") != nullptr;
      if (fail_hook) throw std::runtime_error("ZK_TEST_FAIL_GPU_VERIFY is set");
      std::shared_ptr<BatchVerifier> v;
      { std::lock_guard<std::mutex> lk(g_gpu_mutex); v = gpu_verifier_for_path(path); }  // (building a key's verifier is serialised; using it is not)
      if (v->num_inputs() == ni) {
        std::vector<uint8_t> dev(m, 0); v->verify(ps, inputs, m, dev.data());            // (into a scratch vector: a throw half-way leaves `res` untouched)
        for (size_t j = 0; j < m; j++) res[j] = dev[j] == 2 ? (parsed[j] && verify_proof(*vk_for_path(path), inputs + j * ni, ni, ps[j])) : dev[j];
      // strong IC: a wrong input count rejects (r1cs_gg_ppzksnark.tcc:584-590)
      } else for (size_t j = 0; j < m; j++) res[j] = 0;
      decided = true;
    } catch (const std::exception &e) {
      static std::atomic<int> noted{0};
      if (noted.fetch_add(1, std::memory_order_relaxed) < 8) fprintf(stderr, "libzkgpu: GPU verifier failed (%s); deciding %zu proof(s) on the host\n",
          e.what(), m);
    }
  }
  if (!decided) {
    std::shared_ptr<PreparedVerifyingKey> vk = vk_for_path(path);
    for (size_t j = 0; j < m; j++) res[j] = parsed[j] && verify_proof(*vk, inputs + j * ni, ni, ps[j]);
  }
  for (size_t j = 0; j < m; j++) res[j] = parsed[j] && res[j] == 1;
}
bool verify(CircuitKind k, const char *data, const std::vector<bool> &public_bits, size_t depth = 8) {
  bool ok = false;
  try {
    Proof p;
    if (data && strnlen(data, 512) == 512 && proof_from_hex(data, p)) {
      std::vector<Fe32> inputs = pack_public_bits(public_bits);
      uint8_t parsed = 1, res = 0;
      verify_group(k, &p, &parsed, inputs.data(), inputs.size(), 1, &res, depth);
      ok = res == 1;
    }
  }
  catch (const std::exception &e) { zkgpu_set_error(e.what()); fprintf(stderr, "libzkgpu: %s\n", e.what()); ok = false; } catch (...) { ok = false; }
  printf("Verifying %s proof %s!!!\n", circuit_name(k), ok ? "successfully" : "unsuccessfully"); fflush(stdout); return ok;
}
void append(std::vector<bool> &v, const std::vector<bool> &w) { v.insert(v.end(), w.begin(), w.end()); }
// the statement of a proof as the verifier packs it (X_gadget::witness_map): args in the order of the kind's verifyXproof symbol
std::vector<bool> public_bits(CircuitKind k, const char *const *a, uint64_t value_s) {
  std::vector<bool> bits; auto h256 = [&](const char *s) { append(bits, blob_bits(blob256_from_hex(s ? s : "").b, 32)); };
  switch (k) {
    // cmtA_old, sn_old, cmtA, value_s (mint/circuit/gadget.tcc:252-269)
    case CircuitKind::Mint: case CircuitKind::Redeem: h256(a[0]);
    h256(a[1]);
    h256(a[2]);
    append(bits, u64_bits(value_s));
    break;
    // cmtA_old, sn_old, cmtS, cmtA_new (send/circuit/gadget.tcc:274-291)
    case CircuitKind::Send: h256(a[0]);
    h256(a[1]);
    h256(a[2]);
    h256(a[3]);
    break;
    // RT, pk, cmtb_old, sn_old, cmtb, sns (deposit/circuit/gadget.tcc:301-323)
    default: h256(a[0]);
    append(bits, blob_bits(blob160_from_hex(a[1] ? a[1] : "").b, 20));
    h256(a[2]);
    h256(a[3]);
    h256(a[4]);
    h256(a[5]);
    break;
  }
  return bits; }
}  // namespace

template <class Fn> static int guarded(Fn fn) {
  try {
    if (!gpu_available()) {
      zkgpu_set_error("no HIP device visible; libzkgpu has no CPU fallback");
      return ZKGPU_ERR_NO_DEVICE;
    }
    std::lock_guard<std::mutex> lk(g_gpu_mutex);
    return fn();
  }
  catch (const std::exception &e) {
    zkgpu_set_error(e.what());
    return ZKGPU_ERR_RUNTIME;
  }
  catch (...) {
    zkgpu_set_error("unknown error");
    return ZKGPU_ERR_RUNTIME;
  }
}
template <class Fn> static int guarded_host(Fn fn) {
  try {
    return fn();
  }
  catch (const std::exception &e) {
    zkgpu_set_error(e.what());
    return ZKGPU_ERR_RUNTIME;
  }
  catch (...) {
    zkgpu_set_error("unknown error");
    return ZKGPU_ERR_RUNTIME;
  }
}

// lanes: the extra prover objects of prove_batch (share p's tables), created on first use // proofs on different prover objects may run concurrently (each has
// its own streams); one object is used by one thread at a time
struct zkgpu_prover { std::shared_ptr<Prover> p; std::mutex m; std::vector<std::shared_ptr<Prover>> lanes; };
template <class Fn> static int guarded_prover(zkgpu_prover *h, Fn fn) {
  try {
    if (!gpu_available()) {
      zkgpu_set_error("no HIP device visible; libzkgpu has no CPU fallback");
      return ZKGPU_ERR_NO_DEVICE;
    }
    if (!h) return ZKGPU_ERR_ARG;
    std::lock_guard<std::mutex> lk(h->m);
    return fn();
  }
  catch (const std::exception &e) {
    zkgpu_set_error(e.what());
    return ZKGPU_ERR_RUNTIME;
  }
  catch (...) {
    zkgpu_set_error("unknown error");
    return ZKGPU_ERR_RUNTIME;
  }
}

// the resident commitment tree's handle.  The tree locks for itself (its own mutex, then the device mutex: gpu_tree.hip), so these entries do not go through guarded().
struct zkgpu_tree { CommitmentTree t; explicit zkgpu_tree(int depth) : t(depth) {} };
template <class Fn> static int guarded_tree(zkgpu_tree *t, Fn fn) {
  try {
    if (!gpu_available()) { zkgpu_set_error("no HIP device visible; libzkgpu has no CPU fallback"); return ZKGPU_ERR_NO_DEVICE; }
    if (!t) { zkgpu_set_error("no tree"); return ZKGPU_ERR_ARG; }
    return fn();
  }
  catch (const std::exception &e) { zkgpu_set_error(e.what()); return ZKGPU_ERR_RUNTIME; }
  catch (...) { zkgpu_set_error("unknown error"); return ZKGPU_ERR_RUNTIME; }
}

// the resident set of spent serial numbers: it locks for itself as the tree does (its own mutex, then the device mutex: gpu_snset.hip)
struct zkgpu_snset { SpentSet s; zkgpu_snset(const uint8_t *exempt, int log2_slots, const uint64_t *seed) : s(exempt, log2_slots, seed) {} };
template <class Fn> static int guarded_snset(zkgpu_snset *s, Fn fn) {
  try {
    if (!gpu_available()) { zkgpu_set_error("no HIP device visible; libzkgpu has no CPU fallback"); return ZKGPU_ERR_NO_DEVICE; }
    if (!s) { zkgpu_set_error("no spent set"); return ZKGPU_ERR_ARG; }
    return fn();
  }
  catch (const std::exception &e) { zkgpu_set_error(e.what()); return ZKGPU_ERR_RUNTIME; }
  catch (...) { zkgpu_set_error("unknown error"); return ZKGPU_ERR_RUNTIME; }
}
// the serial number a record spends, as the 32 bytes of its common.Hash: snold (args[3]) for deposit, args[1] for mint, send and redeem; the set's key is what
// common.BytesToAddress keeps of it, bytes 12..31
static const uint8_t *record_sn(const zk_block_record &r) { return r.kind == ZK_KIND_DEPOSIT ? r.args[3] : r.args[1]; }
// the proof cache's handle: it locks for itself (its own mutex, then a set's, then the device mutex: gpu_proof_cache.hip)
struct zkgpu_proof_cache { ProofCache c; zkgpu_proof_cache(uint64_t capacity, const uint8_t *salt) : c(capacity, salt) {} };
template <class Fn> static int guarded_cache(zkgpu_proof_cache *c, Fn fn) {
  try {
    if (!gpu_available()) { zkgpu_set_error("no HIP device visible; libzkgpu has no CPU fallback"); return ZKGPU_ERR_NO_DEVICE; }
    if (!c) { zkgpu_set_error("no proof cache"); return ZKGPU_ERR_ARG; }
    return fn();
  }
  catch (const std::exception &e) { zkgpu_set_error(e.what()); return ZKGPU_ERR_RUNTIME; }
  catch (...) { zkgpu_set_error("unknown error"); return ZKGPU_ERR_RUNTIME; }
}
typedef std::array<uint8_t, 20> SnKey20;
static SnKey20 sn_key20(const uint8_t *p) { SnKey20 k; memcpy(k.data(), p, 20); return k; }
void zk::snset_pairs_finish_host(const uint8_t *keys, const uint8_t *active, size_t n, uint8_t *status, uint8_t *code) {
  std::set<SnKey20> taken;
  for (size_t i = 0; i < n; i++) if (status[i] == 1) for (size_t j = 0; j < 2; j++) if (active[2 * i + j]) taken.insert(sn_key20(keys + 20 * (2 * i + j)));
  for (size_t i = 0; i < n; i++) {
    if (status[i] != 0) continue;
    const bool a0 = active[2 * i] != 0, a1 = active[2 * i + 1] != 0; const SnKey20 k0 = sn_key20(keys + 40 * i), k1 = sn_key20(keys + 40 * i + 20);
    if ((a0 && taken.count(k0)) || (a1 && taken.count(k1)) || (a0 && a1 && k0 == k1)) { status[i] = 2; code[i] = 2; continue; }
    status[i] = 1; if (a0) taken.insert(k0); if (a1) taken.insert(k1);
  }
}
static void sn_keys(const uint8_t *sns, size_t n, std::vector<uint8_t> &keys) { keys.resize(20 * n); for (size_t i = 0; i < n; i++) memcpy(&keys[20 * i], sns + 32 * i + 12, 20); }

extern "C" {
char *zkgpu_abi_genCMT(uint64_t value, char *sn_string, char *r_string) {
  return hash_out(note_cm(value, blob256_from_hex(sn_string), blob256_from_hex(r_string)));
}
char *zkgpu_abi_genCMTS(uint64_t value_s, char *pk_string, char *r_s_string, char *sn_old_string) {
  return hash_out(note_s_cm(value_s, blob160_from_hex(pk_string), blob256_from_hex(r_s_string), blob256_from_hex(sn_old_string)));
}
char *zkgpu_abi_computePRF(char *sk_string, char *r_string) { return hash_out(compute_prf(blob256_from_hex(sk_string), blob256_from_hex(r_string))); }
char *zkgpu_abi_computeCRH(char *pk_string, char *r_string) { return hash_out(compute_crh(blob160_from_hex(pk_string), blob256_from_hex(r_string))); }
// boost::array<uint256, 256> (depositcgo.cpp:304)
static std::vector<Blob256> parse_cmtarray(const char *cmtarray, int n) {
  std::vector<Blob256> leaves;
  std::string s = cmtarray ? cmtarray : "";
  if (n > 256) n = 256;
  for (int i = 0; i < n; i++) leaves.push_back(blob256_from_hex((size_t)i * 66 < s.size() ? s.substr((size_t)i * 66, 66).c_str() : "")); return leaves; }
char *zkgpu_abi_genRoot(char *cmtarray, int n) { return hash_out(merkle_root(parse_cmtarray(cmtarray, n), 8)); }

char *zkgpu_abi_genMintproof(uint64_t value, uint64_t value_old, char *sn_old, char *r_old, char *sn, char *r, char *cmtA_old, char *cmtA, uint64_t value_s,
    char *sk) {
  MintInputs in{value, value_old, value_s, blob256_from_hex(sn_old), blob256_from_hex(r_old), blob256_from_hex(sn), blob256_from_hex(r),
      blob256_from_hex(cmtA_old), blob256_from_hex(cmtA), blob256_from_hex(sk)};
  return generate(CircuitKind::Mint, [&](Circuit &c) { assign_mint(c, in); }); }
// mint_gadget::witness_map (mint/circuit/gadget.tcc:252-269)
bool zkgpu_abi_verifyMintproof(char *data, char *cmtA_old, char *sn_old, char *cmtA, uint64_t value_s) {
  const char *a[3] = {cmtA_old, sn_old, cmtA}; return verify(CircuitKind::Mint, data, public_bits(CircuitKind::Mint, a, value_s)); }
char *zkgpu_abi_genRedeemproof(uint64_t value, uint64_t value_old, char *sn_old, char *r_old, char *sn, char *r, char *cmtA_old, char *cmtA, uint64_t value_s,
    char *sk) {
  RedeemInputs in{value, value_old, value_s, blob256_from_hex(sn_old), blob256_from_hex(r_old), blob256_from_hex(sn), blob256_from_hex(r),
      blob256_from_hex(cmtA_old), blob256_from_hex(cmtA), blob256_from_hex(sk)};
  return generate(CircuitKind::Redeem, [&](Circuit &c) { assign_redeem(c, in); }); }
bool zkgpu_abi_verifyRedeemproof(char *data, char *cmtA_old, char *sn_old, char *cmtA, uint64_t value_s) {
  const char *a[3] = {cmtA_old, sn_old, cmtA}; return verify(CircuitKind::Redeem, data, public_bits(CircuitKind::Redeem, a, value_s)); }

static SendInputs send_inputs(uint64_t value_A, char *r_s, char *sn, char *r, char *cmt_s, char *cmtA, uint64_t value_s, char *pk_recv, uint64_t value_A_new,
    char *sn_A_new, char *r_A_new, char *cmt_A_new, char *sk, char *pk_sender) {
  SendInputs in;   // sendcgo.cpp:317-333: note_old = (value_A, sn, r), notes = (value_s, pk_recv, r_s, sn), note_new = (value_A_new, sn_A_new, r_A_new)
  in.value_old = value_A;
  in.value_s = value_s;
  in.value = value_A_new;
  in.sn_old = blob256_from_hex(sn);
  in.r_old = blob256_from_hex(r);
  in.r_s = blob256_from_hex(r_s);
  in.sn = blob256_from_hex(sn_A_new);
  in.r = blob256_from_hex(r_A_new);
  in.cmtA_old = blob256_from_hex(cmtA);
  in.cmtS = blob256_from_hex(cmt_s);
  in.cmtA = blob256_from_hex(cmt_A_new);
  in.sk = blob256_from_hex(sk);
  in.pk_recv = blob160_from_hex(pk_recv);
  in.pk_sender = blob160_from_hex(pk_sender);
  return in;
}
char *zkgpu_abi_genSendproof(uint64_t value_A, char *r_s, char *sn, char *r, char *cmt_s, char *cmtA, uint64_t value_s, char *pk_recv, uint64_t value_A_new,
    char *sn_A_new, char *r_A_new, char *cmt_A_new, char *sk, char *pk_sender) {
  SendInputs in = send_inputs(value_A, r_s, sn, r, cmt_s, cmtA, value_s, pk_recv, value_A_new, sn_A_new, r_A_new, cmt_A_new, sk, pk_sender);
  return generate(CircuitKind::Send, [&](Circuit &c) { assign_send(c, in); }); }
// send_gadget::witness_map (send/circuit/gadget.tcc:274-291)
bool zkgpu_abi_verifySendproof(char *data, char *cmtA_old, char *sn_old, char *cmtS, char *cmtA_new) {
  const char *a[4] = {cmtA_old, sn_old, cmtS, cmtA_new}; return verify(CircuitKind::Send, data, public_bits(CircuitKind::Send, a, 0)); }

// depositcgo.cpp:327-444: the Merkle path of cmtS is rebuilt from cmtarray (the tree holds the leaves up to and including the first occurrence of cmtS plus
// everything appended afterwards, i.e. all n leaves); RT is ignored and the root recomputed
// the statement's own fields; path, index_bits and rt come from the commitments (deposit_inputs) or from a resident tree (genDepositproofTree)
static DepositInputs deposit_fields(uint64_t value, uint64_t value_old, char *sn_old, char *r_old, char *sn, char *r, char *sns, char *rs, char *cmtB_old,
    char *cmtB, uint64_t value_s, char *pk, char *sn_A_old, char *cmtS, char *sk) {
  DepositInputs in;
  in.value = value;
  in.value_old = value_old;
  in.value_s = value_s;
  in.sn_old = blob256_from_hex(sn_old);
  in.r_old = blob256_from_hex(r_old);
  in.sn = blob256_from_hex(sn);
  in.r = blob256_from_hex(r);
  in.sn_s = blob256_from_hex(sns);
  in.r_s = blob256_from_hex(rs);
  in.cmtB_old = blob256_from_hex(cmtB_old);
  in.cmtB = blob256_from_hex(cmtB);
  in.cmtS = blob256_from_hex(cmtS);
  in.sk = blob256_from_hex(sk);
  in.pk_recv = blob160_from_hex(pk);
  in.sn_A_old = blob256_from_hex(sn_A_old);
  return in;
}
static DepositInputs deposit_inputs(uint64_t value, uint64_t value_old, char *sn_old, char *r_old, char *sn, char *r, char *sns, char *rs, char *cmtB_old,
    char *cmtB, uint64_t value_s, char *pk, char *sn_A_old, char *cmtS, char *cmtarray, int n, char *sk, size_t depth) {
  DepositInputs in = deposit_fields(value, value_old, sn_old, r_old, sn, r, sns, rs, cmtB_old, cmtB, value_s, pk, sn_A_old, cmtS, sk);
  std::vector<Blob256> leaves = parse_cmtarray(cmtarray, n);
  size_t index = 0;
  bool found = false;
  for (size_t i = 0; i < leaves.size(); i++) if (!memcmp(leaves[i].b, in.cmtS.b, 32)) {
    index = i;
    found = true;
    break;
  }
  // the reference throws out of IncrementalMerkleTree::path() here (IncrementalMerkleTree.tcc:214-216), taking the Go process with it
  if (!found) throw std::runtime_error("cmtS is not among the commitments of cmtarray");
  in.path = merkle_path(leaves, depth, index, in.index_bits); in.rt = merkle_root(leaves, depth); return in; }
char *zkgpu_abi_genDepositproof(uint64_t value, uint64_t value_old, char *sn_old, char *r_old, char *sn, char *r, char *sns, char *rs, char *cmtB_old,
    char *cmtB, uint64_t value_s, char *pk, char *sn_A_old, char *cmtS, char *cmtarray, int n, char *RT, char *sk) {
  (void)RT;
  return generate(CircuitKind::Deposit, [&](Circuit &c) { assign_deposit(c, deposit_inputs(value, value_old, sn_old, r_old, sn, r, sns, rs, cmtB_old, cmtB,
      value_s, pk, sn_A_old, cmtS, cmtarray, n, sk, 8)); });
}
// deposit_gadget::witness_map (deposit/circuit/gadget.tcc:301-323)
bool zkgpu_abi_verifyDepositproof(char *data, char *RT, char *pk, char *cmtb_old, char *snold, char *cmtb, char *sns) {
  const char *a[6] = {RT, pk, cmtb_old, snold, cmtb, sns}; return verify(CircuitKind::Deposit, data, public_bits(CircuitKind::Deposit, a, 0)); }

// ---- engine-level entry points for keys, circuits and the resident prover (include/zkgpu.h) ---------------------------
static void write_r1cs_file(const char *path, const R1csHost &cs) {
  FILE *f = fopen(path, "wb");
  if (!f) throw std::runtime_error(std::string("cannot write ") + path);
  uint64_t hdr[3] = {cs.n_inputs, cs.n_vars, cs.n_cons}; fwrite("R1CSBM01", 1, 8, f); fwrite(hdr, 8, 3, f);
  for (int m = 0; m < 3; m++) {
    uint64_t nnz = cs.col[m].size();
    fwrite(&nnz, 8, 1, f);
    fwrite(cs.rowptr[m].data(), 4, cs.rowptr[m].size(), f);
    fwrite(cs.col[m].data(), 4, nnz, f);
    fwrite(cs.coeff[m].data(), 32, nnz, f);
  }
  fclose(f);
}
static R1csHost read_r1cs_file(const char *path) {
  FILE *f = fopen(path, "rb");
  if (!f) throw std::runtime_error(std::string("cannot open ") + path);
  char mg[8];
  uint64_t hdr[3];
  R1csHost cs;
  if (fread(mg, 1, 8, f) != 8 || memcmp(mg, "R1CSBM01", 8) || fread(hdr, 8, 3, f) != 3) {
    fclose(f);
    throw std::runtime_error("bad R1CS file");
  }
  cs.n_inputs = hdr[0];
  cs.n_vars = hdr[1];
  cs.n_cons = hdr[2];
  for (int m = 0; m < 3; m++) {
    uint64_t nnz;
    if (fread(&nnz, 8, 1, f) != 1) {
      fclose(f);
      throw std::runtime_error("bad R1CS file");
    }
    cs.rowptr[m].resize(cs.n_cons + 1);
    cs.col[m].resize(nnz);
    cs.coeff[m].resize(nnz);
    if (fread(cs.rowptr[m].data(), 4, cs.n_cons + 1, f) != cs.n_cons + 1 || fread(cs.col[m].data(), 4, nnz, f) != nnz || fread(cs.coeff[m].data(), 32, nnz,
        f) != nnz) {
      fclose(f);
      throw std::runtime_error("truncated R1CS file");
    }
  }
  fclose(f);
  return cs;
}
static void write_witness_file(const char *path, const std::vector<Fe32> &z) {
  FILE *f = fopen(path, "wb");
  if (!f) throw std::runtime_error(std::string("cannot write ") + path);
  uint64_t n = z.size();
  fwrite(&n, 8, 1, f);
  fwrite(z.data(), 32, n, f);
  fclose(f);
}

int zkgpu_circuit_export(int kind, int tree_depth, const char *r1cs_path) {
  return guarded_host([&] { std::unique_ptr<Circuit> c = kind == 100 ? make_sha256_two_to_one(true) : kind == 101 ? make_merkle_test_circuit(true,
      tree_depth) : kind == 102 ? make_lesscmp_test_circuit(true) : kind == 103 ? make_cmta_test_circuit(true) : kind >= 104 && kind <= 106 ?
      make_hashblock_test_circuit(true, kind - 104) : kind == 107 ? make_unpacker_test_circuit(true, (size_t)tree_depth) : kind == (int)CircuitKind::Deposit ? make_deposit_circuit(true,
      tree_depth) : make_circuit((CircuitKind)kind, true); write_r1cs_file(r1cs_path, c->r1cs()); return ZKGPU_OK; });
}
/* bits: 64 + 256 + 256 bytes, each 0 or 1, in the circuit's bit order */
int zkgpu_witness_cmta(const uint8_t *bits, const char *wit_path) {
  return guarded_host([&] { auto c = make_cmta_test_circuit(false); std::vector<bool> v(bits, bits + 64), sn(bits + 64, bits + 320), r(bits + 320, bits + 576);
      assign_cmta_test(*c, v, sn, r); std::vector<Fe32> z; c->export_assignment(z); write_witness_file(wit_path, z); return ZKGPU_OK; });
}
/* which: 0 CMTS (736 input bits), 1 PRF (512), 2 CRH (416); bits: one byte (0 / 1) per input bit, in the block's message order */
int zkgpu_witness_hashblock(int which, const uint8_t *bits, const char *wit_path) { return guarded_host([&] {
    if (which < 0 || which > 2) throw std::runtime_error("hashblock: which must be 0, 1 or 2"); auto c = make_hashblock_test_circuit(false, which);
  assign_hashblock_test(*c, std::vector<bool>(bits, bits + hashblock_input_bits(which))); std::vector<Fe32> z; c->export_assignment(z);
      write_witness_file(wit_path, z); return ZKGPU_OK; }); }
/* bits: nbits bytes, each 0 or 1 */
int zkgpu_witness_unpacker(int nbits, const uint8_t *bits, const char *wit_path) {
  return guarded_host([&] { auto c = make_unpacker_test_circuit(false, (size_t)nbits); assign_unpacker_test(*c, std::vector<bool>(bits, bits + nbits)); std::vector<Fe32> z;
      c->export_assignment(z); write_witness_file(wit_path, z); return ZKGPU_OK; });
}
int zkgpu_witness_lesscmp(uint64_t value_old, uint64_t value_s, const char *wit_path) {
  return guarded_host([&] { auto c = make_lesscmp_test_circuit(false); assign_lesscmp_test(*c, value_old, value_s); std::vector<Fe32> z;
      c->export_assignment(z); write_witness_file(wit_path, z); return ZKGPU_OK; });
}
int zkgpu_witness_sha256(const uint8_t left[32], const uint8_t right[32], const char *wit_path) {
  return guarded_host([&] { auto c = make_sha256_two_to_one(false); assign_sha256_two_to_one(*c, blob_bits(left, 32), blob_bits(right, 32));
      std::vector<Fe32> z; c->export_assignment(z); write_witness_file(wit_path, z); return ZKGPU_OK; });
}
/* Merkle test circuit: leaf and depth siblings (leaf level first, 32 bytes each, in hashing byte order), position of the leaf; the root is computed */
int zkgpu_witness_merkle(int depth, const uint8_t leaf[32], const uint8_t *siblings, uint64_t position, const char *wit_path) { return guarded_host([&] {
    auto c = make_merkle_test_circuit(false, depth);
  Blob256 lf; memcpy(lf.b, leaf, 32); std::vector<Blob256> path(depth); std::vector<bool> idx(depth); Blob256 cur = lf;
  for (int d = 0; d < depth; d++) {
    memcpy(path[d].b, siblings + 32 * d, 32);
    idx[d] = (position >> d) & 1;
    Blob256 nx;
    if (idx[d]) sha256_compress_raw(path[d].b, cur.b, nx.b);
    else sha256_compress_raw(cur.b, path[d].b, nx.b);
    cur = nx;
  }
  assign_merkle_test(*c, lf, path, idx, cur); std::vector<Fe32> z; c->export_assignment(z); write_witness_file(wit_path, z); return ZKGPU_OK; }); }
int zkgpu_witness_deposit(uint64_t value, uint64_t value_old, char *sn_old, char *r_old, char *sn, char *r, char *sns, char *rs, char *cmtB_old, char *cmtB,
    uint64_t value_s, char *pk, char *sn_A_old, char *cmtS, char *cmtarray, int n, char *sk, int tree_depth, const char *wit_path) {
  return guarded_host([&] { DepositInputs in = deposit_inputs(value, value_old, sn_old, r_old, sn, r, sns, rs, cmtB_old, cmtB, value_s, pk, sn_A_old, cmtS,
      cmtarray, n, sk, (size_t)tree_depth);
    auto c = make_deposit_circuit(false, (size_t)tree_depth); assign_deposit(*c, in); std::vector<Fe32> z; c->export_assignment(z);
        write_witness_file(wit_path, z); return ZKGPU_OK; }); }
int zkgpu_witness_send(uint64_t value_A, char *r_s, char *sn, char *r, char *cmt_s, char *cmtA, uint64_t value_s, char *pk_recv, uint64_t value_A_new,
    char *sn_A_new, char *r_A_new, char *cmt_A_new, char *sk, char *pk_sender, const char *wit_path) {
  return guarded_host([&] { auto c = make_send_circuit(false); assign_send(*c, send_inputs(value_A, r_s, sn, r, cmt_s, cmtA, value_s, pk_recv, value_A_new,
      sn_A_new, r_A_new, cmt_A_new, sk, pk_sender)); std::vector<Fe32> z; c->export_assignment(z); write_witness_file(wit_path, z); return ZKGPU_OK; });
}
int zkgpu_witness_mint_redeem(int redeem, uint64_t value, uint64_t value_old, char *sn_old, char *r_old, char *sn, char *r, char *cmtA_old, char *cmtA,
    uint64_t value_s, char *sk, const char *wit_path) {
  return guarded_host([&] { MintInputs in{value, value_old, value_s, blob256_from_hex(sn_old), blob256_from_hex(r_old), blob256_from_hex(sn),
      blob256_from_hex(r), blob256_from_hex(cmtA_old), blob256_from_hex(cmtA), blob256_from_hex(sk)};
    auto c = redeem ? make_redeem_circuit(false) : make_mint_circuit(false);
    if (redeem) {
      RedeemInputs ri{in.value, in.value_old, in.value_s, in.sn_old, in.r_old, in.sn, in.r, in.cmtA_old, in.cmtA, in.sk};
      assign_redeem(*c, ri);
    } else assign_mint(*c, in);
    std::vector<Fe32> z; c->export_assignment(z); write_witness_file(wit_path, z); return ZKGPU_OK; }); }

int zkgpu_debug_time_send_witness(double out[3]) { return guarded_host([&] { auto now = [] {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  SendInputs in{};
  in.value_old = 22;
  in.value_s = 8;
  in.value = 14;
  double t0 = now();
  auto c = make_send_circuit(false);
  double t1 = now();
  assign_send(*c, in);
  double t2 = now();
  std::vector<Fe32> z;
  c->export_assignment(z);
  double t3 = now();
  assign_send(*c, in); double t4 = now(); out[0] = t1 - t0; out[1] = t4 - t3; out[2] = t3 - t2; return ZKGPU_OK; }); }
/* host only: the groups of variables with identical columns of an R1CS file, flattened as [size, members ...] per group; returns the number of words written (or needed) */
int zkgpu_test_equal_columns(const char *r1cs_path, uint32_t *out, size_t cap) { int res = 0; int rc = guarded_host([&] {
    if (!r1cs_path) return ZKGPU_ERR_ARG; const R1csHost cs = read_r1cs_file(r1cs_path); size_t at = 0;
    for (const auto &g : equal_column_groups(cs)) { if (out && at < cap) out[at] = (uint32_t)g.size(); at++; for (uint32_t v : g) { if (out && at < cap) out[at] = v; at++; } }
    res = (int)at; return ZKGPU_OK; }); return rc == ZKGPU_OK ? res : rc; }
int zkgpu_keygen_from_r1cs(const char *r1cs_path, uint64_t seed, const char *pk_path, const char *vk_path) { return guarded([&] {
    R1csHost cs = read_r1cs_file(r1cs_path); ProvingKeyHost pk; VerifyingKeyHost vk;
  generate_keys(cs, seed ? ToxicWaste::from_seed(seed) : ToxicWaste::random(), pk, vk); save_proving_key(pk_path, pk); save_verifying_key(vk_path, vk);
      return ZKGPU_OK; }); }
int zkgpu_keygen(int kind, int tree_depth, uint64_t seed, const char *pk_path, const char *vk_path) { return guarded([&] {
    std::unique_ptr<Circuit> c = kind == (int)CircuitKind::Deposit ? make_deposit_circuit(true, tree_depth) : make_circuit((CircuitKind)kind, true);
  ProvingKeyHost pk; VerifyingKeyHost vk; generate_keys(c->r1cs(), seed ? ToxicWaste::from_seed(seed) : ToxicWaste::random(), pk, vk);
      save_proving_key(pk_path, pk); save_verifying_key(vk_path, vk); return ZKGPU_OK; }); }

zkgpu_prover *zkgpu_prover_load_shard(const char *pk_path, size_t shard_rank, size_t shard_world) { zkgpu_prover *h = nullptr; guarded([&] { FileStamp before;
    if (!stamp_of(pk_path, before)) throw std::runtime_error(std::string("proving key not found: ") + pk_path); bool cached = false;
    ProvingKeyHost pk = load_proving_key_fast(pk_path, cached); std::unique_ptr<zkgpu_prover> p(new zkgpu_prover);
    p->p.reset(new Prover(pk, shard_rank, shard_world));
  if (!cached) write_container_quietly(pk_path, pk, before); h = p.release(); return ZKGPU_OK; }); return h; }
/* pure host logic of the multi-device pool, for the CPU tests: parses `spec` as ZK_DEVICES would be (n_visible devices, `fallback` = ZK_DEVICE / LOCAL_RANK) into out_devices (returns
 * the count), and writes into out_order the device that each of n_order callers arriving AT THE SAME TIME (nobody has finished yet) is sent to by acquire_prover's policy */
int zkgpu_test_device_plan(const char *spec, int n_visible, int fallback, int per_device, int *out_devices, int *out_order, int n_order) {
  std::vector<int> l = parse_device_list(spec, n_visible, fallback); for (size_t i = 0; i < l.size(); i++) out_devices[i] = l[i];
  const int D = std::max<int>(1, (int)l.size()); std::vector<int> rel(n_order, -1); (void)per_device;
  zkgpu_test_pool_plan(D, 1, rel.data(), n_order, out_order); return (int)l.size(); }
/* acquire_prover's device choice replayed on the host: call i first lets go of the proof that call release_before[i] started (-1: nobody finishes), then picks its device
 * (a pool that has to be built counts as loaded from then on).  out_dev[i] = the device slot.  Returns the number of pools built. */
int zkgpu_test_pool_plan(int D, int spill, const int *release_before, int n_calls, int *out_dev) {
  if (D < 1 || D > 64 || n_calls < 0) return -1;
  std::vector<uint8_t> loaded(D, 0), building(D, 0); std::vector<int> busy(D, 0); int built = 0;
  for (int i = 0; i < n_calls; i++) {
    const int r = release_before ? release_before[i] : -1; if (r >= 0 && r < i && out_dev[r] >= 0 && busy[out_dev[r]] > 0) busy[out_dev[r]]--;
    const int d = zk_pool_pick_device(loaded.data(), building.data(), busy.data(), D, spill < 1 ? 1 : spill, (unsigned)i); out_dev[i] = d; if (d < 0) return -1;
    if (!loaded[d]) { loaded[d] = 1; built++; } busy[d]++; }
  return built; }
/* the stream-lane planner of gpu.hip replayed on the host: n_slots devices whose pools are built one device at a time, `kinds` circuit kinds x per_kind members each taking
 * a lane.  Returns -1 if any member is left without a lane, else the largest number of provers sharing one lane; out_lanes_per_slot[d] = lanes bound to device slot d. */
int zkgpu_test_lane_plan(int n_slots, int kinds, int per_kind, int *out_lanes_per_slot) {
  return lane_plan_simulate(n_slots, kinds, per_kind, out_lanes_per_slot); }
/* the hand-over's block classifiers, scalar against the forms the host's CPU selects (AVX2 where it has it): see groth16_prover.cpp: test_scan_blocks */
int zkgpu_test_scan_blocks(const uint8_t *tags64, const uint64_t *elems64x4, const uint64_t *one4, uint64_t *out10) {
  return guarded_host([&] { test_scan_blocks(tags64, elems64x4, one4, out10); return ZKGPU_OK; });
}
/* the hand-over's scan pool (groth16_prover.cpp: ScanPool) driven from `callers` threads at once, host only: rounds that ran on the pool (>= 0), -1 if a chunk was counted twice or not at all */
int zkgpu_test_cgroup_quota(const char *root) { int out = -1; guarded_host([&] { out = test_cgroup_quota(root); return ZKGPU_OK; }); return out; }
int zkgpu_test_scan_pool(int callers, int rounds) { int out = -1; guarded_host([&] { out = test_scan_pool(callers, rounds); return ZKGPU_OK; }); return out; }
/* host-only self-test of the container code (tests/test_key_container_cpu.py): a synthetic transformed key of the given shape is written, mapped back and compared; then the
 * file is truncated, a payload byte is flipped, and the source stamp is changed — each must make the loader refuse.  Returns 0 if every step behaved. */
int zkgpu_test_key_container(const char *path, size_t n_vars, size_t n_cons, size_t m) { int rc = -1; guarded_host([&] {
  ProvingKeyHost pk;
  uint64_t s = 0x1234;
  auto rnd = [&](void *p, size_t n) {
    uint8_t *b = (uint8_t *)p;
    for (size_t i = 0; i < n; i++) {
      s = s * 6364136223846793005ull + 1442695040888963407ull;
      b[i] = (uint8_t)(s >> 56);
    }
  };
  pk.cs.n_inputs = 3;
  pk.cs.n_vars = n_vars;
  pk.cs.n_cons = n_cons;
  pk.A.resize(n_vars + 1);
  pk.L_star.resize(n_vars + 1);
  pk.H_lagrange.resize(m);
  size_t nB = n_vars / 2 + 1;
  pk.B_idx.resize(nB);
  pk.B_g1.resize(nB);
  pk.B_g2.resize(nB);
  rnd(&pk.alpha_g1, 64);
  rnd(&pk.beta_g1, 64);
  rnd(&pk.delta_g1, 64);
  rnd(&pk.beta_g2, 128);
  rnd(&pk.delta_g2, 128);
  rnd(pk.A.data(), pk.A.size() * 64);
  rnd(pk.L_star.data(), pk.L_star.size() * 64);
  rnd(pk.H_lagrange.data(), m * 64);
  rnd(pk.B_g1.data(), nB * 64);
  rnd(pk.B_g2.data(), nB * 128);
  for (size_t i = 0; i < nB; i++) pk.B_idx[i] = (uint32_t)(2 * i);
  for (int k = 0; k < 3; k++) {
    pk.cs.rowptr[k].resize(n_cons + 1);
    pk.cs.rowptr[k][0] = 0;
    for (size_t i = 0; i < n_cons; i++) pk.cs.rowptr[k][i + 1] = pk.cs.rowptr[k][i] + (uint32_t)((i + k) % 3);
    size_t nnz = pk.cs.rowptr[k][n_cons];
    pk.cs.col[k].resize(nnz);
    pk.cs.coeff[k].resize(nnz);
    for (size_t e = 0; e < nnz; e++) pk.cs.col[k][e] = (uint32_t)(e % (n_vars + 1));
    rnd(pk.cs.coeff[k].data(), nnz * 32);
  }
  KeyStamp st{12345, 1700000000, 42}; save_key_container(path, pk, st); ProvingKeyHost q;
  auto same = [&](const ProvingKeyHost &a, const ProvingKeyHost &b) {
    bool ok = !memcmp(&a.alpha_g1, &b.alpha_g1, 64) && !memcmp(&a.delta_g2, &b.delta_g2,
        128) && a.B_idx == b.B_idx && a.cs.n_cons == b.cs.n_cons && a.cs.n_vars == b.cs.n_vars && a.cs.n_inputs == b.cs.n_inputs;
    ok = ok && a.A.size() == b.A.size() && !memcmp(a.A.data(), b.A.data(), a.A.size() * 64) && a.L_star.size() == b.L_star.size() && !memcmp(a.L_star.data(),
        b.L_star.data(), a.L_star.size() * 64) && a.H_lagrange.size() == b.H_lagrange.size() && !memcmp(a.H_lagrange.data(), b.H_lagrange.data(),
        a.H_lagrange.size() * 64);
    ok = ok && a.B_g2.size() == b.B_g2.size() && !memcmp(a.B_g2.data(), b.B_g2.data(), a.B_g2.size() * 128) && !memcmp(a.B_g1.data(), b.B_g1.data(),
        a.B_g1.size() * 64);
    for (int k = 0; k < 3 && ok; k++) ok = a.cs.rowptr[k] == b.cs.rowptr[k] && a.cs.col[k] == b.cs.col[k] && a.cs.coeff[k].size() == b.cs.coeff[k].size() &&
        !memcmp(a.cs.coeff[k].data(), b.cs.coeff[k].data(), a.cs.coeff[k].size() * 32);
    return ok;
  };
  if (!load_key_container(path, st, q) || !same(pk, q)) { rc = 1; return ZKGPU_OK; }
  // the key file changed: stale
  KeyStamp other = st;
  other.mtime_ns++;
  if (load_key_container(path, other, q)) {
    rc = 2;
    return ZKGPU_OK;
  }
  struct stat sb; if (stat(path, &sb)) { rc = 3; return ZKGPU_OK; }
  // bit rot: checksum
  {
    FILE *f = fopen(path, "r+b");
    fseek(f, (long)(sb.st_size / 2), SEEK_SET);
    int ch = fgetc(f);
    fseek(f, (long)(sb.st_size / 2), SEEK_SET);
    fputc(ch ^ 1, f);
    fclose(f);
    if (load_key_container(path, st, q)) {
      rc = 4;
      return ZKGPU_OK;
    }
    f = fopen(path, "r+b");
    fseek(f, (long)(sb.st_size / 2), SEEK_SET);
    fputc(ch, f);
    fclose(f);
    if (!load_key_container(path, st, q)) {
      rc = 5;
      return ZKGPU_OK;
    }
  }
  // truncated
  if (truncate(path, sb.st_size - 64)) {
    rc = 6;
    return ZKGPU_OK;
  }
  if (load_key_container(path, st, q)) {
    rc = 7;
    return ZKGPU_OK;
  }
  rc = 0; return ZKGPU_OK; }); return rc; }
/* 1 if a valid container exists for this key file (what the next load will use), 0 if not */
int zkgpu_key_container_valid(const char *pk_path) {
  int r = 0;
  guarded_host([&] { KeyStamp ks; ProvingKeyHost pk; std::string cp = key_container_path(pk_path);
      r = !cp.empty() && key_stamp_of(pk_path, ks) && load_key_container(cp, ks, pk) ? 1 : 0; return ZKGPU_OK; });
  return r;
}
zkgpu_prover *zkgpu_prover_load(const char *pk_path) { return zkgpu_prover_load_shard(pk_path, 0, 1); }
int zkgpu_prover_prove_partial(zkgpu_prover *h, uint8_t out[384]) {
  return guarded_prover(h, [&] { if (!h) return ZKGPU_ERR_ARG; if (!h->p->prove_partial(out)) {
      zkgpu_set_error("assignment does not satisfy the constraint system (constraint " + std::to_string(h->p->last_failed_row) + " among those violated)"); return ZKGPU_ERR_UNSATISFIED; } return ZKGPU_OK; });
}
int zkgpu_prover_finish(zkgpu_prover *h, const uint8_t *records, size_t n, const uint8_t *r, const uint8_t *s, char proof_hex[513]) { return guarded_host([&] {
    if (!h) return ZKGPU_ERR_ARG; Proof p; h->p->finish_from_partials(records, n, (const Fe32 *)r, (const Fe32 *)s, p);
  std::string hx = proof_to_hex(p); memcpy(proof_hex, hx.c_str(), 513); return ZKGPU_OK; }); }
zkgpu_prover *zkgpu_prover_clone(zkgpu_prover *h) {
  zkgpu_prover *out = nullptr;
  guarded([&] { if (!h) return ZKGPU_ERR_ARG; std::unique_ptr<zkgpu_prover> p(new zkgpu_prover); p->p.reset(new Prover(*h->p)); out = p.release();
      return ZKGPU_OK; });
  return out;
}
int zkgpu_prover_prove_batch(zkgpu_prover *h, const uint8_t *zs, size_t n, const uint8_t *rs, char *proofs_hex) { return guarded_prover(h, [&] {
  if (!h || (n && (!zs || !proofs_hex))) return ZKGPU_ERR_ARG; if (!n) return ZKGPU_OK;
  static const size_t want = [] { const char *e = getenv("ZK_BATCH_LANES"); long v = e ? atol(e) : 6; return (size_t)(v < 1 ? 1 : v > 7 ? 7 : v); }();
  const size_t K = std::min(want, n);
  {
    std::lock_guard<std::mutex> lk(g_gpu_mutex);
    while (h->lanes.size() + 1 < K) h->lanes.push_back(std::make_shared<Prover>(*h->p));
  }
  const size_t zbytes = 32 * h->p->num_variables(); std::vector<uint8_t> bad(n, 0); std::vector<std::string> errs(K); std::vector<std::thread> th; std::atomic<size_t> next{0};
  auto work = [&](size_t lane) { Prover &pv = lane ? *h->lanes[lane - 1] : *h->p;
    try {
      // (the next statement nobody has taken: a lane that is slowed down — a preempted helper, the lane that shares its SIMDs with another's H accumulation —
      // simply takes fewer, and the batch ends when the last statement does, not when the unluckiest lane has worked off its fixed share)
      for (size_t i = next.fetch_add(1, std::memory_order_relaxed); i < n; i = next.fetch_add(1, std::memory_order_relaxed)) {
        Proof pr;
        const Fe32 *r = rs ? (const Fe32 *)(rs + 64 * i) : nullptr, *s_ = rs ? (const Fe32 *)(rs + 64 * i + 32) : nullptr;
        if (!pv.prove((const Fe32 *)(zs + zbytes * i), r, s_, pr)) {
          bad[i] = 1;
          pr = default_proof();
        }
        std::string hx = proof_to_hex(pr);
        memcpy(proofs_hex + 513 * i, hx.c_str(), 513);
      }
    }
    catch (const std::exception &e) { errs[lane] = e.what(); } catch (...) { errs[lane] = "unknown error"; } };
  for (size_t lane = 1; lane < K; lane++) th.emplace_back(work, lane);
  work(0); for (auto &t : th) t.join();
  for (auto &e : errs) if (!e.empty()) throw std::runtime_error(e);
  std::string which; for (size_t i = 0; i < n; i++) if (bad[i]) which += (which.empty() ? "" : ", ") + std::to_string(i);
  if (!which.empty()) { zkgpu_set_error("assignment does not satisfy the constraint system: batch record(s) " + which); return ZKGPU_ERR_UNSATISFIED; }
  return ZKGPU_OK; }); }
void zkgpu_prover_destroy(zkgpu_prover *h) { guarded([&] { delete h; return ZKGPU_OK; }); }
int zkgpu_prover_info(zkgpu_prover *h, size_t out[3]) {
  if (!h) return ZKGPU_ERR_ARG;
  out[0] = h->p->num_variables();
  out[1] = h->p->num_inputs();
  out[2] = h->p->domain_size();
  return ZKGPU_OK;
}
int zkgpu_prover_prove(zkgpu_prover *h, const uint8_t *z, const uint8_t *r, const uint8_t *s, char proof_hex[513]) { return guarded_prover(h, [&] {
    if (!h) return ZKGPU_ERR_ARG; Proof p;
  if (!h->p->prove((const Fe32 *)z, (const Fe32 *)r, (const Fe32 *)s, p)) { zkgpu_set_error("assignment does not satisfy the constraint system (constraint " + std::to_string(h->p->last_failed_row) + " among those violated)");
      return ZKGPU_ERR_UNSATISFIED; } std::string hx = proof_to_hex(p); memcpy(proof_hex, hx.c_str(), 513); return ZKGPU_OK; }); }
int zkgpu_prover_set_witness(zkgpu_prover *h, const uint8_t *z) {
  return guarded_prover(h, [&] { if (!h) return ZKGPU_ERR_ARG; h->p->set_witness((const Fe32 *)z, false); gpu_sync(); return ZKGPU_OK; });
}
int zkgpu_prover_prove_resident(zkgpu_prover *h, const uint8_t *r, const uint8_t *s, char proof_hex[513]) { return guarded_prover(h, [&] {
    if (!h) return ZKGPU_ERR_ARG; Proof p;
  if (!h->p->prove_resident((const Fe32 *)r, (const Fe32 *)s, p)) { zkgpu_set_error("assignment does not satisfy the constraint system (constraint " + std::to_string(h->p->last_failed_row) + " among those violated)");
      return ZKGPU_ERR_UNSATISFIED; } std::string hx = proof_to_hex(p); memcpy(proof_hex, hx.c_str(), 513); return ZKGPU_OK; }); }
int zkgpu_prover_stash_witness(zkgpu_prover *h, uint32_t *slot) {
  return guarded_prover(h, [&] { if (!h || !slot) return ZKGPU_ERR_ARG; *slot = (uint32_t)h->p->stash_witness(); return ZKGPU_OK; });
}
int zkgpu_prover_drop_stash(zkgpu_prover *h, uint32_t slot) {
  return guarded_prover(h, [&] { if (!h) return ZKGPU_ERR_ARG; h->p->drop_stash(slot == 0xffffffffu ? (size_t)-1 : (size_t)slot); return ZKGPU_OK; });
}
/* process-wide: how often a fast MSM path raised its flag and the MSM was repeated on the general path (soak runs, tests) */
uint64_t zkgpu_general_path_repeats(void) { return general_path_repeats(); }
uint64_t zkgpu_queries_without_tables(void) { return queries_without_tables(); }
int zkgpu_prover_equal_column_groups(zkgpu_prover *h, uint32_t *count) { if (!h || !count) return ZKGPU_ERR_ARG; *count = (uint32_t)h->p->equal_column_groups(); return ZKGPU_OK; }
int zkgpu_prover_read_stash(zkgpu_prover *h, uint32_t slot, uint8_t *z_out) {
  return guarded_prover(h, [&] { if (!h || !z_out) return ZKGPU_ERR_ARG; h->p->read_stash(slot, (Fe32 *)z_out); return ZKGPU_OK; });
}
int zkgpu_prover_stash_count(zkgpu_prover *h, uint32_t *count) {
  if (!h || !count) return ZKGPU_ERR_ARG;
  *count = (uint32_t)h->p->stash_count(); return ZKGPU_OK;
}
int zkgpu_prover_prove_stashed(zkgpu_prover *h, uint32_t slot, const uint8_t *r, const uint8_t *s, char proof_hex[513]) { return guarded_prover(h, [&] {
    if (!h) return ZKGPU_ERR_ARG; Proof p;
  if (!h->p->prove_stashed(slot, (const Fe32 *)r, (const Fe32 *)s, p)) { zkgpu_set_error("assignment does not satisfy the constraint system (constraint " + std::to_string(h->p->last_failed_row) + " among those violated)");
      return ZKGPU_ERR_UNSATISFIED; } std::string hx = proof_to_hex(p); memcpy(proof_hex, hx.c_str(), 513); return ZKGPU_OK; }); }
int zkgpu_prover_timings(zkgpu_prover *h, double out[5]) {
  if (!h) return ZKGPU_ERR_ARG;
  out[0] = h->p->last.upload_ms;
  out[1] = h->p->last.qap_ms;
  out[2] = h->p->last.msm_ms;
  out[3] = h->p->last.finish_ms;
  out[4] = h->p->last.total_ms;
  return ZKGPU_OK;
}
int zkgpu_profile_enable(int on) { return guarded([&] { profile_enable(on != 0); return ZKGPU_OK; }); }
int zkgpu_profile_report(char *buf, size_t cap) {
  return guarded([&] { std::string r = profile_report(); if (r.size() + 1 > cap) return ZKGPU_ERR_ARG; memcpy(buf, r.c_str(), r.size() + 1); return ZKGPU_OK;
      });
}
// host verifier on the prepared key (cached by the file's size and mtime)
int zkgpu_verify(const char *vk_path, const char *proof_hex, const uint8_t *inputs, size_t n_inputs) { int res = 0; int rc = guarded_host([&] {
    std::shared_ptr<PreparedVerifyingKey> vk = vk_for_path(vk_path); Proof p;
  if (!proof_hex || strnlen(proof_hex, 512) < 512 || !proof_from_hex(proof_hex, p)) { res = 0; return ZKGPU_OK;
      } res = verify_proof(*vk, (const Fe32 *)inputs, n_inputs, p) ? 1 : 0; return ZKGPU_OK; }); return rc == ZKGPU_OK ? res : rc; }
/* test entry: the decision of the GPU verifier's schedule (verify_sched.hpp), interpreted on the HOST — no device needed; stats[8] (optional): rounds, slots, products, linear operations, constants, rounds of products / eight-lane sums / one-lane sums */
int zkgpu_test_verify_schedule(const char *vk_path, const char *proof_hex, const uint8_t *inputs, size_t n_inputs, uint32_t *stats) { int res = 0;
    int rc = guarded_host([&] { std::shared_ptr<PreparedVerifyingKey> vk = vk_for_path(vk_path); Proof p;
  if (!proof_hex || strnlen(proof_hex, 512) < 512 || !proof_from_hex(proof_hex, p)) { res = 0; return ZKGPU_OK;
      } res = verify_by_schedule_on_host(*vk, (const Fe32 *)inputs, n_inputs, p, stats) ? 1 : 0; return ZKGPU_OK; }); return rc == ZKGPU_OK ? res : rc; }
/* small verification calls taken by the key's GPU verifier / launches made for them (calls that meet share a launch) */
int zkgpu_verify_counters(const char *vk_path, uint64_t out[2]) { return guarded([&] { if (!vk_path || !out) return ZKGPU_ERR_ARG; gpu_verifier_for_path(vk_path)->counters(out); return ZKGPU_OK; }); }
/* test entry: small calls, launches for them, launches of the workgroup-per-proof branch (65 to ZK_VERIFY_WAVE_MAX proofs), launches of the lane-per-proof branch */
int zkgpu_verify_path_counters(const char *vk_path, uint64_t out[4]) { return guarded([&] { if (!vk_path || !out) return ZKGPU_ERR_ARG; gpu_verifier_for_path(vk_path)->path_counters(out); return ZKGPU_OK; }); }
/* test entry (GPU): kernel K9's values after every `every`-th round of its schedule against the host model of the same limb arithmetic.  out[0] = first differing round or -1,
 * out[1] = the slot, out[2] = the kernel's verdict (1 accept, 0 reject, 2 handed back) */
int zkgpu_test_verify_trace(const char *vk_path, const char *proof_hex, const uint8_t *inputs, size_t n_inputs, uint32_t every, long out[3]) { return guarded([&] {
  if (!vk_path || !proof_hex || !out || !every) return ZKGPU_ERR_ARG; Proof p; if (strnlen(proof_hex, 512) < 512 || !proof_from_hex(proof_hex, p)) return ZKGPU_ERR_ARG;
  std::shared_ptr<BatchVerifier> v = gpu_verifier_for_path(vk_path); std::shared_ptr<PreparedVerifyingKey> vk = vk_for_path(vk_path); uint32_t slot = 0; uint8_t ok = 0;
  out[0] = verify_schedule_trace_on_device(*v, *vk, (const Fe32 *)inputs, n_inputs, p, every, &slot, &ok); out[1] = slot; out[2] = ok; return ZKGPU_OK; }); }
// batched verification on the GPU (kernel K9).  proofs_hex: n * 512 characters; inputs: n * n_inputs canonical field elements; ok[i] = 1 accept / 0 reject
// (a record that is not 512 hex digits is rejected without reaching the device; coordinates are taken modulo q like proof_from_hex in zkgpu_verify)
int zkgpu_verify_batch(const char *vk_path, const char *proofs_hex, const uint8_t *inputs, size_t n_inputs, size_t n, uint8_t *ok) { return guarded([&] {
  if (!vk_path || (!proofs_hex && n) || !ok) return ZKGPU_ERR_ARG;
  struct { std::shared_ptr<BatchVerifier> v; } slot{gpu_verifier_for_path(vk_path)};                                  // caller holds the device mutex (guarded)
  // strong IC: wrong input count rejects (r1cs_gg_ppzksnark.tcc:584-590)
  if (slot.v->num_inputs() != n_inputs) {
    for (size_t i = 0; i < n; i++) ok[i] = 0;
    return ZKGPU_OK;
  }
  std::vector<Proof> ps(n); std::vector<uint8_t> parsed(n);
  for (size_t i = 0; i < n; i++) {
    parsed[i] = strnlen(proofs_hex + 512 * i, 512) == 512 && proof_from_hex(proofs_hex + 512 * i, ps[i]);
    if (!parsed[i]) memset(&ps[i], 0, sizeof(Proof));
  }
  slot.v->verify(ps.data(), (const Fe32 *)inputs, n, ok);
  // 2: input accumulator at infinity, the host verifier decides (pairing.cuh)
  for (size_t i = 0; i < n; i++) {
    if (!parsed[i]) ok[i] = 0;
    else if (ok[i] == 2) ok[i] = verify_proof(*vk_for_path(vk_path), (const Fe32 *)inputs + i * n_inputs, n_inputs, ps[i]) ? 1 : 0;
  }
  return ZKGPU_OK; }); }
// ---- verifyBatch: the optional batch entry of include/zk_batch.h --------------------------------------------------- go-ethereum checks
// every ZK transaction twice, once in the pool and once in the block (core/tx_pool.go:612-645, core/state_processor.go:106-163), one cgo call and one key load
// per proof. A block's worth of proofs in ONE call is what the GPU verifier is for (kernel K9: one workgroup per proof interpreting the operation schedule of
// verify_sched.hpp on 29-bit limbs — 2.1 ms per launch up to 256 proofs, 31,000 proofs/s at 64, 124,000 at 512): the records are grouped by circuit kind and
// every group goes through verify_group above, exactly like the kind's verifyXproof symbol.
int verifyBatch(const zk_verify_item *items, int n, unsigned char *ok) {
  if (n < 0 || (n && (!items || !ok))) return -1;
  try {
    int accepted = 0; std::vector<int> idx[4];
    for (int i = 0; i < n; i++) { ok[i] = 0; if (items[i].kind >= 0 && items[i].kind <= 3) idx[items[i].kind].push_back(i); }
    for (int k = 0; k < 4; k++) { if (idx[k].empty()) continue; const CircuitKind kind = (CircuitKind)k; const size_t m = idx[k].size();
      std::vector<Proof> ps(m); std::vector<uint8_t> parsed(m), res(m, 0); std::vector<Fe32> inputs; size_t ni = 0;
      for (size_t j = 0; j < m; j++) {
        const zk_verify_item &it = items[idx[k][j]];
        parsed[j] = it.proof && strnlen(it.proof, 512) == 512 && proof_from_hex(it.proof, ps[j]);
        if (!parsed[j]) memset(&ps[j], 0, sizeof(Proof));
        std::vector<Fe32> in = pack_public_bits(public_bits(kind, it.args, it.value_s)); ni = in.size(); inputs.insert(inputs.end(), in.begin(), in.end()); }
      verify_group(kind, ps.data(), parsed.data(), inputs.data(), ni, m, res.data());
      for (size_t j = 0; j < m; j++) { ok[idx[k][j]] = res[j]; accepted += res[j]; } }
    return accepted;
  }
  catch (const std::exception &e) {
    zkgpu_set_error(e.what());
    fprintf(stderr, "libzkgpu: verifyBatch: %s\n", e.what());
    for (int i = 0; i < n; i++) ok[i] = 0;
    return -1;
  }
  catch (...) { for (int i = 0; i < n; i++) ok[i] = 0; return -1; }
}

// ---- the randomized block check (DESIGN.md "Block verification"; include/zk_block.h, zkgpu_verify_batch_rlc) ------------------------------------------------
// One equation over all records of a call, FE(prod_i Miller(A_i, B_i)^{r_i} * Miller(-S_acc, gamma) * Miller(-S_C, delta)) == alpha_g1_beta_g2^{sum r_i}; when it
// fails, or cannot be formed, every record is decided by the per-proof path and the verdicts are verifyBatch's.  Below RLC_MIN_RECORDS records (of a call, or
// of one kind in a block) the per-proof path is taken at once: the lane-per-record kernel has a floor of about 15 ms that the per-proof kernel K9 undercuts on
// small calls.  profiles/verify_block.txt: in device time the crossover lies between 4,096 records (K9 12.4 ms, block kernels 15.1) and 6,144 (18.4 against
// 15.2); the equation's host work (S_acc, the closing Miller loops and final exponentiation) adds a few ms a call, and 8,192 is the smallest measured size at
// which the call is faster in device and in wall time alike — a conservative bound.
static const size_t RLC_MIN_RECORDS = 8192;
static std::atomic<uint64_t> g_rlc_passed{0}, g_rlc_failed{0}, g_rlc_per_proof{0};
namespace {
// the key's device half of the check, null if the key fails rlc_key_ok (its calls are then decided proof by proof)
static std::shared_ptr<BlockVerifier> block_verifier_for_path(const std::string &path) {
  std::shared_ptr<PreparedVerifyingKey> vk = vk_for_path(path); std::lock_guard<std::mutex> lk(g_cache_mutex); VkSlot &slot = g_vks[path];
  if (slot.rlc_ok < 0) slot.rlc_ok = rlc_key_ok(*vk) ? 1 : 0;
  if (slot.rlc_ok == 1 && !slot.block) slot.block = std::shared_ptr<BlockVerifier>(make_block_verifier(*vk).release());
  return slot.rlc_ok == 1 ? slot.block : nullptr;
}
static bool is_zero_weight(const uint8_t *w) { for (int k = 0; k < 16; k++) if (w[k]) return false; return true; }
static void random_bytes(uint8_t *p, size_t n) {
  for (size_t got = 0; got < n;) { const ssize_t k = getrandom(p + got, n - got, 0); if (k < 0) { if (errno == EINTR) continue; throw std::runtime_error("getrandom failed"); } got += (size_t)k; }
}
// r_i uniform in [1, 2^128) from getrandom(2): a draw of 0 is drawn again
static void fresh_weights(uint8_t *w, size_t n) {
  random_bytes(w, 16 * n);
  for (size_t i = 0; i < n; i++) while (is_zero_weight(w + 16 * i)) random_bytes(w + 16 * i, 16);
}
// one key's share of the equation: the device half, then S_acc on the host.  false: this key cannot take part (it fails rlc_key_ok).  in_eq: records flagged 1
// (from records: `sums` = the device's integer sums, `handed` = the records flagged 2 with their device-made proof and inputs, for verify_proof)
struct RlcHanded { size_t i; Proof p; std::vector<Fe32> in; };
struct RlcPart { std::vector<uint8_t> flags; host::HFq12 prod; host::HG1 s_acc, s_c; uint64_t s[4]; size_t in_eq = 0; std::vector<uint64_t> sums; std::vector<RlcHanded> handed; };
static bool rlc_part(const std::string &path, const Proof *ps, const Fe32 *inputs, size_t ni, size_t m, const uint8_t *w, bool lock, RlcPart &out) {
  std::unique_lock<std::mutex> gl(g_gpu_mutex, std::defer_lock); if (lock) gl.lock();
  std::shared_ptr<BlockVerifier> bv = block_verifier_for_path(path); if (!bv) return false;
  if (bv->num_inputs() != ni) throw std::runtime_error("block verify: input count");
  out.flags.assign(m, 0); out.handed.clear(); bv->run(ps, inputs, w, m, out.flags.data(), out.prod, out.s_c); if (lock) gl.unlock();
  for (size_t i = 0; i < m; i++) if (out.flags[i] == 2) out.handed.push_back(RlcHanded{i, ps[i], std::vector<Fe32>(inputs + i * ni, inputs + (i + 1) * ni)});
  out.s_acc = rlc_acc_sum(*vk_for_path(path), inputs, ni, w, out.flags.data(), m, out.s);
  out.in_eq = 0; for (size_t i = 0; i < m; i++) out.in_eq += out.flags[i] == 1;
  return true;
}
// verdicts of a part whose equation held: the screen's rejections, the per-proof host verifier for an accumulator at infinity (the records in `handed`).  parsed: one
// byte a record, or null where the `parsed` byte is part of the device's screen already (calls from records: a record flagged 1 or 2 is a parsed one)
static void decide_from_flags(const std::string &path, const RlcPart &p, const uint8_t *parsed, size_t ni, size_t m, uint8_t *res) {
  for (size_t i = 0; i < m; i++) res[i] = (!parsed || parsed[i]) && p.flags[i] == 1 ? 1 : 0;
  for (const RlcHanded &h : p.handed) res[h.i] = (!parsed || parsed[h.i]) && verify_proof(*vk_for_path(path), h.in.data(), ni, h.p) ? 1 : 0;
}
// The engine entries' decision, shared by zkgpu_verify_batch_rlc and zkgpu_verify_records_rlc: from RLC_MIN_RECORDS records on the equation (`part` makes the call's
// device half), otherwise or if it fails, cannot be formed or throws, `per_proof` (exactly zkgpu_verify_batch).  The caller holds the device mutex.
extern "C++" {
template <class Part, class PerProof> static int rlc_engine_call(const char *vk_path, const uint8_t *parsed, size_t ni, size_t n, uint8_t *ok, uint32_t *by_equation,
    Part part, PerProof per_proof) {
  bool decided = false;
  if (n >= RLC_MIN_RECORDS) {
    try {
      RlcPart p;
      if (part(p) && p.in_eq && !p.s_acc.is_inf() && !p.s_c.is_inf()) {
        const bool pass = host::final_exponentiation(rlc_lhs(*vk_for_path(vk_path), p.prod, p.s_acc, p.s_c)) == rlc_rhs(*vk_for_path(vk_path), p.s);
        (pass ? g_rlc_passed : g_rlc_failed).fetch_add(1);
        if (pass) { decide_from_flags(vk_path, p, parsed, ni, n, ok); decided = true; }
      }
    } catch (const std::exception &e) { fprintf(stderr, "libzkgpu: block check failed (%s); deciding %zu proof(s) one by one\n", e.what(), n); }
  }
  if (!decided) { g_rlc_per_proof.fetch_add(1); per_proof(); }
  if (by_equation) *by_equation = decided ? 1 : 0;
  return ZKGPU_OK;
}
}  // extern "C++"
// the per-proof tail of both: kernel K9, then the host verifier for its verdict 2
static void per_proof_verdicts(const char *vk_path, BatchVerifier &v, const Proof *ps, const uint8_t *parsed, const Fe32 *in, size_t ni, size_t n, uint8_t *ok) {
  v.verify(ps, in, n, ok);
  for (size_t i = 0; i < n; i++) { if (!parsed[i]) ok[i] = 0; else if (ok[i] == 2) ok[i] = verify_proof(*vk_for_path(vk_path), in + i * ni, ni, ps[i]) ? 1 : 0; }
}
static void gt_bytes(const host::HFq12 &g, uint8_t out[384]) {
  host::HFq c[12]; static_assert(sizeof(c) == sizeof(g), "GT layout"); memcpy(c, &g, sizeof c);
  for (int k = 0; k < 12; k++) { const host::HFq v = c[k].from_mont(); memcpy(out + 32 * k, v.l, 32); }
}
// a call's records parsed as zkgpu_verify_batch parses them
static void parse_records(const char *proofs_hex, size_t n, std::vector<Proof> &ps, std::vector<uint8_t> &parsed) {
  ps.assign(n, Proof()); parsed.assign(n, 0);
  for (size_t i = 0; i < n; i++) {
    parsed[i] = strnlen(proofs_hex + 512 * i, 512) == 512 && proof_from_hex(proofs_hex + 512 * i, ps[i]);
    if (!parsed[i]) memset(&ps[i], 0, sizeof(Proof));
  }
}
static bool weights_from(const uint8_t *given, size_t n, std::vector<uint8_t> &w) {
  w.assign(16 * n, 0); if (!given) { fresh_weights(w.data(), n); return true; }
  memcpy(w.data(), given, 16 * n); for (size_t i = 0; i < n; i++) if (is_zero_weight(&w[16 * i])) return false;
  return true;
}
}  // namespace

int zkgpu_verify_batch_rlc(const char *vk_path, const char *proofs_hex, const uint8_t *inputs, size_t n_inputs, size_t n, const uint8_t *weights, uint8_t *ok,
    uint32_t *by_equation) { return guarded([&] {
  if (!vk_path || (!proofs_hex && n) || !ok) return ZKGPU_ERR_ARG;
  if (by_equation) *by_equation = 0;
  std::vector<uint8_t> w; if (!weights_from(weights, n, w)) { zkgpu_set_error("a weight is 0"); return ZKGPU_ERR_ARG; }
  std::shared_ptr<BatchVerifier> v = gpu_verifier_for_path(vk_path); const Fe32 *in = (const Fe32 *)inputs;
  if (v->num_inputs() != n_inputs) { for (size_t i = 0; i < n; i++) ok[i] = 0; g_rlc_per_proof.fetch_add(1); return ZKGPU_OK; }   // strong IC
  std::vector<Proof> ps; std::vector<uint8_t> parsed; parse_records(proofs_hex, n, ps, parsed);
  return rlc_engine_call(vk_path, parsed.data(), n_inputs, n, ok, by_equation, [&](RlcPart &p) { return rlc_part(vk_path, ps.data(), in, n_inputs, n, w.data(), false, p); },
      [&] { per_proof_verdicts(vk_path, *v, ps.data(), parsed.data(), in, n_inputs, n, ok); }); }); }
// test entries: the left-hand side's GT value FE(...) and whether it equals the right-hand side, for given weights, on the device (whatever the record count) or on
// the host.  Points at infinity contribute 1 (no fallback here).  Returns 1 / 0, or an error
int zkgpu_test_verify_rlc_device(const char *vk_path, const char *proofs_hex, const uint8_t *inputs, size_t n_inputs, size_t n, const uint8_t *weights, uint8_t *gt) {
  int res = 0; int rc = guarded([&] {
    if (!vk_path || !proofs_hex || !n) return ZKGPU_ERR_ARG;
    std::vector<uint8_t> w; if (!weights_from(weights, n, w)) return ZKGPU_ERR_ARG;
    std::vector<Proof> ps; std::vector<uint8_t> parsed; parse_records(proofs_hex, n, ps, parsed); RlcPart p;
    if (!rlc_part(vk_path, ps.data(), (const Fe32 *)inputs, n_inputs, n, w.data(), false, p)) { zkgpu_set_error("the key fails the subgroup checks of the block equation"); return ZKGPU_ERR_ARG; }
    const host::HFq12 g = host::final_exponentiation(rlc_lhs(*vk_for_path(vk_path), p.prod, p.s_acc, p.s_c)); if (gt) gt_bytes(g, gt);
    res = g == rlc_rhs(*vk_for_path(vk_path), p.s) ? 1 : 0; return ZKGPU_OK; });
  return rc == ZKGPU_OK ? res : rc; }
int zkgpu_test_verify_rlc_host(const char *vk_path, const char *proofs_hex, const uint8_t *inputs, size_t n_inputs, size_t n, const uint8_t *weights, uint8_t *gt) {
  int res = 0; int rc = guarded_host([&] {
    if (!vk_path || !proofs_hex || !n) return ZKGPU_ERR_ARG;
    std::vector<uint8_t> w; if (!weights_from(weights, n, w)) return ZKGPU_ERR_ARG;
    std::shared_ptr<PreparedVerifyingKey> vk = vk_for_path(vk_path); if (vk->vk.IC.size() != n_inputs + 1) return ZKGPU_ERR_ARG;
    std::vector<Proof> ps; std::vector<uint8_t> parsed; parse_records(proofs_hex, n, ps, parsed); host::HFq12 g;
    res = rlc_equation_host(*vk, ps.data(), parsed.data(), (const Fe32 *)inputs, n_inputs, n, w.data(), &g, nullptr) ? 1 : 0; if (gt) gt_bytes(g, gt); return ZKGPU_OK; });
  return rc == ZKGPU_OK ? res : rc; }
int zkgpu_verify_rlc_counters(uint64_t out[3]) {
  if (!out) return ZKGPU_ERR_ARG;
  out[0] = g_rlc_passed.load(); out[1] = g_rlc_failed.load(); out[2] = g_rlc_per_proof.load(); return ZKGPU_OK;
}

// ---- from records (include/zk_records.h; DESIGN.md "Block verification", "From records") ---------------------------------------------------------------------
// A block as the node holds it: 720-byte records, the proof as its 512 characters and the statement as the bytes of its hashes.  On the equation's path nothing
// derived from them is computed on the host: the records of a kind are gathered into pinned memory, uploaded once, and k_ingest_records makes the proof records, the
// packed inputs and a `parsed` byte where BlockVerifier::run_resident reads them; the integer sums of the right-hand scalars come back from the device too.
// records_to_host is the same conversion written from the functions verifyBatch uses — the road without a device, after a device failure, and the model the
// kernel is tested against.
namespace {
static RecordIngest &record_ingest() { static RecordIngest *g = new RecordIngest(); return *g; }   // one staging area a process; the caller holds the device mutex
static const zk_block_record &record_at(const zk_block_record *recs, const int *idx, size_t j) { return recs[idx ? (size_t)idx[j] : j]; }
// Below this many records of a kind the host converter is used even where a device is there: a conversion costs the host 3.7 us a record, the device about
// 0.4 ms a kind whatever the count (profiles/verify_records.txt): the device pays from about 100 records on.
static const size_t INGEST_DEVICE_MIN = 256;
static void records_to_host(const zk_block_record *recs, const int *idx, size_t m, CircuitKind kind, std::vector<Proof> &ps, std::vector<uint8_t> &parsed,
    std::vector<Fe32> &inputs) {
  const size_t ni = record_num_inputs((int)kind); ps.assign(m, Proof()); parsed.assign(m, 0); inputs.resize(m * ni);
  for (size_t j = 0; j < m; j++) {
    const zk_block_record &r = record_at(recs, idx, j); char hex[513]; memcpy(hex, r.proof, 512); hex[512] = 0;
    parsed[j] = strnlen(hex, 512) == 512 && proof_from_hex(hex, ps[j]);
    if (!parsed[j]) memset(&ps[j], 0, sizeof(Proof));
    // the statement of public_bits(): a blob is the hash's bytes reversed (what blob256_from_hex makes of common.ToHex's string)
    std::vector<bool> bits; auto blob = [&](int a, size_t nbytes) { uint8_t b[32]; for (size_t i = 0; i < nbytes; i++) b[i] = r.args[a][nbytes - 1 - i]; append(bits, blob_bits(b, nbytes)); };
    switch (kind) {
      case CircuitKind::Mint: case CircuitKind::Redeem: blob(0, 32); blob(1, 32); blob(2, 32); append(bits, u64_bits(r.value_s)); break;
      case CircuitKind::Send: blob(0, 32); blob(1, 32); blob(2, 32); blob(3, 32); break;
      default: blob(0, 32); blob(1, 20); blob(2, 32); blob(3, 32); blob(4, 32); blob(5, 32); break;
    }
    const std::vector<Fe32> in = pack_public_bits(bits); if (in.size() != ni) throw std::runtime_error("block records: input count");
    memcpy(&inputs[j * ni], in.data(), ni * sizeof(Fe32));
  }
}
static void stage_records(RecordIngest &ing, const zk_block_record *recs, const int *idx, size_t m) {
  HostSpan span("host.staging"); uint8_t *st = ing.stage(m);
  if (!idx) memcpy(st, recs, m * sizeof(zk_block_record));
  else for (size_t j = 0; j < m; j++) memcpy(st + j * sizeof(zk_block_record), &recs[idx[j]], sizeof(zk_block_record));
}
// the same three arrays made by the device and brought back (the per-proof path takes host arrays)
static void records_to_host_by_device(const zk_block_record *recs, const int *idx, size_t m, CircuitKind kind, std::vector<Proof> &ps, std::vector<uint8_t> &parsed,
    std::vector<Fe32> &inputs, bool lock) {
  const size_t ni = record_num_inputs((int)kind); ps.assign(m, Proof()); parsed.assign(m, 0); inputs.resize(m * ni);
  std::unique_lock<std::mutex> gl(g_gpu_mutex, std::defer_lock); if (lock) gl.lock();
  RecordIngest &ing = record_ingest(); stage_records(ing, recs, idx, m); ing.run(m, (int)kind, proof_encoding_strict()); ing.download(0, m, ps.data(), inputs.data(), parsed.data());
}
// rlc_part from records: ingest, the device half on the resident arrays, the integer sums from the device; the host keeps their reduction and the IC products
static bool rlc_part_records(const std::string &path, CircuitKind kind, const zk_block_record *recs, const int *idx, size_t m, const uint8_t *w, bool lock, RlcPart &out) {
  const size_t ni = record_num_inputs((int)kind);
  { std::unique_lock<std::mutex> gl(g_gpu_mutex, std::defer_lock); if (lock) gl.lock();
    std::shared_ptr<BlockVerifier> bv = block_verifier_for_path(path); if (!bv) return false;
    if (bv->num_inputs() != ni) throw std::runtime_error("block verify: input count");
    RecordIngest &ing = record_ingest(); stage_records(ing, recs, idx, m); ing.run(m, (int)kind, proof_encoding_strict());
    out.flags.assign(m, 0); out.sums.assign((ni + 1) * 7, 0); out.handed.clear();
    bv->run_resident(ing.items_dev(), ing.inputs_dev(), ing.parsed_dev(), w, m, out.flags.data(), out.prod, out.s_c, out.sums.data());
    for (size_t i = 0; i < m; i++) if (out.flags[i] == 2) { RlcHanded h; h.i = i; h.in.resize(ni); ing.download(i, 1, &h.p, h.in.data(), nullptr); out.handed.push_back(std::move(h)); } }
  { HostSpan span("host.s_acc"); out.s_acc = rlc_acc_from_sums(*vk_for_path(path), out.sums.data(), ni, out.s); }
  out.in_eq = 0; for (size_t i = 0; i < m; i++) out.in_eq += out.flags[i] == 1;
  return true;
}
// host arrays of a kind's records for the per-proof path: from the device where there is one and the kind is large enough to pay for the trip, else (or if that
// fails) from the host converter
static void records_for_per_proof(const zk_block_record *recs, const int *idx, size_t m, CircuitKind kind, std::vector<Proof> &ps, std::vector<uint8_t> &parsed,
    std::vector<Fe32> &inputs, bool lock) {
  if (m >= INGEST_DEVICE_MIN && gpu_available()) {
    try { records_to_host_by_device(recs, idx, m, kind, ps, parsed, inputs, lock); return; }
    catch (const std::exception &e) { fprintf(stderr, "libzkgpu: record ingest failed (%s); converting %zu record(s) on the host\n", e.what(), m); }
  }
  records_to_host(recs, idx, m, kind, ps, parsed, inputs);
}
// The decision of a block of records (verifyBlockRecords, and verifyBlock behind its conversion): the records grouped by kind as verifyBatch groups them.  A kind
// with at least RLC_MIN_RECORDS records (and the right input count) takes part in the block's equation: its left-hand factor goes into one Fq12 value, its
// alpha_beta^s into one right-hand side, and the block takes ONE final exponentiation.  Every other kind — a small one, one whose key fails rlc_key_ok, one with no
// record in the equation or a sum at infinity — goes through verify_group exactly as in verifyBatch, and so does every kind of the equation if the equation fails or
// a device step throws.
// (depth: the Merkle depth whose key the deposit records are verified with; 8 = depositvk.txt, every entry but verifyBlockTree)
static int verify_block_records(const zk_block_record *recs, int n, unsigned char *ok, const char *who, size_t depth = 8) {
  try {
    struct Group { CircuitKind kind; std::string path; std::vector<int> idx; std::vector<uint8_t> res; size_t ni = 0; RlcPart part; bool in_eq = false, decided = false; };
    std::vector<Group> groups; std::vector<int> idx[4];
    for (int i = 0; i < n; i++) { ok[i] = 0; if (recs[i].kind <= 3) idx[recs[i].kind].push_back(i); }
    for (int k = 0; k < 4; k++) { if (idx[k].empty()) continue; Group g; g.kind = (CircuitKind)k; g.path = key_path(g.kind, false, depth); g.idx = std::move(idx[k]);
      g.ni = record_num_inputs(k); g.res.assign(g.idx.size(), 0); groups.push_back(std::move(g)); }
    const bool one_kind = groups.size() == 1 && groups[0].idx.size() == (size_t)n;       // (a block of one kind is staged with one copy)
    bool any_eq = false;
    if (gpu_available()) {
      try {
        host::HFq12 lhs = host::HFq12::one(), rhs = host::HFq12::one();
        for (Group &g : groups) {
          const size_t m = g.idx.size(); if (m < RLC_MIN_RECORDS) continue;
          std::shared_ptr<PreparedVerifyingKey> vk = vk_for_path(g.path); if (vk->vk.IC.size() != g.ni + 1) continue;   // (strong IC: verify_group rejects the group)
          std::vector<uint8_t> w(16 * m); { HostSpan span("host.weights"); fresh_weights(w.data(), m); }
          if (!rlc_part_records(g.path, g.kind, recs, one_kind ? nullptr : g.idx.data(), m, w.data(), true, g.part) || !g.part.in_eq || g.part.s_acc.is_inf() ||
              g.part.s_c.is_inf()) continue;
          HostSpan span("host.closing"); lhs = lhs * rlc_lhs(*vk, g.part.prod, g.part.s_acc, g.part.s_c); rhs = rhs * rlc_rhs(*vk, g.part.s); g.in_eq = true; any_eq = true;
        }
        if (any_eq) {
          bool pass; { HostSpan span("host.closing"); pass = host::final_exponentiation(lhs) == rhs; } (pass ? g_rlc_passed : g_rlc_failed).fetch_add(1);
          if (pass) { for (Group &g : groups) if (g.in_eq) { decide_from_flags(g.path, g.part, nullptr, g.ni, g.idx.size(), g.res.data()); g.decided = true; } }
          else any_eq = false;
        }
      } catch (const std::exception &e) {
        fprintf(stderr, "libzkgpu: %s: block check failed (%s); deciding proof by proof\n", who, e.what());
        any_eq = false; for (Group &g : groups) g.decided = false;
      }
    }
    if (!any_eq) g_rlc_per_proof.fetch_add(1);
    for (Group &g : groups) if (!g.decided) {
      std::vector<Proof> ps; std::vector<uint8_t> parsed; std::vector<Fe32> inputs;
      records_for_per_proof(recs, one_kind ? nullptr : g.idx.data(), g.idx.size(), g.kind, ps, parsed, inputs, true);
      verify_group(g.kind, ps.data(), parsed.data(), inputs.data(), g.ni, g.idx.size(), g.res.data(), depth);
    }
    int accepted = 0;
    for (Group &g : groups) for (size_t j = 0; j < g.idx.size(); j++) { ok[g.idx[j]] = g.res[j]; accepted += g.res[j]; }
    return accepted;
  }
  catch (const std::exception &e) {
    zkgpu_set_error(e.what()); fprintf(stderr, "libzkgpu: %s: %s\n", who, e.what());
    for (int i = 0; i < n; i++) ok[i] = 0;
    return -1;
  }
  catch (...) { for (int i = 0; i < n; i++) ok[i] = 0; return -1; }
}

// ---- the proof cache in front of the proof step (DESIGN.md "Proof cache"; include/zk_proof_cache.h) ---------------------------------------------------------
// The key of a record: the first 20 bytes of SHA-256(salt || vktag || record).  record_digests makes the keys of a call, on the device (k_record_digest) or by the
// host model below, which is the same function on notes.cpp's SHA-256; a record whose kind has no bit in `kinds` gets 20 zero bytes.
// Below this many records the host model is used even where a device is there: it costs the host 2.1 us a record, the device road 0.07-0.10 ms for its upload,
// launch and download up to a few hundred records (profiles/proof_cache.txt): the two meet between 32 and 64 records.
static const size_t DIGEST_DEVICE_MIN = 48;
static void record_digests(const uint8_t salt[32], const uint8_t (*tags)[32], uint32_t kinds, const zk_block_record *recs, size_t n, bool device, uint8_t *out20) {
  if (device) {
    uint32_t mid[32]; memset(mid, 0, sizeof mid);                                        // the state after the block salt || vktag, once per kind and call
    for (int k = 0; k < 4; k++) if ((kinds >> k) & 1u) { uint8_t st[32]; sha256_compress_raw(salt, tags[k], st);
      for (int j = 0; j < 8; j++) mid[8 * k + j] = (uint32_t)st[4 * j] << 24 | (uint32_t)st[4 * j + 1] << 16 | (uint32_t)st[4 * j + 2] << 8 | st[4 * j + 3]; }
    std::lock_guard<std::mutex> gl(g_gpu_mutex); record_digests_dev((const uint8_t *)recs, n, mid, kinds, out20); return;
  }
  uint8_t m[64 + sizeof(zk_block_record)], d[32]; memcpy(m, salt, 32);
  for (size_t i = 0; i < n; i++) {
    const uint8_t kind = recs[i].kind; if (kind > 3 || !((kinds >> kind) & 1u)) { memset(out20 + 20 * i, 0, 20); continue; }
    memcpy(m + 32, tags[kind], 32); memcpy(m + 64, &recs[i], sizeof(zk_block_record)); sha256(m, sizeof m, d); memcpy(out20 + 20 * i, d, 20);
  }
}
// verify_block_records behind an optional cache: the keys, the lookup, the misses in one contiguous array through verify_block_records unchanged, the verdicts
// scattered back with ok = 1 for the hits, and the accepted misses stored.  Lookup and insert are two critical sections of the cache; verification between them runs
// without its mutex, so two threads may both verify a record — it is then stored once.  The cache never costs a decision: if a step of it throws, every record is
// treated as a miss and nothing is stored, which is the uncached entry.  A kind's tag is read before verification and again after it, and its records are stored only
// if the two are equal: a key file replaced during the call stores nothing under either name.
static int verify_block_records_cached(zkgpu_proof_cache *cache, const zk_block_record *recs, int n, unsigned char *ok, const char *who, size_t depth = 8) {
  if (!cache || n <= 0 || !gpu_available()) return verify_block_records(recs, n, ok, who, depth);
  const size_t N = (size_t)n; std::vector<uint8_t> keys, has_key, hit; uint8_t tags[4][32]; uint32_t kinds = 0; bool usable = false; size_t n_hit = 0;
  try {
    has_key.assign(N, 0); hit.assign(N, 0); bool present[4] = {false, false, false, false};
    for (size_t i = 0; i < N; i++) if (recs[i].kind <= 3) present[recs[i].kind] = true;
    for (int k = 0; k < 4; k++) if (present[k]) {                                         // (a kind whose key cannot be loaded has no key: its records go to verification as they are)
      try { vk_for_path(key_path((CircuitKind)k, false, depth), tags[k]); kinds |= 1u << k; } catch (const std::exception &) {} }
    if (kinds) {
      HostSpan span("host.cache_lookup");
      keys.resize(20 * N); record_digests(cache->c.salt(), tags, kinds, recs, N, N >= DIGEST_DEVICE_MIN, keys.data());
      std::vector<uint8_t> packed; std::vector<size_t> at; packed.reserve(20 * N); at.reserve(N);
      for (size_t i = 0; i < N; i++) if (recs[i].kind <= 3 && ((kinds >> recs[i].kind) & 1u)) { has_key[i] = 1; at.push_back(i); packed.insert(packed.end(), &keys[20 * i], &keys[20 * i] + 20); }
      std::vector<uint8_t> h(at.size(), 0); cache->c.lookup(packed.data(), at.size(), h.data());
      for (size_t j = 0; j < at.size(); j++) { hit[at[j]] = h[j]; n_hit += h[j] != 0; }
      usable = true;
    }
  }
  catch (const std::exception &e) { fprintf(stderr, "libzkgpu: %s: the proof cache failed (%s); verifying every record\n", who, e.what()); usable = false; n_hit = 0; }
  catch (...) { fprintf(stderr, "libzkgpu: %s: the proof cache failed; verifying every record\n", who); usable = false; n_hit = 0; }
  int rc;
  if (!n_hit) rc = verify_block_records(recs, n, ok, who, depth);
  else {
    try {
      std::vector<zk_block_record> miss; std::vector<size_t> idx; miss.reserve(N - n_hit); idx.reserve(N - n_hit);
      { HostSpan span("host.cache_gather"); for (size_t i = 0; i < N; i++) if (!hit[i]) { miss.push_back(recs[i]); idx.push_back(i); } }
      std::vector<unsigned char> mok(miss.size() + 1, 0);
      rc = miss.empty() ? 0 : verify_block_records(miss.data(), (int)miss.size(), mok.data(), who, depth);   // (a block of hits alone runs no verifier at all)
      if (rc < 0) { for (int i = 0; i < n; i++) ok[i] = 0; return -1; }
      for (size_t i = 0; i < N; i++) ok[i] = hit[i] ? 1 : 0;
      for (size_t j = 0; j < idx.size(); j++) ok[idx[j]] = mok[j];
      rc += (int)n_hit;
    }
    catch (const std::exception &e) { fprintf(stderr, "libzkgpu: %s: the proof cache failed (%s); verifying every record\n", who, e.what()); return verify_block_records(recs, n, ok, who, depth); }
  }
  if (rc < 0 || !usable) return rc;
  try {
    bool same[4] = {false, false, false, false};
    for (int k = 0; k < 4; k++) if ((kinds >> k) & 1u) { uint8_t t[32];
      try { vk_for_path(key_path((CircuitKind)k, false, depth), t); same[k] = !memcmp(t, tags[k], 32); } catch (const std::exception &) {} }
    std::vector<uint8_t> mask(N, 0); bool any = false;
    for (size_t i = 0; i < N; i++) { mask[i] = has_key[i] && !hit[i] && ok[i] && same[recs[i].kind]; any |= mask[i] != 0; }
    if (any) { HostSpan span("host.cache_insert"); cache->c.insert(keys.data(), mask.data(), N); }
  }
  catch (const std::exception &e) { fprintf(stderr, "libzkgpu: %s: the proof cache stored nothing (%s)\n", who, e.what()); }
  catch (...) { fprintf(stderr, "libzkgpu: %s: the proof cache stored nothing\n", who); }
  return rc;
}
}  // namespace

int verifyBlockRecords(const zk_block_record *recs, int n, unsigned char *ok) {
  if (n < 0 || (n && (!recs || !ok))) return -1;
  return verify_block_records(recs, n, ok, "verifyBlockRecords");
}
// verifyBlock (include/zk_block.h), the entry that takes strings: every item becomes a record — an argument through blob256_from_hex / blob160_from_hex, so every
// odd string keeps its meaning, the blob reversed into the hash's byte order; the proof's 512 characters copied, or left as NULs (no hex digits: the record does
// not parse) where the string is missing or shorter — and the block is decided as verifyBlockRecords decides it.
int verifyBlock(const zk_verify_item *items, int n, unsigned char *ok) {
  if (n < 0 || (n && (!items || !ok))) return -1;
  try {
    std::vector<zk_block_record> recs((size_t)n);                                         // (value-initialised: all zero)
    for (int i = 0; i < n; i++) {
      const zk_verify_item &it = items[i]; zk_block_record &r = recs[i]; r.kind = it.kind >= 0 && it.kind <= 3 ? (uint8_t)it.kind : 0xff; r.value_s = it.value_s;
      if (it.proof && strnlen(it.proof, 512) == 512) memcpy(r.proof, it.proof, 512);
      if (r.kind == 0xff) continue;
      const int n_args = r.kind == ZK_KIND_SEND ? 4 : r.kind == ZK_KIND_DEPOSIT ? 6 : 3;
      for (int a = 0; a < n_args; a++) {
        if (r.kind == ZK_KIND_DEPOSIT && a == 1) { const Blob160 b = blob160_from_hex(it.args[a] ? it.args[a] : ""); for (int k = 0; k < 20; k++) r.args[a][k] = b.b[19 - k]; }
        else { const Blob256 b = blob256_from_hex(it.args[a] ? it.args[a] : ""); for (int k = 0; k < 32; k++) r.args[a][k] = b.b[31 - k]; }
      }
    }
    return verify_block_records(recs.data(), n, ok, "verifyBlock");
  }
  catch (const std::exception &e) {
    zkgpu_set_error(e.what()); fprintf(stderr, "libzkgpu: verifyBlock: %s\n", e.what());
    for (int i = 0; i < n; i++) ok[i] = 0;
    return -1;
  }
  catch (...) { for (int i = 0; i < n; i++) ok[i] = 0; return -1; }
}

// zkgpu_verify_batch_rlc for records of ONE kind (include/zkgpu.h)
static int records_one_kind(const zk_block_record *recs, size_t n) {
  if (!recs || !n || recs[0].kind > 3) return -1;
  for (size_t i = 1; i < n; i++) if (recs[i].kind != recs[0].kind) return -1;
  return recs[0].kind;
}
int zkgpu_verify_records_rlc(const char *vk_path, const zk_block_record *recs, size_t n, const uint8_t *weights, uint8_t *ok, uint32_t *by_equation) { return guarded([&] {
  if (!vk_path || (!recs && n) || !ok) return ZKGPU_ERR_ARG;
  if (by_equation) *by_equation = 0;
  if (!n) return ZKGPU_OK;
  const int kind = records_one_kind(recs, n); if (kind < 0) { zkgpu_set_error("the records are not of one known kind"); return ZKGPU_ERR_ARG; }
  std::vector<uint8_t> w; if (!weights_from(weights, n, w)) { zkgpu_set_error("a weight is 0"); return ZKGPU_ERR_ARG; }
  std::shared_ptr<BatchVerifier> v = gpu_verifier_for_path(vk_path); const size_t ni = record_num_inputs(kind);
  if (v->num_inputs() != ni) { for (size_t i = 0; i < n; i++) ok[i] = 0; g_rlc_per_proof.fetch_add(1); return ZKGPU_OK; }   // strong IC
  return rlc_engine_call(vk_path, nullptr, ni, n, ok, by_equation, [&](RlcPart &p) { return rlc_part_records(vk_path, (CircuitKind)kind, recs, nullptr, n, w.data(), false, p); },
      [&] { std::vector<Proof> ps; std::vector<uint8_t> parsed; std::vector<Fe32> in; records_for_per_proof(recs, nullptr, n, (CircuitKind)kind, ps, parsed, in, false);
            per_proof_verdicts(vk_path, *v, ps.data(), parsed.data(), in.data(), ni, n, ok); }); }); }
// test entries.  zkgpu_test_ingest_records: the converter's three arrays for records of one kind, from k_ingest_records (device = 1) or from records_to_host
// (device = 0: no device needed).  zkgpu_test_records_rlc: the equation through the device path from records, whatever their count: 1 / 0 as
// zkgpu_test_verify_rlc_device, its GT value and the device's integer sums.  zkgpu_test_rlc_sums_host: the host loop's sums.
int zkgpu_test_ingest_records(const zk_block_record *recs, size_t n, int device, uint8_t *items_out, uint8_t *inputs_out, size_t *n_inputs_out, uint8_t *parsed_out) {
  auto body = [&] {
    if (!n_inputs_out) return ZKGPU_ERR_ARG; *n_inputs_out = 0;
    if (!n) return ZKGPU_OK;
    const int kind = records_one_kind(recs, n); if (kind < 0 || !items_out || !inputs_out || !parsed_out) { zkgpu_set_error("the records are not of one known kind"); return ZKGPU_ERR_ARG; }
    std::vector<Proof> ps; std::vector<uint8_t> parsed; std::vector<Fe32> in;
    if (device) records_to_host_by_device(recs, nullptr, n, (CircuitKind)kind, ps, parsed, in, false); else records_to_host(recs, nullptr, n, (CircuitKind)kind, ps, parsed, in);
    *n_inputs_out = record_num_inputs(kind); memcpy(items_out, ps.data(), n * sizeof(Proof)); memcpy(inputs_out, in.data(), in.size() * sizeof(Fe32)); memcpy(parsed_out, parsed.data(), n);
    return ZKGPU_OK; };
  return device ? guarded(body) : guarded_host(body); }
int zkgpu_test_records_rlc(const char *vk_path, const zk_block_record *recs, size_t n, const uint8_t *weights, uint8_t *gt, uint64_t *sums_out) {
  int res = 0; int rc = guarded([&] {
    if (!vk_path || !recs || !n) return ZKGPU_ERR_ARG;
    const int kind = records_one_kind(recs, n); if (kind < 0) { zkgpu_set_error("the records are not of one known kind"); return ZKGPU_ERR_ARG; }
    std::vector<uint8_t> w; if (!weights_from(weights, n, w)) return ZKGPU_ERR_ARG;
    if (vk_for_path(vk_path)->vk.IC.size() != record_num_inputs(kind) + 1) { zkgpu_set_error("the key's input count is not the kind's"); return ZKGPU_ERR_ARG; }
    RlcPart p;
    if (!rlc_part_records(vk_path, (CircuitKind)kind, recs, nullptr, n, w.data(), false, p)) { zkgpu_set_error("the key fails the subgroup checks of the block equation"); return ZKGPU_ERR_ARG; }
    const host::HFq12 g = host::final_exponentiation(rlc_lhs(*vk_for_path(vk_path), p.prod, p.s_acc, p.s_c)); if (gt) gt_bytes(g, gt);
    if (sums_out) memcpy(sums_out, p.sums.data(), p.sums.size() * sizeof(uint64_t));
    res = g == rlc_rhs(*vk_for_path(vk_path), p.s) ? 1 : 0; return ZKGPU_OK; });
  return rc == ZKGPU_OK ? res : rc; }
int zkgpu_test_rlc_sums_host(const uint8_t *inputs, size_t n_inputs, const uint8_t *weights, const uint8_t *flags, size_t n, uint64_t *sums_out) { return guarded_host([&] {
  if ((n && (!weights || !flags || (n_inputs && !inputs))) || !sums_out) return ZKGPU_ERR_ARG;
  rlc_int_sums((const Fe32 *)inputs, n_inputs, weights, flags, n, sums_out); return ZKGPU_OK; }); }

// ---- the resident commitment tree (DESIGN.md "Commitment tree"; include/zkgpu.h, include/zk_tree.h) ---------------------------------------------------------
zkgpu_tree *zkgpu_tree_create(int depth) {
  zkgpu_tree *t = nullptr;
  try {
    if (!gpu_available()) { zkgpu_set_error("no HIP device visible; libzkgpu has no CPU fallback"); return nullptr; }
    if (depth < 1 || depth > 32) { zkgpu_set_error("commitment tree: the depth must lie between 1 and 32"); return nullptr; }
    t = new zkgpu_tree(depth);
  }
  catch (const std::exception &e) { zkgpu_set_error(e.what()); } catch (...) { zkgpu_set_error("unknown error"); }
  return t;
}
void zkgpu_tree_destroy(zkgpu_tree *t) { try { delete t; } catch (...) {} }
int zkgpu_tree_append(zkgpu_tree *t, const uint8_t *leaves, size_t n) { return guarded_tree(t, [&] {
  if (n && !leaves) return ZKGPU_ERR_ARG;
  if (!t->t.append(leaves, n)) { zkgpu_set_error("commitment tree: more than 2^" + std::to_string(t->t.depth()) + " leaves"); return ZKGPU_ERR_ARG; }
  return ZKGPU_OK; }); }
int zkgpu_tree_size(zkgpu_tree *t, uint64_t *n) { return guarded_tree(t, [&] { if (!n) return ZKGPU_ERR_ARG; *n = t->t.size(); return ZKGPU_OK; }); }
int zkgpu_tree_root(zkgpu_tree *t, uint8_t root[32]) { return guarded_tree(t, [&] { if (!root) return ZKGPU_ERR_ARG; t->t.root(root); return ZKGPU_OK; }); }
int zkgpu_tree_path(zkgpu_tree *t, uint64_t index, uint8_t *siblings) { return guarded_tree(t, [&] {
  if (!siblings) return ZKGPU_ERR_ARG;
  if (!t->t.path(index, siblings)) { zkgpu_set_error("commitment tree: no leaf " + std::to_string(index)); return ZKGPU_ERR_ARG; }
  return ZKGPU_OK; }); }
int zkgpu_tree_find(zkgpu_tree *t, const uint8_t leaf[32], uint64_t *index) { return guarded_tree(t, [&] {
  if (!leaf || !index) return ZKGPU_ERR_ARG;
  if (!t->t.find(leaf, *index)) { zkgpu_set_error("commitment tree: the leaf is not in the tree"); return ZKGPU_ERR_ARG; }
  return ZKGPU_OK; }); }
int zkgpu_test_tree_launches(zkgpu_tree *t, uint64_t *launches) { return guarded_tree(t, [&] { if (!launches) return ZKGPU_ERR_ARG; *launches = t->t.launches(); return ZKGPU_OK; }); }
// past states (DESIGN.md "Past states of the commitment tree"): the tree checks sizes and indices under its own lock, before anything is queued
int zkgpu_tree_roots_at(zkgpu_tree *t, const uint64_t *sizes, size_t q, uint8_t *roots) { return guarded_tree(t, [&] {
  if (q && (!sizes || !roots)) { zkgpu_set_error("commitment tree: a null pointer"); return ZKGPU_ERR_ARG; }
  if (!t->t.roots_at(sizes, q, roots)) { zkgpu_set_error("commitment tree: a size above the tree's size"); return ZKGPU_ERR_ARG; }
  return ZKGPU_OK; }); }
int zkgpu_tree_paths_at(zkgpu_tree *t, uint64_t size, const uint64_t *indices, size_t q, uint8_t *siblings, uint8_t root[32]) { return guarded_tree(t, [&] {
  if (q && (!indices || !siblings)) { zkgpu_set_error("commitment tree: a null pointer"); return ZKGPU_ERR_ARG; }
  if (!t->t.paths_at(size, indices, q, siblings, root)) { zkgpu_set_error("commitment tree: size " + std::to_string(size) + " is above the tree's size, or an index is not below it"); return ZKGPU_ERR_ARG; }
  return ZKGPU_OK; }); }
int zkgpu_tree_find_at(zkgpu_tree *t, uint64_t size, const uint8_t leaf[32], uint64_t *index) { return guarded_tree(t, [&] {
  if (!leaf || !index) return ZKGPU_ERR_ARG;
  uint64_t got = 0;
  if (!t->t.find_at(size, leaf, got)) { zkgpu_set_error("commitment tree: the leaf is not among the first " + std::to_string(size) + " leaves, or the tree is smaller"); return ZKGPU_ERR_ARG; }
  *index = got; return ZKGPU_OK; }); }
int zkgpu_tree_rewind(zkgpu_tree *t, uint64_t size) { return guarded_tree(t, [&] {
  if (!t->t.rewind(size)) { zkgpu_set_error("commitment tree: cannot rewind to " + std::to_string(size) + " leaves, the tree holds fewer"); return ZKGPU_ERR_ARG; }
  return ZKGPU_OK; }); }
// anchors (DESIGN.md "A block against the resident tree"): sizes are checked under the tree's lock, before anything is queued
int zkgpu_tree_match_roots(zkgpu_tree *t, const uint64_t *sizes, size_t n_sizes, const uint8_t *rts, size_t n, int hash_order, int32_t *match_out) { return guarded_tree(t, [&] {
  if ((n_sizes && !sizes) || (n && (!rts || !match_out))) { zkgpu_set_error("commitment tree: a null pointer"); return ZKGPU_ERR_ARG; }
  if (n_sizes >= (1ull << 31)) { zkgpu_set_error("commitment tree: 2^31 anchors or more"); return ZKGPU_ERR_ARG; }
  if (!t->t.match_roots(sizes, n_sizes, rts, n, hash_order != 0, match_out)) { zkgpu_set_error("commitment tree: a size above the tree's size"); return ZKGPU_ERR_ARG; }
  return ZKGPU_OK; }); }
int zkgpu_tree_match_roots_window(zkgpu_tree *t, const uint64_t *sizes, size_t n_sizes, const uint8_t *rts, size_t n, const uint32_t *lo, const uint32_t *hi, int hash_order,
                                  int32_t *match_out) { return guarded_tree(t, [&] {
  if ((n_sizes && !sizes) || (n && (!rts || !lo || !hi || !match_out))) { zkgpu_set_error("commitment tree: a null pointer"); return ZKGPU_ERR_ARG; }
  if (n_sizes >= (1ull << 31)) { zkgpu_set_error("commitment tree: 2^31 anchors or more"); return ZKGPU_ERR_ARG; }
  if (!t->t.match_roots_window(sizes, n_sizes, rts, n, lo, hi, hash_order != 0, match_out)) {
    zkgpu_set_error("commitment tree: a size above the tree's size, or a window with lo > hi or hi above the number of anchors"); return ZKGPU_ERR_ARG; }
  return ZKGPU_OK; }); }
int zkgpu_test_tree_state_launches(zkgpu_tree *t, uint64_t *launches) { return guarded_tree(t, [&] { if (!launches) return ZKGPU_ERR_ARG; *launches = t->t.state_launches(); return ZKGPU_OK; }); }
int zkgpu_test_tree_host(int depth, const uint8_t *leaves, size_t n, uint64_t index, uint8_t root[32], uint8_t *path) { return guarded_host([&] {
  if (depth < 1 || depth > 32 || (n && !leaves) || n > (1ull << depth) || (path && index >= n)) return ZKGPU_ERR_ARG;
  std::vector<Blob256> lv(n); if (n) memcpy(lv.data(), leaves, 32 * n);
  if (root) { const Blob256 r = merkle_root(lv, (size_t)depth); memcpy(root, r.b, 32); }
  if (path) { std::vector<bool> bits; const std::vector<Blob256> p = merkle_path(lv, (size_t)depth, (size_t)index, bits); memcpy(path, p.data(), 32 * (size_t)depth); }
  return ZKGPU_OK; }); }

zk_tree *zkTreeNew(int depth) { return zkgpu_tree_create(depth); }
void zkTreeFree(zk_tree *t) { zkgpu_tree_destroy(t); }
long long zkTreeAppend(zk_tree *t, char *cmtarray, int n) {
  uint64_t size = 0;
  const int rc = guarded_tree(t, [&] {
    if (n < 0) return ZKGPU_ERR_ARG;
    const size_t len = cmtarray ? strlen(cmtarray) : 0; std::vector<Blob256> leaves((size_t)n); char item[67];
    for (size_t i = 0; i < (size_t)n; i++) {                                                     // genRoot's format (parse_cmtarray), without its limit of 256 items
      const size_t at = i * 66, k = at < len ? std::min<size_t>(66, len - at) : 0; if (k) memcpy(item, cmtarray + at, k); item[k] = 0; leaves[i] = blob256_from_hex(item); }
    if (!t->t.append(n ? leaves[0].b : nullptr, (size_t)n)) { zkgpu_set_error("commitment tree: more than 2^" + std::to_string(t->t.depth()) + " leaves"); return ZKGPU_ERR_ARG; }
    size = t->t.size(); return ZKGPU_OK; });
  if (rc != ZKGPU_OK) { fprintf(stderr, "libzkgpu: zkTreeAppend: %s\n", zkgpu_last_error()); return -1; }
  return (long long)size;
}
char *zkTreeRoot(zk_tree *t) {
  Blob256 r; if (guarded_tree(t, [&] { t->t.root(r.b); return ZKGPU_OK; }) != ZKGPU_OK) { fprintf(stderr, "libzkgpu: zkTreeRoot: %s\n", zkgpu_last_error()); return nullptr; }
  return hash_out(r);
}
// genDepositproof against the resident tree: ONE snapshot gives the leaf's index, its path and the root they belong to; the proof's statement is that root.
// size < 0: the tree's newest state (genDepositproofTree); otherwise the state of the first `size` leaves (genDepositproofTreeAt)
static char *deposit_proof_tree(uint64_t value, uint64_t value_old, char *sn_old, char *r_old, char *sn, char *r, char *sns, char *rs, char *cmtB_old, char *cmtB,
    uint64_t value_s, char *pk, char *sn_A_old, char *cmtS, char *sk, zk_tree *t, bool at, long long size, char rt_out[65]) {
  if (rt_out) rt_out[0] = 0;
  try {
    const std::string sentinel = proof_to_hex(default_proof());
    if (!gpu_available()) {
      zkgpu_set_error("no HIP device visible; libzkgpu has no CPU fallback"); fprintf(stderr, "libzkgpu: no HIP device visible, cannot generate deposit proof\n");
      return dup_string(sentinel);
    }
    if (!t || !rt_out) throw std::runtime_error("genDepositproofTree: no tree or no rt_out");
    DepositInputs in = deposit_fields(value, value_old, sn_old, r_old, sn, r, sns, rs, cmtB_old, cmtB, value_s, pk, sn_A_old, cmtS, sk);
    CommitmentTree::Snapshot snap;
    // the reference throws out of IncrementalMerkleTree::path() here (IncrementalMerkleTree.tcc:214-216)
    if (at && size < 0) throw std::runtime_error("genDepositproofTreeAt: a negative size");
    if (at ? !t->t.snapshot_at((uint64_t)size, in.cmtS.b, snap) : !t->t.snapshot(in.cmtS.b, snap))
      throw std::runtime_error(at ? "cmtS is not among the first " + std::to_string(size) + " commitments of the tree, or the tree holds fewer" : std::string("cmtS is not among the commitments of the tree"));
    const size_t depth = (size_t)t->t.depth(); in.path.resize(depth); memcpy(in.path.data(), snap.path.data(), 32 * depth); in.index_bits = snap.index_bits; memcpy(in.rt.b, snap.root, 32);
    char *proof = generate(CircuitKind::Deposit, [&](Circuit &c) { assign_deposit(c, in); }, depth);
    if (proof && sentinel != proof) { const std::string rt = blob_to_hex(in.rt.b, 32); memcpy(rt_out, rt.c_str(), 65); }
    return proof;
  }
  catch (const std::exception &e) { zkgpu_set_error(e.what()); fprintf(stderr, "libzkgpu: %s\n", e.what()); }
  catch (...) { zkgpu_set_error("unknown error"); }
  try { return dup_string(proof_to_hex(default_proof())); } catch (...) { return nullptr; }
}
char *genDepositproofTree(uint64_t value, uint64_t value_old, char *sn_old, char *r_old, char *sn, char *r, char *sns, char *rs, char *cmtB_old, char *cmtB,
    uint64_t value_s, char *pk, char *sn_A_old, char *cmtS, char *sk, zk_tree *t, char rt_out[65]) {
  return deposit_proof_tree(value, value_old, sn_old, r_old, sn, r, sns, rs, cmtB_old, cmtB, value_s, pk, sn_A_old, cmtS, sk, t, false, 0, rt_out); }
// ---- include/zk_tree_states.h: roots and proofs at past sizes, rewind ----
char *genDepositproofTreeAt(uint64_t value, uint64_t value_old, char *sn_old, char *r_old, char *sn, char *r, char *sns, char *rs, char *cmtB_old, char *cmtB,
    uint64_t value_s, char *pk, char *sn_A_old, char *cmtS, char *sk, zk_tree *t, long long size, char rt_out[65]) {
  return deposit_proof_tree(value, value_old, sn_old, r_old, sn, r, sns, rs, cmtB_old, cmtB, value_s, pk, sn_A_old, cmtS, sk, t, true, size, rt_out); }
int zkTreeRootsAt(zk_tree *t, const long long *sizes, int q, uint8_t *roots) {
  const int rc = guarded_tree(t, [&] {
    if (q < 0 || (q && (!sizes || !roots))) { zkgpu_set_error("zkTreeRootsAt: a negative count or a null pointer"); return ZKGPU_ERR_ARG; }
    std::vector<uint64_t> m((size_t)q); std::vector<uint8_t> out(32 * (size_t)q);
    for (int i = 0; i < q; i++) { if (sizes[i] < 0) { zkgpu_set_error("zkTreeRootsAt: a negative size"); return ZKGPU_ERR_ARG; } m[i] = (uint64_t)sizes[i]; }
    if (!t->t.roots_at(m.data(), (size_t)q, out.data())) { zkgpu_set_error("zkTreeRootsAt: a size above the tree's size"); return ZKGPU_ERR_ARG; }
    for (size_t i = 0; i < (size_t)q; i++) for (int b = 0; b < 32; b++) roots[32 * i + b] = out[32 * i + 31 - b];   // blob order -> the bytes of the common.Hash
    return ZKGPU_OK; });
  if (rc != ZKGPU_OK) { fprintf(stderr, "libzkgpu: zkTreeRootsAt: %s\n", zkgpu_last_error()); return -1; }
  return 0;
}
char *zkTreeRootAt(zk_tree *t, long long size) {
  Blob256 r;
  const int rc = guarded_tree(t, [&] {
    const uint64_t m = (uint64_t)size;
    if (size < 0 || !t->t.roots_at(&m, 1, r.b)) { zkgpu_set_error("zkTreeRootAt: the tree does not hold " + std::to_string(size) + " leaves"); return ZKGPU_ERR_ARG; }
    return ZKGPU_OK; });
  if (rc != ZKGPU_OK) { fprintf(stderr, "libzkgpu: zkTreeRootAt: %s\n", zkgpu_last_error()); return nullptr; }
  return hash_out(r);
}
long long zkTreeRewind(zk_tree *t, long long size) {
  const int rc = guarded_tree(t, [&] {
    if (size < 0 || !t->t.rewind((uint64_t)size)) { zkgpu_set_error("zkTreeRewind: the tree does not hold " + std::to_string(size) + " leaves"); return ZKGPU_ERR_ARG; }
    return ZKGPU_OK; });
  if (rc != ZKGPU_OK) { fprintf(stderr, "libzkgpu: zkTreeRewind: %s\n", zkgpu_last_error()); return -1; }
  return size;
}
bool verifyDepositproofDepth(int depth, char *data, char *RT, char *pk, char *cmtb_old, char *snold, char *cmtb, char *sns) {
  if (depth < 1 || depth > 32) return false;
  const char *a[6] = {RT, pk, cmtb_old, snold, cmtb, sns}; return verify(CircuitKind::Deposit, data, public_bits(CircuitKind::Deposit, a, 0), (size_t)depth); }

// ---- the roots of many commitment lists (DESIGN.md "Roots of many lists"; include/zkgpu.h, include/zk_roots.h) --------------------------------------------------
// The device road is gpu_list_roots.hip; list_roots_host is the same roots from merkle_root, list by list — the model the kernel is tested against and the road of
// verifyBlockRecordsRoots without a device or after a device failure, as records_to_host is for the records.
static_assert(sizeof(zkgpu_leaf_range) == sizeof(LeafRange) && sizeof(zk_cmt_range) == sizeof(LeafRange), "a leaf range is two 64-bit words at every level");
static int list_roots_args(int depth, const uint8_t *leaves, size_t n_leaves, const zkgpu_leaf_range *lists, size_t n_lists, const uint8_t *roots) {
  if (depth < 1 || depth > 32) { zkgpu_set_error("list roots: the depth must lie between 1 and 32"); return ZKGPU_ERR_ARG; }
  if ((n_leaves && !leaves) || (n_lists && (!lists || !roots))) { zkgpu_set_error("list roots: a null pointer"); return ZKGPU_ERR_ARG; }
  for (size_t i = 0; i < n_lists; i++) {
    if (lists[i].first > n_leaves || lists[i].count > n_leaves - lists[i].first) { zkgpu_set_error("list roots: list " + std::to_string(i) + " leaves the array"); return ZKGPU_ERR_ARG; }
    if (lists[i].count > (1ull << depth)) { zkgpu_set_error("list roots: list " + std::to_string(i) + " holds more than 2^" + std::to_string(depth) + " leaves"); return ZKGPU_ERR_ARG; }
  }
  return ZKGPU_OK;
}
static void list_roots_host(int depth, const uint8_t *leaves, const zkgpu_leaf_range *lists, size_t n_lists, bool hash_order, uint8_t *roots) {
  std::vector<Blob256> lv;
  for (size_t i = 0; i < n_lists; i++) {
    lv.resize((size_t)lists[i].count);
    for (size_t k = 0; k < lv.size(); k++) { const uint8_t *src = leaves + 32 * ((size_t)lists[i].first + k);
      if (hash_order) for (int b = 0; b < 32; b++) lv[k].b[b] = src[31 - b]; else memcpy(lv[k].b, src, 32); }
    const Blob256 r = merkle_root(lv, (size_t)depth);
    if (hash_order) for (int b = 0; b < 32; b++) roots[32 * i + b] = r.b[31 - b]; else memcpy(roots + 32 * i, r.b, 32);
  }
}
int zkgpu_list_roots(int depth, const uint8_t *leaves, size_t n_leaves, const zkgpu_leaf_range *lists, size_t n_lists, int hash_order, uint8_t *roots) {
  const int rc = guarded_host([&] { return list_roots_args(depth, leaves, n_leaves, lists, n_lists, roots); }); if (rc != ZKGPU_OK) return rc;
  return guarded([&] { list_roots_dev(depth, leaves, n_leaves, (const LeafRange *)lists, n_lists, hash_order != 0, roots); return ZKGPU_OK; }); }
int zkgpu_test_list_roots_host(int depth, const uint8_t *leaves, size_t n_leaves, const zkgpu_leaf_range *lists, size_t n_lists, int hash_order, uint8_t *roots) { return guarded_host([&] {
  const int rc = list_roots_args(depth, leaves, n_leaves, lists, n_lists, roots); if (rc != ZKGPU_OK) return rc;
  list_roots_host(depth, leaves, lists, n_lists, hash_order != 0, roots); return ZKGPU_OK; }); }
int zkgpu_test_list_roots_launches(uint64_t *launches) { if (!launches) return ZKGPU_ERR_ARG; *launches = list_roots_launches(); return ZKGPU_OK; }

int genRoots(const zk_cmt_lists *l, int depth, uint8_t *roots) {
  if (!l || l->n_lists < 0) { zkgpu_set_error("genRoots: no lists"); return -1; }
  const int rc = zkgpu_list_roots(depth, l->cmts, (size_t)l->n_cmts, (const zkgpu_leaf_range *)l->lists, (size_t)l->n_lists, 1, roots);
  if (rc != ZKGPU_OK) { fprintf(stderr, "libzkgpu: genRoots: %s\n", zkgpu_last_error()); return -1; }
  return 0;
}
// verifyBlockRecords, then RT of every record that names a list against that list's depth-8 root.  The roots of all lists are made once, on the device; a list of
// more than 256 commitments has no depth-8 root: it is computed as an empty one and rejects whoever names it.
// (cache: the proof step goes through verify_block_records_cached; null = no cache, the entry as it always was)
static int block_records_roots(const zk_block_record *recs, int n, const zk_cmt_lists *l, const int32_t *list_of, unsigned char *ok, zkgpu_proof_cache *cache = nullptr) {
  if (n < 0 || (n && (!recs || !ok))) return -1;
  auto fail = [&](const std::string &why) { zkgpu_set_error(why); fprintf(stderr, "libzkgpu: verifyBlockRecordsRoots: %s\n", why.c_str()); for (int i = 0; i < n; i++) ok[i] = 0; return -1; };
  try {
    bool any = false; if (list_of) for (int i = 0; i < n; i++) any |= list_of[i] >= 0;
    if (any && !l) return fail("records name lists and there are none");
    size_t n_lists = 0; std::vector<uint8_t> roots, usable; std::vector<zkgpu_leaf_range> ranges;
    if (l) {
      if (l->n_lists < 0 || (l->n_lists && !l->lists) || (l->n_cmts && !l->cmts)) return fail("a null pointer in the lists");
      n_lists = (size_t)l->n_lists; usable.assign(n_lists, 0); ranges.assign(n_lists, zkgpu_leaf_range{0, 0});
      { HostSpan span("host.roots_ranges");
        for (size_t j = 0; j < n_lists; j++) {
          const zk_cmt_range &r = l->lists[j]; if (r.first > l->n_cmts || r.count > l->n_cmts - r.first) return fail("list " + std::to_string(j) + " leaves the array of commitments");
          if (r.count <= 256) { usable[j] = 1; ranges[j] = zkgpu_leaf_range{r.first, r.count}; }
        } }
      if (any) {
        roots.resize(32 * n_lists); bool done = false;
        if (gpu_available()) {
          try { std::lock_guard<std::mutex> gl(g_gpu_mutex); list_roots_dev(8, l->cmts, (size_t)l->n_cmts, (const LeafRange *)ranges.data(), n_lists, true, roots.data()); done = true; }
          catch (const std::exception &e) { fprintf(stderr, "libzkgpu: verifyBlockRecordsRoots: the roots failed on the device (%s); computing %zu root(s) on the host\n", e.what(), n_lists); }
        }
        if (!done) list_roots_host(8, l->cmts, ranges.data(), n_lists, true, roots.data());
      }
    }
    const int rc = verify_block_records_cached(cache, recs, n, ok, "verifyBlockRecordsRoots"); if (rc < 0 || !list_of) return rc;
    HostSpan span("host.roots_compare"); int accepted = 0;
    for (int i = 0; i < n; i++) {
      const int32_t j = list_of[i];
      if (ok[i] && j != -1 && (j < 0 || (size_t)j >= n_lists || !usable[j] || recs[i].kind != ZK_KIND_DEPOSIT || memcmp(recs[i].args[0], &roots[32 * (size_t)j], 32))) ok[i] = 0;
      accepted += ok[i];
    }
    return accepted;
  }
  catch (const std::exception &e) { return fail(e.what()); }
  catch (...) { return fail("unknown error"); }
}
int verifyBlockRecordsRoots(const zk_block_record *recs, int n, const zk_cmt_lists *l, const int32_t *list_of, unsigned char *ok) { return block_records_roots(recs, n, l, list_of, ok); }

// ---- the resident set of spent serial numbers (DESIGN.md "Spent serial numbers"; include/zkgpu.h, include/zk_spent.h) ----------------------------------------
static zkgpu_snset *snset_create(const uint8_t *exempt, int log2_slots, const uint64_t *seed) {
  zkgpu_snset *s = nullptr;
  try {
    if (!gpu_available()) { zkgpu_set_error("no HIP device visible; libzkgpu has no CPU fallback"); return nullptr; }
    s = new zkgpu_snset(exempt, log2_slots, seed);
  }
  catch (const std::exception &e) { zkgpu_set_error(e.what()); } catch (...) { zkgpu_set_error("unknown error"); }
  return s;
}
zkgpu_snset *zkgpu_snset_create(const uint8_t exempt[20]) { return snset_create(exempt, 0, nullptr); }
zkgpu_snset *zkgpu_test_snset_create(int log2_slots, uint64_t seed, const uint8_t exempt[20]) {
  if (log2_slots < 4 || log2_slots > 31) { zkgpu_set_error("spent set: a table has 2^4 to 2^31 slots"); return nullptr; }
  return snset_create(exempt, log2_slots, &seed); }
void zkgpu_snset_destroy(zkgpu_snset *s) { try { delete s; } catch (...) {} }
int zkgpu_snset_size(zkgpu_snset *s, uint64_t *n) { return guarded_snset(s, [&] { if (!n) return ZKGPU_ERR_ARG; *n = s->s.size(); return ZKGPU_OK; }); }
int zkgpu_snset_spend(zkgpu_snset *s, const uint8_t *keys, const uint8_t *mask, size_t n, int commit, uint8_t *conflict, uint64_t *size_out) { return guarded_snset(s, [&] {
  if (!s->s.spend(keys, mask, n, commit != 0, conflict, size_out)) { zkgpu_set_error("spent set: a null pointer, or the log would reach 2^32 - 2 entries"); return ZKGPU_ERR_ARG; }
  return ZKGPU_OK; }); }
int zkgpu_snset_query(zkgpu_snset *s, uint64_t size, const uint8_t *keys, size_t q, uint64_t *index) { return guarded_snset(s, [&] {
  if (!s->s.query(size, keys, q, index)) { zkgpu_set_error("spent set: size " + std::to_string(size) + " is above the set's size, or a null pointer"); return ZKGPU_ERR_ARG; }
  return ZKGPU_OK; }); }
int zkgpu_snset_rewind(zkgpu_snset *s, uint64_t size) { return guarded_snset(s, [&] {
  if (!s->s.rewind(size)) { zkgpu_set_error("spent set: cannot rewind to " + std::to_string(size) + " keys, the set holds fewer"); return ZKGPU_ERR_ARG; }
  return ZKGPU_OK; }); }
int zkgpu_snset_read_log(zkgpu_snset *s, uint64_t first, uint64_t count, uint8_t *keys) { return guarded_snset(s, [&] {
  if (!s->s.read_log(first, count, keys)) { zkgpu_set_error("spent set: the range leaves the log, or a null pointer"); return ZKGPU_ERR_ARG; }
  return ZKGPU_OK; }); }
int zkgpu_test_snset_slots(zkgpu_snset *s, uint32_t *slots, uint64_t *n_slots, uint64_t *seed, uint64_t *tombstones) { return guarded_snset(s, [&] {
  if (!n_slots || !seed || !tombstones) return ZKGPU_ERR_ARG;
  std::vector<uint32_t> t; uint64_t sd = 0, tb = 0; s->s.table(t, sd, tb);
  if (slots) { if (*n_slots != t.size()) { zkgpu_set_error("spent set: the table has " + std::to_string(t.size()) + " slots"); return ZKGPU_ERR_ARG; } memcpy(slots, t.data(), 4 * t.size()); }
  *n_slots = t.size(); *seed = sd; *tombstones = tb; return ZKGPU_OK; }); }
int zkgpu_test_snset_launches(uint64_t *launches) { if (!launches) return ZKGPU_ERR_ARG; *launches = SpentSet::launches(); return ZKGPU_OK; }
// the model: for each record in turn, Exist -> conflict, otherwise (commit) CreateAccount.  A check-only call inserts nothing, so what it remembers of the call itself
// is kept apart from the set.
int zkgpu_test_snset_host(const uint8_t *resident, size_t n_resident, const uint8_t exempt[20], const uint8_t *keys, const uint8_t *mask, size_t n, int commit,
                          uint8_t *conflict, uint8_t *appended, size_t *n_appended) { return guarded_host([&] {
  if ((n_resident && !resident) || (n && (!keys || !conflict || (commit && !appended))) || !n_appended) return ZKGPU_ERR_ARG;
  typedef std::array<uint8_t, 20> Key; auto key = [](const uint8_t *p) { Key k; memcpy(k.data(), p, 20); return k; };
  std::set<Key> state, seen; for (size_t i = 0; i < n_resident; i++) state.insert(key(resident + 20 * i));
  size_t added = 0;
  for (size_t i = 0; i < n; i++) {
    const Key k = key(keys + 20 * i); conflict[i] = 0;
    if ((mask && !mask[i]) || (exempt && !memcmp(k.data(), exempt, 20))) continue;
    if (state.count(k)) { conflict[i] = 1; continue; }                                            // statedb.Exist: "sn is already used"
    if (seen.count(k)) { conflict[i] = 2; continue; }                                             // ... by an earlier transaction of this block
    seen.insert(k); if (commit) memcpy(appended + 20 * added++, k.data(), 20);                    // CreateAccount
  }
  *n_appended = added; return ZKGPU_OK; }); }
// ---- two keys a record (DESIGN.md "Two keys a record"; include/zk_spent_pk.h) -----------------------------------------------------------------------------------
int zkgpu_snset_spend_pairs(zkgpu_snset *s, const uint8_t *keys, const uint8_t *nkeys, size_t n, int commit, uint8_t *conflict, uint64_t *size_out) { return guarded_snset(s, [&] {
  if (!s->s.spend_pairs(keys, nkeys, n, commit != 0, conflict, size_out)) { zkgpu_set_error("spent set: a null pointer, more than two keys a record, or the log could reach 2^32 - 2 entries"); return ZKGPU_ERR_ARG; }
  return ZKGPU_OK; }); }
int zkgpu_test_snset_round_cap(zkgpu_snset *s, uint32_t rounds) { return guarded_snset(s, [&] { s->s.set_round_cap(rounds); return ZKGPU_OK; }); }
int zkgpu_test_snset_rounds(uint64_t *rounds, uint64_t *host_finishes) { if (!rounds || !host_finishes) return ZKGPU_ERR_ARG; SpentSet::rounds(*rounds, *host_finishes); return ZKGPU_OK; }
// the model: the loop above with up to two keys a record.  Exist on each key -> 1; a key that an earlier accepted record of the call created, or k1 == k2 -> 2;
// otherwise CreateAccount on each, k1 first.  The exempt key is skipped as k1 and rejects as k2.
int zkgpu_test_snset_host_pairs(const uint8_t *resident, size_t n_resident, const uint8_t exempt[20], const uint8_t *keys, const uint8_t *nkeys, size_t n, int commit,
                                uint8_t *conflict, uint8_t *appended, size_t *n_appended) { return guarded_host([&] {
  if ((n_resident && !resident) || (n && (!keys || !nkeys || !conflict || (commit && !appended))) || !n_appended) return ZKGPU_ERR_ARG;
  for (size_t i = 0; i < n; i++) if (nkeys[i] > 2) return ZKGPU_ERR_ARG;
  std::set<SnKey20> state, seen; for (size_t i = 0; i < n_resident; i++) state.insert(sn_key20(resident + 20 * i));
  size_t added = 0;
  for (size_t i = 0; i < n; i++) {
    const uint8_t *k = keys + 40 * i; conflict[i] = 0; if (!nkeys[i]) continue;
    SnKey20 ks[2]; size_t m = 0;
    if (!(exempt && !memcmp(k, exempt, 20))) ks[m++] = sn_key20(k);
    if (nkeys[i] == 2) { if (exempt && !memcmp(k + 20, exempt, 20)) { conflict[i] = 1; continue; } ks[m++] = sn_key20(k + 20); }
    bool in_state = false, in_call = m == 2 && ks[0] == ks[1];
    for (size_t j = 0; j < m; j++) { in_state |= state.count(ks[j]) != 0; in_call |= seen.count(ks[j]) != 0; }
    if (in_state) { conflict[i] = 1; continue; }
    if (in_call) { conflict[i] = 2; continue; }
    for (size_t j = 0; j < m; j++) { seen.insert(ks[j]); if (commit) memcpy(appended + 20 * added++, ks[j].data(), 20); }
  }
  *n_appended = added; return ZKGPU_OK; }); }

zk_snset *zkSnSetNew(const uint8_t *exempt_sn) { return zkgpu_snset_create(exempt_sn ? exempt_sn + 12 : nullptr); }
void zkSnSetFree(zk_snset *set) { zkgpu_snset_destroy(set); }
long long zkSnSetSize(zk_snset *set) { uint64_t n = 0; return zkgpu_snset_size(set, &n) == ZKGPU_OK ? (long long)n : -1; }
int zkSnSetContains(zk_snset *set, long long size, const uint8_t *sns, int n, unsigned char *in) {
  const int rc = guarded_snset(set, [&] {
    if (n < 0 || (n && (!sns || !in))) { zkgpu_set_error("zkSnSetContains: a negative count or a null pointer"); return ZKGPU_ERR_ARG; }
    std::vector<uint8_t> keys; sn_keys(sns, (size_t)n, keys); std::vector<uint64_t> index((size_t)n);
    if (!set->s.query(size < 0 ? 0 : (uint64_t)size, keys.data(), (size_t)n, index.data(), size < 0)) { zkgpu_set_error("zkSnSetContains: the set does not hold " + std::to_string(size) + " keys"); return ZKGPU_ERR_ARG; }
    for (int i = 0; i < n; i++) in[i] = index[i] != UINT64_MAX;
    return ZKGPU_OK; });
  if (rc != ZKGPU_OK) { fprintf(stderr, "libzkgpu: zkSnSetContains: %s\n", zkgpu_last_error()); return -1; }
  return 0;
}
long long zkSnSetRewind(zk_snset *set, long long size) {
  const int rc = guarded_snset(set, [&] {
    if (size < 0 || !set->s.rewind((uint64_t)size)) { zkgpu_set_error("zkSnSetRewind: the set does not hold " + std::to_string(size) + " keys"); return ZKGPU_ERR_ARG; }
    return ZKGPU_OK; });
  if (rc != ZKGPU_OK) { fprintf(stderr, "libzkgpu: zkSnSetRewind: %s\n", zkgpu_last_error()); return -1; }
  return size;
}
long long zkSnSetSpend(zk_snset *set, const uint8_t *sns, int n, int commit, unsigned char *spent) {
  uint64_t size = 0;
  const int rc = guarded_snset(set, [&] {
    if (n < 0 || (n && (!sns || !spent))) { zkgpu_set_error("zkSnSetSpend: a negative count or a null pointer"); return ZKGPU_ERR_ARG; }
    std::vector<uint8_t> keys, conflict((size_t)n); sn_keys(sns, (size_t)n, keys);
    if (!set->s.spend(keys.data(), nullptr, (size_t)n, commit != 0, conflict.data(), &size)) { zkgpu_set_error("zkSnSetSpend: the log would reach 2^32 - 2 entries"); return ZKGPU_ERR_ARG; }
    for (int i = 0; i < n; i++) spent[i] = conflict[i] != 0;
    return ZKGPU_OK; });
  if (rc != ZKGPU_OK) { fprintf(stderr, "libzkgpu: zkSnSetSpend: %s\n", zkgpu_last_error()); return -1; }
  return (long long)size;
}
static int block_full(const zk_block_record *recs, int n, const zk_cmt_lists *l, const int32_t *list_of, zk_snset *set, int commit, unsigned char *ok, long long *size_out,
                      zkgpu_proof_cache *cache = nullptr) {
  const int accepted = block_records_roots(recs, n, l, list_of, ok, cache); if (accepted < 0 || !set) return accepted;
  uint64_t size = 0; std::vector<uint8_t> conflict;
  const int rc = guarded_snset(set, [&] {
    std::vector<uint8_t> keys((size_t)20 * n); conflict.resize((size_t)n);
    { HostSpan span("host.sn_keys"); for (int i = 0; i < n; i++) memcpy(&keys[20 * (size_t)i], record_sn(recs[i]) + 12, 20); }
    if (!set->s.spend(keys.data(), ok, (size_t)n, commit != 0, conflict.data(), &size)) { zkgpu_set_error("the log would reach 2^32 - 2 entries"); return ZKGPU_ERR_ARG; }
    return ZKGPU_OK; });
  if (rc != ZKGPU_OK) { fprintf(stderr, "libzkgpu: verifyBlockFull: %s\n", zkgpu_last_error()); for (int i = 0; i < n; i++) ok[i] = 0; return -1; }
  int still = 0; for (int i = 0; i < n; i++) { if (conflict[i]) ok[i] = 0; still += ok[i] != 0; }
  if (size_out) *size_out = (long long)size;
  return still;
}
int verifyBlockFull(const zk_block_record *recs, int n, const zk_cmt_lists *l, const int32_t *list_of, zk_snset *set, int commit, unsigned char *ok, long long *size_out) {
  return block_full(recs, n, l, list_of, set, commit, ok, size_out); }
// include/zk_spent_pk.h: an all-zero pks[i] = record i has no second key
long long zkSnSetSpendPairs(zk_snset *set, const uint8_t *sns, const uint8_t *pks, int n, int commit, unsigned char *spent) {
  uint64_t size = 0;
  const int rc = guarded_snset(set, [&] {
    if (n < 0 || (n && (!sns || !spent))) { zkgpu_set_error("zkSnSetSpendPairs: a negative count or a null pointer"); return ZKGPU_ERR_ARG; }
    static const uint8_t none[32] = {0};
    std::vector<uint8_t> keys((size_t)40 * n), nkeys((size_t)n), conflict((size_t)n);
    for (int i = 0; i < n; i++) {
      memcpy(&keys[40 * (size_t)i], sns + 32 * (size_t)i + 12, 20); nkeys[i] = 1;
      if (pks && memcmp(pks + 32 * (size_t)i, none, 32)) { memcpy(&keys[40 * (size_t)i + 20], pks + 32 * (size_t)i + 12, 20); nkeys[i] = 2; }
    }
    if (!set->s.spend_pairs(keys.data(), nkeys.data(), (size_t)n, commit != 0, conflict.data(), &size)) { zkgpu_set_error("zkSnSetSpendPairs: the log could reach 2^32 - 2 entries"); return ZKGPU_ERR_ARG; }
    for (int i = 0; i < n; i++) spent[i] = conflict[i] != 0;
    return ZKGPU_OK; });
  if (rc != ZKGPU_OK) { fprintf(stderr, "libzkgpu: zkSnSetSpendPairs: %s\n", zkgpu_last_error()); return -1; }
  return (long long)size;
}
// the spend step on pairs: a record with ok[i] = 0 brings no key, a deposit its serial number and its one-time pk address (args[1][0..19]), every other record its
// serial number.  A record in conflict loses its ok.  Returns the records still accepted, or -1 with every ok[i] = 0 and the set unchanged.
static int block_spend_pairs(const zk_block_record *recs, int n, zk_snset *set, int commit, unsigned char *ok, uint64_t &size, const char *who) {
  std::vector<uint8_t> conflict;
  const int rc = guarded_snset(set, [&] {
    std::vector<uint8_t> keys((size_t)40 * n), nkeys((size_t)n); conflict.resize((size_t)n);
    { HostSpan span("host.sn_keys");
      for (int i = 0; i < n; i++) {
        uint8_t *k = &keys[40 * (size_t)i]; memcpy(k, record_sn(recs[i]) + 12, 20); nkeys[i] = !ok[i] ? 0 : recs[i].kind == ZK_KIND_DEPOSIT ? 2 : 1;
        if (recs[i].kind == ZK_KIND_DEPOSIT) memcpy(k + 20, recs[i].args[1], 20);
      } }
    if (!set->s.spend_pairs(keys.data(), nkeys.data(), (size_t)n, commit != 0, conflict.data(), &size)) { zkgpu_set_error("the log could reach 2^32 - 2 entries"); return ZKGPU_ERR_ARG; }
    return ZKGPU_OK; });
  if (rc != ZKGPU_OK) { fprintf(stderr, "libzkgpu: %s: %s\n", who, zkgpu_last_error()); for (int i = 0; i < n; i++) ok[i] = 0; return -1; }
  int still = 0; for (int i = 0; i < n; i++) { if (conflict[i]) ok[i] = 0; still += ok[i] != 0; }
  return still;
}
// block_full with the spend step on pairs
int verifyBlockState(zk_proof_cache *cache, const zk_block_record *recs, int n, const zk_cmt_lists *l, const int32_t *list_of, zk_snset *set, int commit, unsigned char *ok,
                     long long *size_out) {
  const int accepted = block_records_roots(recs, n, l, list_of, ok, cache); if (accepted < 0 || !set) return accepted;
  uint64_t size = 0; const int still = block_spend_pairs(recs, n, set, commit, ok, size, "verifyBlockState"); if (still < 0) return -1;
  if (size_out) *size_out = (long long)size;
  return still;
}

// ---- a block against the resident tree (DESIGN.md "A block against the resident tree"; include/zk_tree_block.h) -----------------------------------------------
// verifyBlockState's steps with the deposit key of the tree's depth, the anchor step on the device in place of the depth-8 lists, and the accepted sends' cmtS
// appended at the end.  The tree's mutex is held only inside size(), match_roots() and append(), never together with the cache's or the set's.
int verifyBlockTree(zk_proof_cache *cache, const zk_block_record *recs, int n, zk_tree *tree, const long long *anchors, int n_anchors, zk_snset *set, int commit,
                    unsigned char *ok, int32_t *anchor_of, long long *set_size_out, long long *tree_size_out) {
  if (!tree) {
    if (anchor_of) for (int i = 0; i < n; i++) anchor_of[i] = -1;
    if (tree_size_out) *tree_size_out = -1;
    return verifyBlockState(cache, recs, n, nullptr, nullptr, set, commit, ok, set_size_out);
  }
  auto fail = [&](const std::string &why) {
    zkgpu_set_error(why); fprintf(stderr, "libzkgpu: verifyBlockTree: %s\n", why.c_str());
    for (int i = 0; i < n; i++) { if (ok) ok[i] = 0; if (anchor_of) anchor_of[i] = -1; }
    return -1; };
  try {
    // 1. the arguments, before anything is queued
    if (n < 0 || (n && (!recs || !ok))) return fail("a negative count or a null pointer");
    if (n_anchors < 0 || (n_anchors && !anchors)) return fail("a negative number of anchors or a null pointer");
    if (!gpu_available()) return fail("no HIP device visible; libzkgpu has no CPU fallback");
    const size_t depth = (size_t)tree->t.depth(); const uint64_t size0 = tree->t.size();
    std::vector<uint64_t> sizes((size_t)n_anchors);
    for (int a = 0; a < n_anchors; a++) {
      if (anchors[a] < 0 || (uint64_t)anchors[a] > size0) return fail("anchor " + std::to_string(a) + " is negative or above the tree's size");
      sizes[a] = (uint64_t)anchors[a]; }
    if (commit) {
      uint64_t sends = 0; for (int i = 0; i < n; i++) sends += recs[i].kind == ZK_KIND_SEND;
      if (sends > (1ull << depth) - size0) return fail("the block's sends do not fit into the tree");
    }
    for (int i = 0; i < n; i++) if (anchor_of) anchor_of[i] = -1;
    // 2. the proof step, the deposits under the key of the tree's depth
    if (verify_block_records_cached(cache, recs, n, ok, "verifyBlockTree", depth) < 0) return fail(zkgpu_last_error());
    // 3. the anchor step: the RTs of the deposits still accepted, against the roots at the anchors
    std::vector<int> at; std::vector<uint8_t> gathered;
    { HostSpan span("host.tree_gather");
      for (int i = 0; i < n; i++) if (ok[i] && recs[i].kind == ZK_KIND_DEPOSIT) { at.push_back(i); gathered.insert(gathered.end(), recs[i].args[0], recs[i].args[0] + 32); } }
    if (!at.empty()) {
      std::vector<int32_t> match(at.size(), -1);
      if (!tree->t.match_roots(sizes.data(), sizes.size(), gathered.data(), at.size(), true, match.data())) return fail("an anchor is above the tree's size: the tree was rewound during the call");
      for (size_t j = 0; j < at.size(); j++) { if (match[j] < 0) ok[at[j]] = 0; else if (anchor_of) anchor_of[at[j]] = match[j]; }
    }
    // 4. the spend step
    int accepted = 0; uint64_t set_size = 0, set_before = 0;
    if (set) {
      if (commit) set_before = set->s.size();
      accepted = block_spend_pairs(recs, n, set, commit, ok, set_size, "verifyBlockTree"); if (accepted < 0) return fail(zkgpu_last_error());   // (a deposit that loses here keeps the anchor it matched)
    } else for (int i = 0; i < n; i++) accepted += ok[i] != 0;
    // 5. the append step: the cmtS of the sends still accepted, as zkTreeAppend makes its leaves, in one append
    if (commit) {
      gathered.clear();
      { HostSpan span("host.tree_gather");
        for (int i = 0; i < n; i++) if (ok[i] && recs[i].kind == ZK_KIND_SEND) for (int b = 0; b < 32; b++) gathered.push_back(recs[i].args[2][31 - b]); }
      bool appended = false; std::string why = "the tree is full: another writer appended during the call";
      try { appended = tree->t.append(gathered.empty() ? nullptr : gathered.data(), gathered.size() / 32); } catch (const std::exception &e) { why = e.what(); }
      if (!appended) {
        if (set) { try { set->s.rewind(set_before); } catch (const std::exception &e) { fprintf(stderr, "libzkgpu: verifyBlockTree: the spent set could not be rewound (%s)\n", e.what()); } }
        return fail(why);
      }
    }
    // 6. the sizes after the call
    if (set && set_size_out) *set_size_out = (long long)set_size;
    if (tree_size_out) *tree_size_out = (long long)tree->t.size();
    return accepted;
  }
  catch (const std::exception &e) { return fail(e.what()); }
  catch (...) { return fail("unknown error"); }
}

// ---- the account table at the drop-in level, and a block decided with it (DESIGN.md "Account table"; include/zk_accounts.h) -------------------------------------
zk_accts *zkAcctsNew(void) { return zkgpu_accts_create(); }
void zkAcctsFree(zk_accts *accts) { zkgpu_accts_destroy(accts); }
long long zkAcctsSize(zk_accts *accts) { uint64_t n = 0; return zkgpu_accts_size(accts, &n) == ZKGPU_OK ? (long long)n : -1; }
static int accts_rc(int rc, const char *who) { if (rc == ZKGPU_OK) return 0; fprintf(stderr, "libzkgpu: %s: %s\n", who, zkgpu_last_error()); return -1; }
int zkAcctsSet(zk_accts *accts, const uint8_t (*addrs)[20], const uint8_t (*values)[32], int n) {
  if (n < 0) { zkgpu_set_error("a negative count"); return accts_rc(ZKGPU_ERR_ARG, "zkAcctsSet"); }
  return accts_rc(zkgpu_accts_set(accts, (const uint8_t *)addrs, (const uint8_t *)values, (size_t)n), "zkAcctsSet"); }
int zkAcctsGet(zk_accts *accts, const uint8_t (*addrs)[20], int n, long long at_size, uint8_t (*out)[32]) {
  if (n < 0) { zkgpu_set_error("a negative count"); return accts_rc(ZKGPU_ERR_ARG, "zkAcctsGet"); }
  return accts_rc(zkgpu_accts_get(accts, (const uint8_t *)addrs, (size_t)n, (int64_t)at_size, (uint8_t *)out), "zkAcctsGet"); }
int zkAcctsRewind(zk_accts *accts, long long size) {
  if (size < 0) { zkgpu_set_error("a negative size"); return accts_rc(ZKGPU_ERR_ARG, "zkAcctsRewind"); }
  return accts_rc(zkgpu_accts_rewind(accts, (uint64_t)size), "zkAcctsRewind"); }
int zkAcctsFillRecords(zk_accts *accts, const uint8_t (*froms)[20], zk_block_record *recs, int n, int chained) {
  if (n < 0) { zkgpu_set_error("a negative count"); return accts_rc(ZKGPU_ERR_ARG, "zkAcctsFillRecords"); }
  return accts_rc(zkgpu_accts_fill(accts, (const uint8_t *)froms, recs, (size_t)n, chained), "zkAcctsFillRecords"); }
// The table's mutex is held only inside fill and commit_chain, never together with the cache's, the set's or the tree's: verifyBlockTree runs between the two.
int verifyBlockAccounts(zk_proof_cache *cache, zk_block_record *recs, const uint8_t (*froms)[20], int n, zk_accts *accts, zk_tree *tree, const long long *anchors,
                        int n_anchors, zk_snset *set, int commit, unsigned char *ok, int32_t *anchor_of, long long *accts_size_out, long long *set_size_out,
                        long long *tree_size_out) {
  auto fail = [&](const std::string &why) {
    zkgpu_set_error(why); fprintf(stderr, "libzkgpu: verifyBlockAccounts: %s\n", why.c_str());
    for (int i = 0; i < n; i++) { if (ok) ok[i] = 0; if (anchor_of) anchor_of[i] = -1; }
    return -1; };
  try {
    // 1. the arguments — verifyBlockTree's among them, which it looks at again — before anything is queued and before recs is written
    if (n < 0 || (n && (!recs || !ok || !froms))) return fail("a negative count or a null pointer");
    if (!accts) return fail("no account table");
    if (n_anchors < 0 || (n_anchors && !anchors)) return fail("a negative number of anchors or a null pointer");
    if (!gpu_available()) return fail("no HIP device visible; libzkgpu has no CPU fallback");
    if (tree) {
      const uint64_t size0 = tree->t.size();
      for (int a = 0; a < n_anchors; a++) if (anchors[a] < 0 || (uint64_t)anchors[a] > size0) return fail("anchor " + std::to_string(a) + " is negative or above the tree's size");
      if (commit) { uint64_t sends = 0; for (int i = 0; i < n; i++) sends += recs[i].kind == ZK_KIND_SEND; if (sends > (1ull << tree->t.depth()) - size0) return fail("the block's sends do not fit into the tree"); }
    }
    // 2. every record's old balance commitment from the table, chained through the block
    if (zkgpu_accts_fill(accts, (const uint8_t *)froms, recs, (size_t)n, 1) != ZKGPU_OK) return fail(zkgpu_last_error());
    // 3. verifyBlockTree's road on the statements as they now stand
    uint64_t set_before = 0, tree_before = 0;
    if (commit) { if (set) set_before = set->s.size(); if (tree) tree_before = tree->t.size(); }
    long long set_size = -1, tree_size = -1;
    if (verifyBlockTree(cache, recs, n, tree, anchors, n_anchors, set, commit, ok, anchor_of, &set_size, &tree_size) < 0) return -1;   // (it has written the failure's outputs)
    // 4. the first rejected record ends the block: what follows it was verified under an assumption that does not hold
    int f = 0; while (f < n && ok[f]) f++;
    auto take_back = [&]() -> bool {                                                                // the shrink of "A stretch of the chain": set and tree to their sizes before the call
      bool good = true;
      if (set) { try { good = set->s.rewind(set_before) && good; } catch (const std::exception &e) { good = false; fprintf(stderr, "libzkgpu: verifyBlockAccounts: the spent set could not be rewound (%s)\n", e.what()); } }
      if (tree) { try { good = tree->t.rewind(tree_before) && good; } catch (const std::exception &e) { good = false; fprintf(stderr, "libzkgpu: verifyBlockAccounts: the tree could not be rewound (%s)\n", e.what()); } }
      return good; };
    // a failure after verifyBlockTree has committed that the rewinds could not undo: the one -1 that may leave the set or the tree changed.  The three sizes as they
    // now are go to the caller, who can rewind to the sizes it stored before the call.
    auto fail_after = [&](const std::string &why) {
      if (accts_size_out) *accts_size_out = (long long)accts->a.size();
      if (set && set_size_out) *set_size_out = (long long)set->s.size();
      if (tree_size_out) *tree_size_out = tree ? (long long)tree->t.size() : -1;
      return fail(why + " (the sizes after the call are reported)"); };
    if (f < n) {
      for (int i = f + 1; i < n; i++) { ok[i] = 0; if (anchor_of) anchor_of[i] = -1; }
      if (commit) { if (!take_back()) return fail_after("the set or the tree could not be rewound: another writer changed it during the call"); set_size = (long long)set_before; if (tree) tree_size = (long long)tree_before; }
    } else if (commit && n) {
      if (zkgpu_accts_commit_chain(accts, (const uint8_t *)froms, recs, (size_t)n) != ZKGPU_OK) { const std::string why = zkgpu_last_error(); return take_back() ? fail(why) : fail_after(why + "; the set or the tree could not be rewound either"); }
    }
    if (accts_size_out) *accts_size_out = (long long)accts->a.size();
    if (set && set_size_out) *set_size_out = set_size;
    if (tree_size_out) *tree_size_out = tree_size;
    return f;
  }
  catch (const std::exception &e) { return fail(e.what()); }
  catch (...) { return fail("unknown error"); }
}

// ---- a stretch of the chain (DESIGN.md "A stretch of the chain"; include/zk_tree_chain.h) ----------------------------------------------------------------------
// The loop "verifyBlockTree(commit = 1) block after block, stop at the first block with a rejected record and take it back" without the loop: every step runs once on
// the longest prefix of blocks that can still be valid.  B1 >= B2 >= B3 are the first block with a record rejected by the proof step, by the anchor step, by the spend
// step; blocks < B3 are accepted, block B3's verdicts are already those of the loop (no later record changes an earlier one's verdict), and what was appended or spent
// beyond block B3 - 1 is rewound.  The tree's, the cache's and the set's mutexes are taken one step after the other, never together.
int verifyChainTree(zk_proof_cache *cache, const zk_block_record *recs, int n, const int *block_first, int n_blocks, zk_tree *tree, const long long *prior_anchors,
                    int n_prior, int window, zk_snset *set, unsigned char *ok, int32_t *anchor_of, long long *set_sizes, long long *tree_sizes) {
  bool appended = false, spent = false; uint64_t size0 = 0, set_before = 0;
  auto fail = [&](const std::string &why) {
    zkgpu_set_error(why); fprintf(stderr, "libzkgpu: verifyChainTree: %s\n", why.c_str());
    if (spent) { try { if (!set->s.rewind(set_before)) throw GpuError("it holds fewer keys than before the call"); } catch (const std::exception &e) { fprintf(stderr, "libzkgpu: verifyChainTree: the spent set could not be rewound (%s)\n", e.what()); } }
    if (appended) { try { if (!tree->t.rewind(size0)) throw GpuError("it holds fewer leaves than before the call"); } catch (const std::exception &e) { fprintf(stderr, "libzkgpu: verifyChainTree: the tree could not be rewound (%s)\n", e.what()); } }
    for (int i = 0; i < n; i++) { if (ok) ok[i] = 0; if (anchor_of) anchor_of[i] = -1; }
    return -1; };
  try {
    // 0. the arguments, before anything is queued
    if (!tree) return fail("no tree");
    if (n < 0 || n_blocks < 0 || (n && (!recs || !ok))) return fail("a negative count or a null pointer");
    if (!block_first || block_first[0] != 0 || block_first[n_blocks] != n) return fail("block_first does not run from 0 to n");
    for (int b = 0; b < n_blocks; b++) if (block_first[b] > block_first[b + 1]) return fail("block_first decreases at block " + std::to_string(b));
    if (n_prior < 0 || (n_prior && !prior_anchors)) return fail("a negative number of prior anchors or a null pointer");
    if (window < 0) return fail("a negative window");
    if (!gpu_available()) return fail("no HIP device visible; libzkgpu has no CPU fallback");
    const size_t depth = (size_t)tree->t.depth(); size0 = tree->t.size();
    for (int a = 0; a < n_prior; a++) if (prior_anchors[a] < 0 || (uint64_t)prior_anchors[a] > size0) return fail("prior anchor " + std::to_string(a) + " is negative or above the tree's size");
    { uint64_t sends = 0; for (int i = 0; i < n; i++) sends += recs[i].kind == ZK_KIND_SEND;
      if (sends > (1ull << depth) - size0) return fail("the segment's sends do not fit into the tree"); }
    for (int i = 0; i < n; i++) if (anchor_of) anchor_of[i] = -1;
    std::vector<int> blk((size_t)n); for (int b = 0; b < n_blocks; b++) for (int i = block_first[b]; i < block_first[b + 1]; i++) blk[i] = b;
    auto first_rejected = [&](int end) { for (int i = 0; i < end; i++) if (!ok[i]) return blk[i]; return n_blocks; };   // (end = block_first[B + 1] of a block B with a rejection, or n)
    auto end_of = [&](int B) { return block_first[B < n_blocks ? B + 1 : n_blocks]; };
    // 1. the proof step over every record, the deposits under the key of the tree's depth
    if (n && verify_block_records_cached(cache, recs, n, ok, "verifyChainTree", depth) < 0) return fail(zkgpu_last_error());
    const int B1 = first_rejected(n);
    // 2. the append: the cmtS of every send of the blocks < B1, in record order, in one append; s[b] = the tree's size after block b
    std::vector<uint64_t> s((size_t)B1); std::vector<uint8_t> gathered;
    { HostSpan span("host.tree_gather"); uint64_t at = size0;
      for (int b = 0; b < B1; b++) {
        for (int i = block_first[b]; i < block_first[b + 1]; i++) if (recs[i].kind == ZK_KIND_SEND) { at++; for (int k = 0; k < 32; k++) gathered.push_back(recs[i].args[2][31 - k]); }
        s[b] = at; } }
    if (!gathered.empty()) { if (!tree->t.append(gathered.data(), gathered.size() / 32)) return fail("the tree is full: another writer appended during the call"); appended = true; }
    // 3. the anchor step on the deposits of the blocks <= B1, each with its window of A = prior_anchors | s; the roots of the part of A that some window covers
    std::vector<int> at; std::vector<uint32_t> lo, hi; gathered.clear(); uint64_t a_lo = UINT64_MAX, a_hi = 0;
    { HostSpan span("host.tree_gather");
      for (int i = 0, end = end_of(B1); i < end; i++) if (ok[i] && recs[i].kind == ZK_KIND_DEPOSIT) {
        const uint64_t h = (uint64_t)n_prior + (uint64_t)blk[i], l = h > (uint64_t)window ? h - (uint64_t)window : 0;
        at.push_back(i); lo.push_back((uint32_t)l); hi.push_back((uint32_t)h); gathered.insert(gathered.end(), recs[i].args[0], recs[i].args[0] + 32);
        if (l < h) { a_lo = std::min(a_lo, l); a_hi = std::max(a_hi, h); } } }
    if (!at.empty()) {
      if (a_lo > a_hi) a_lo = a_hi = 0;                                                           // (every window is empty)
      std::vector<uint64_t> sizes((size_t)(a_hi - a_lo)); std::vector<int32_t> match(at.size(), -1);
      for (uint64_t a = a_lo; a < a_hi; a++) sizes[a - a_lo] = a < (uint64_t)n_prior ? (uint64_t)prior_anchors[a] : s[a - (uint64_t)n_prior];   // (a - n_prior < blk[i] <= B1)
      for (size_t j = 0; j < at.size(); j++) { if (lo[j] < hi[j]) { lo[j] -= (uint32_t)a_lo; hi[j] -= (uint32_t)a_lo; } else lo[j] = hi[j] = 0; }
      if (!tree->t.match_roots_window(sizes.data(), sizes.size(), gathered.data(), at.size(), lo.data(), hi.data(), true, match.data())) return fail("an anchor is above the tree's size: the tree was rewound during the call");
      for (size_t j = 0; j < at.size(); j++) { if (match[j] < 0) ok[at[j]] = 0; else if (anchor_of) anchor_of[at[j]] = match[j] + (int32_t)a_lo; }
    }
    const int B2 = first_rejected(end_of(B1));
    // 4. the spend step over the records of the blocks <= B2; a record rejected above brings no key
    const int end2 = end_of(B2); uint64_t set_size = 0; std::vector<uint64_t> set_at((size_t)n_blocks);
    if (set) {
      set_size = set_before = set->s.size(); spent = true;                                        // (a call that fails leaves the set alone, and a rewind to its own size is nothing)
      if (end2 && block_spend_pairs(recs, end2, set, 1, ok, set_size, "verifyChainTree") < 0) return fail(zkgpu_last_error());
    }
    const int B3 = first_rejected(end2);
    // 5. the sizes of the set after each accepted block: an accepted record inserts its serial number unless that is the exempt key (which is never inserted), and a
    //    deposit its pk address.  Then the shrink: what lies beyond block B3 - 1 is taken back.  A segment accepted whole rewinds nothing.
    if (set) {
      uint8_t exempt[20]; const bool has_exempt = set->s.exempt_key(exempt); uint64_t at_set = set_before;
      for (int b = 0; b < B3; b++) {
        for (int i = block_first[b]; i < block_first[b + 1]; i++) at_set += (!(has_exempt && !memcmp(record_sn(recs[i]) + 12, exempt, 20)) ? 1 : 0) + (recs[i].kind == ZK_KIND_DEPOSIT ? 1 : 0);
        set_at[b] = at_set; }
      if (at_set > set_size || (B3 == n_blocks && at_set != set_size)) return fail("the spent set's size after the call is not what the accepted records account for");
      if (at_set != set_size) { if (!set->s.rewind(at_set)) return fail("the spent set could not be rewound to the end of block " + std::to_string(B3 - 1)); set_size = at_set; }
    }
    const uint64_t tree_size = B3 ? s[B3 - 1] : size0;
    if (tree_size != (B1 ? s[B1 - 1] : size0) && !tree->t.rewind(tree_size)) return fail("the tree could not be rewound to the end of block " + std::to_string(B3 - 1));
    // 6. the verdicts: block B3's are those of the loop already; the blocks after it are not decided
    for (int i = end_of(B3); i < n; i++) { ok[i] = 0; if (anchor_of) anchor_of[i] = -1; }
    for (int b = 0; b < n_blocks; b++) {
      if (set && set_sizes) set_sizes[b] = (long long)(b < B3 ? set_at[b] : set_size);
      if (tree_sizes) tree_sizes[b] = (long long)(b < B3 ? s[b] : tree_size); }
    return B3;
  }
  catch (const std::exception &e) { return fail(e.what()); }
  catch (...) { return fail("unknown error"); }
}

// ---- a stretch of the chain with accounts (DESIGN.md "A stretch of the chain with accounts"; include/zk_accounts_chain.h) ----------------------------------------
// The loop "verifyBlockAccounts(commit = 1) block after block, stop at the first block that is not accepted whole" without the loop: one chained fill over the whole
// segment (the tiled search), verifyChainTree on the filled records, the cut at the first rejection of the first rejected block, one append of the accepted blocks'
// records.  The table's mutex is held only inside the two segment calls, never together with the cache's, the set's or the tree's.
int verifyChainAccounts(zk_proof_cache *cache, zk_block_record *recs, const uint8_t (*froms)[20], int n, const int *block_first, int n_blocks, zk_accts *accts,
                        zk_tree *tree, const long long *prior_anchors, int n_prior, int window, zk_snset *set, unsigned char *ok, int32_t *anchor_of,
                        long long *accts_sizes, long long *set_sizes, long long *tree_sizes) {
  auto fail = [&](const std::string &why) {
    zkgpu_set_error(why); fprintf(stderr, "libzkgpu: verifyChainAccounts: %s\n", why.c_str());
    for (int i = 0; i < n; i++) { if (ok) ok[i] = 0; if (anchor_of) anchor_of[i] = -1; }
    return -1; };
  try {
    // 0. the arguments — verifyChainTree's among them, which it looks at again — before recs is written or anything is queued
    if (!tree) return fail("no tree");
    if (n < 0 || n_blocks < 0 || (n && (!recs || !ok || !froms))) return fail("a negative count or a null pointer");
    if (!accts) return fail("no account table");
    if (!block_first || block_first[0] != 0 || block_first[n_blocks] != n) return fail("block_first does not run from 0 to n");
    for (int b = 0; b < n_blocks; b++) if (block_first[b] > block_first[b + 1]) return fail("block_first decreases at block " + std::to_string(b));
    if (n_prior < 0 || (n_prior && !prior_anchors)) return fail("a negative number of prior anchors or a null pointer");
    if (window < 0) return fail("a negative window");
    if (!gpu_available()) return fail("no HIP device visible; libzkgpu has no CPU fallback");
    const uint64_t tree_before = tree->t.size(), set_before = set ? set->s.size() : 0, accts_before = accts->a.size();
    for (int a = 0; a < n_prior; a++) if (prior_anchors[a] < 0 || (uint64_t)prior_anchors[a] > tree_before) return fail("prior anchor " + std::to_string(a) + " is negative or above the tree's size");
    { uint64_t sends = 0; for (int i = 0; i < n; i++) sends += recs[i].kind == ZK_KIND_SEND;
      if (sends > (1ull << tree->t.depth()) - tree_before) return fail("the segment's sends do not fit into the tree"); }
    if (accts_before + (uint64_t)n >= 0xFFFFFFFEull) return fail("the segment's records do not fit into the account table's log");
    // 1. every record's old balance commitment from the table, chained through the whole segment
    if (n && zkgpu_accts_fill_segment(accts, (const uint8_t *)froms, recs, (size_t)n) != ZKGPU_OK) return fail(zkgpu_last_error());
    // 2. verifyChainTree's road on the statements as they now stand; a failure there has rewound what it did and written the failure's outputs
    std::vector<long long> set_at((size_t)n_blocks + 1), tree_at((size_t)n_blocks + 1); std::vector<uint64_t> accts_at((size_t)n_blocks + 1, 0);   // (nothing below allocates once the set and the tree are written)
    const int B = verifyChainTree(cache, recs, n, block_first, n_blocks, tree, prior_anchors, n_prior, window, set, ok, anchor_of, set_at.data(), tree_at.data());
    if (B < 0) return -1;
    // 3. the first rejected record f of the first rejected block ends the decided part: what follows it in the block was verified under an assumption that failed
    if (B < n_blocks) {
      int f = block_first[B]; while (f < block_first[B + 1] && ok[f]) f++;
      for (int i = f; i < block_first[B + 1]; i++) { ok[i] = 0; if (anchor_of && i > f) anchor_of[i] = -1; }
    }
    // 4. the records of the accepted blocks become entries of the table, in one append; the table's size after each block follows from the records with kind <= 3
    const int end = block_first[B];
    { uint64_t at = accts_before;
      for (int b = 0; b < n_blocks; b++) { if (b < B) for (int i = block_first[b]; i < block_first[b + 1]; i++) at += recs[i].kind <= 3; accts_at[b] = at; } }
    if (end) {
      std::string why; bool good = zkgpu_accts_commit_segment(accts, (const uint8_t *)froms, recs, (size_t)end) == ZKGPU_OK;
      if (!good) why = zkgpu_last_error();
      else if (accts->a.size() != (B ? accts_at[B - 1] : accts_before)) { good = false; why = "the account table's size after the call is not what the accepted records account for: another writer changed it during the call"; }
      if (!good) {                                                                                  // 5. the set and the tree go back to their sizes before the call
        bool back = true;
        if (set) { try { back = set->s.rewind(set_before) && back; } catch (const std::exception &e) { back = false; fprintf(stderr, "libzkgpu: verifyChainAccounts: the spent set could not be rewound (%s)\n", e.what()); } }
        try { back = tree->t.rewind(tree_before) && back; } catch (const std::exception &e) { back = false; fprintf(stderr, "libzkgpu: verifyChainAccounts: the tree could not be rewound (%s)\n", e.what()); }
        if (!back && n_blocks) {                                                                    // the one -1 that may leave the set or the tree changed: the sizes as they now are
          if (accts_sizes) accts_sizes[n_blocks - 1] = (long long)accts->a.size();
          if (set && set_sizes) set_sizes[n_blocks - 1] = (long long)set->s.size();
          if (tree_sizes) tree_sizes[n_blocks - 1] = (long long)tree->t.size();
          why += "; the set or the tree could not be rewound either (the sizes after the call are reported)";
        }
        return fail(why);
      }
    }
    for (int b = 0; b < n_blocks; b++) {
      if (accts_sizes) accts_sizes[b] = (long long)accts_at[b];
      if (set && set_sizes) set_sizes[b] = set_at[b];
      if (tree_sizes) tree_sizes[b] = tree_at[b]; }
    return B;
  }
  catch (const std::exception &e) { return fail(e.what()); }
  catch (...) { return fail("unknown error"); }
}

// ---- the proof cache (DESIGN.md "Proof cache"; include/zkgpu.h, include/zk_proof_cache.h) ----------------------------------------------------------------------
static zkgpu_proof_cache *proof_cache_create(uint64_t capacity, const uint8_t *salt) {
  zkgpu_proof_cache *c = nullptr;
  try {
    if (!gpu_available()) { zkgpu_set_error("no HIP device visible; libzkgpu has no CPU fallback"); return nullptr; }
    if (capacity < 2) { zkgpu_set_error("proof cache: a capacity of 2 entries or more"); return nullptr; }
    c = new zkgpu_proof_cache(capacity, salt);
  }
  catch (const std::exception &e) { zkgpu_set_error(e.what()); } catch (...) { zkgpu_set_error("unknown error"); }
  return c;
}
zkgpu_proof_cache *zkgpu_proof_cache_create(uint64_t capacity) { return proof_cache_create(capacity, nullptr); }
zkgpu_proof_cache *zkgpu_test_proof_cache_create(uint64_t capacity, const uint8_t salt[32]) {
  if (!salt) { zkgpu_set_error("proof cache: no salt"); return nullptr; }
  return proof_cache_create(capacity, salt); }
void zkgpu_proof_cache_destroy(zkgpu_proof_cache *c) { try { delete c; } catch (...) {} }
int zkgpu_proof_cache_clear(zkgpu_proof_cache *c) { return guarded_cache(c, [&] { c->c.clear(); return ZKGPU_OK; }); }
int zkgpu_proof_cache_stats(zkgpu_proof_cache *c, uint64_t out[4]) { return guarded_cache(c, [&] { if (!out) return ZKGPU_ERR_ARG; c->c.stats(out); return ZKGPU_OK; }); }
int zkgpu_test_record_digests(const uint8_t salt[32], const uint8_t tags[4][32], const zk_block_record *recs, size_t n, int device, uint8_t *out20) { return guarded_host([&] {
  if (!salt || !tags || (n && (!recs || !out20))) { zkgpu_set_error("record digests: a null pointer"); return ZKGPU_ERR_ARG; }
  if (device && !gpu_available()) { zkgpu_set_error("no HIP device visible; libzkgpu has no CPU fallback"); return ZKGPU_ERR_NO_DEVICE; }
  record_digests(salt, tags, 0xfu, recs, n, device != 0, out20); return ZKGPU_OK; }); }
int zkgpu_test_proof_cache_launches(uint64_t *launches) { if (!launches) return ZKGPU_ERR_ARG; *launches = record_digest_launches(); return ZKGPU_OK; }

zk_proof_cache *zkProofCacheNew(long long capacity) { return capacity < 2 ? nullptr : zkgpu_proof_cache_create((uint64_t)capacity); }
void zkProofCacheFree(zk_proof_cache *cache) { zkgpu_proof_cache_destroy(cache); }
int zkProofCacheClear(zk_proof_cache *cache) {
  if (zkgpu_proof_cache_clear(cache) == ZKGPU_OK) return 0;
  fprintf(stderr, "libzkgpu: zkProofCacheClear: %s\n", zkgpu_last_error()); return -1; }
int zkProofCacheStats(zk_proof_cache *cache, uint64_t out[4]) { return zkgpu_proof_cache_stats(cache, out) == ZKGPU_OK ? 0 : -1; }
int verifyRecordsCached(zk_proof_cache *cache, const zk_block_record *recs, int n, unsigned char *ok) {
  if (n < 0 || (n && (!recs || !ok))) return -1;
  return verify_block_records_cached(cache, recs, n, ok, "verifyRecordsCached"); }
int verifyBlockFullCached(zk_proof_cache *cache, const zk_block_record *recs, int n, const zk_cmt_lists *l, const int32_t *list_of, zk_snset *set, int commit, unsigned char *ok,
                          long long *size_out) { return block_full(recs, n, l, list_of, set, commit, ok, size_out, cache); }

// the reference's symbol names, exported by libzkgpu.so itself (the four libzk_*.so forward to the zkgpu_abi_* names above)
char *genCMT(uint64_t v, char *a, char *b) { return zkgpu_abi_genCMT(v, a, b); }
char *genCMTS(uint64_t v, char *a, char *b, char *c) { return zkgpu_abi_genCMTS(v, a, b, c); }
char *computePRF(char *a, char *b) { return zkgpu_abi_computePRF(a, b); }
char *computeCRH(char *a, char *b) { return zkgpu_abi_computeCRH(a, b); }
char *genRoot(char *a, int n) { return zkgpu_abi_genRoot(a, n); }
char *genMintproof(uint64_t a, uint64_t b, char *c, char *d, char *e, char *f, char *g, char *h, uint64_t i, char *j) {
  return zkgpu_abi_genMintproof(a, b, c, d, e, f, g, h, i, j);
}
bool verifyMintproof(char *a, char *b, char *c, char *d, uint64_t e) { return zkgpu_abi_verifyMintproof(a, b, c, d, e); }
char *genRedeemproof(uint64_t a, uint64_t b, char *c, char *d, char *e, char *f, char *g, char *h, uint64_t i, char *j) {
  return zkgpu_abi_genRedeemproof(a, b, c, d, e, f, g, h, i, j);
}
bool verifyRedeemproof(char *a, char *b, char *c, char *d, uint64_t e) { return zkgpu_abi_verifyRedeemproof(a, b, c, d, e); }
char *genSendproof(uint64_t a, char *b, char *c, char *d, char *e, char *f, uint64_t g, char *h, uint64_t i, char *j, char *k, char *l, char *m, char *n) {
  return zkgpu_abi_genSendproof(a, b, c, d, e, f, g, h, i, j, k, l, m, n);
}
bool verifySendproof(char *a, char *b, char *c, char *d, char *e) { return zkgpu_abi_verifySendproof(a, b, c, d, e); }
char *genDepositproof(uint64_t a, uint64_t b, char *c, char *d, char *e, char *f, char *g, char *h, char *i, char *j, uint64_t k, char *l, char *m, char *n,
    char *o, int p, char *q, char *r) {
  return zkgpu_abi_genDepositproof(a, b, c, d, e, f, g, h, i, j, k, l, m, n, o, p, q, r);
}
bool verifyDepositproof(char *a, char *b, char *c, char *d, char *e, char *f, char *g) { return zkgpu_abi_verifyDepositproof(a, b, c, d, e, f, g); }
}  // extern "C"
