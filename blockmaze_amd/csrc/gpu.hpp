// Host-side interface to the HIP kernels (implemented in gpu.hip).  Plain pointers and sizes only; device buffers are
// owned by the objects declared here.  Everything runs on one HIP stream per GpuContext; results that the host needs
// come back through pinned buffers after a single stream synchronisation.
#pragma once
#include <cstddef>
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>
#include "hostmath.hpp"
#include "pairing_host.hpp"

namespace zk {

struct GpuError : std::runtime_error { using std::runtime_error::runtime_error; };
struct GpuOutOfMemory : GpuError { using GpuError::GpuError; };   // a device allocation that did not fit (DevBuf): the one failure a caller may answer by asking for less
uint64_t queries_without_tables();   // key queries loaded without their fixed-base tables because the tables did not fit the device (the prover is then several times slower on them)
void note_query_without_tables();

// raw 32-byte field element / point records as they sit in HBM (Montgomery form, little-endian limbs)
struct Fe32 { uint32_t l[8]; };
struct G1AffineRaw { Fe32 x, y; };            // 64 B
struct G2AffineRaw { Fe32 x0, x1, y0, y1; };  // 128 B

class GpuContext;
GpuContext &gpu();                             // lazily initialised process-wide context (device from ZK_DEVICE / LOCAL_RANK)
int gpu_device_numa_node(int device);            // NUMA node of the socket the device hangs off, -1 unknown (sysfs)
bool gpu_available();                          // false if no HIP device is visible
int lane_plan_simulate(int n_slots, int kinds, int per_kind, int *out_lanes_per_slot);   // the lane planner on a private table (CPU tests)
// independent stream sets (gpu.hip); a lane belongs to one device of the list below
int gpu_lane_acquire(int device_slot = 0);
void gpu_lane_release(int lane);
int gpu_lane_current();
void gpu_lane_select(int lane);
// The devices this process works on: ZK_DEVICES = "all" or a comma-separated list of HIP device indices; without it the single device ZK_DEVICE / LOCAL_RANK
// (default 0) as before. Slot k of the list is what device_slot arguments mean. A plain go-ethereum process calling the cgo symbols from many goroutines
// thereby uses every GPU of the node: the key pool holds provers on each device (capi_zk.cpp) and spreads the callers over them.
int gpu_device_slots(); int gpu_slot_of_lane(int lane);
std::vector<int> parse_device_list(const char *spec, int n_visible, int fallback_device);   // pure function (unit-tested on the CPU)
struct LaneScope { int prev; explicit LaneScope(int lane) : prev(gpu_lane_current()) { gpu_lane_select(lane); } ~LaneScope() { gpu_lane_select(prev);
    } LaneScope(const LaneScope &) = delete; };

template <class T> class DevBuf {              // RAII device allocation
 public:
  DevBuf() = default; explicit DevBuf(size_t n); ~DevBuf(); DevBuf(DevBuf &&o) noexcept; DevBuf &operator=(DevBuf &&o) noexcept;
  DevBuf(const DevBuf &) = delete; DevBuf &operator=(const DevBuf &) = delete;
  T *get() const { return p_; } size_t size() const { return n_; }
  void upload(const T *host, size_t n); void download(T *host, size_t n) const; void zero();
 private:
  T *p_ = nullptr; size_t n_ = 0;
};

template <class T> class PinnedBuf {           // page-locked host staging buffer
 public:
  PinnedBuf() = default; explicit PinnedBuf(size_t n); ~PinnedBuf(); PinnedBuf(const PinnedBuf &) = delete; PinnedBuf &operator=(const PinnedBuf &) = delete;
  PinnedBuf &operator=(PinnedBuf &&o) noexcept { if (this != &o) { release(); p_ = o.p_; n_ = o.n_; o.p_ = nullptr; o.n_ = 0; } return *this; }
  T *get() const { return p_; } size_t size() const { return n_; }
 private:
  void release(); T *p_ = nullptr; size_t n_ = 0;
};
void upload_async(void *dev, const void *pinned_host, size_t bytes);   // on the main stream, no synchronisation
void copy_dev_async(void *dst, const void *src, size_t bytes);          // device to device, on the main stream, no synchronisation

// A fixed set of base points resident in HBM (one query of a proving key) plus the reusable MSM workspace for it.
struct WsortBuffers;                           // the sorted witness digits an MSM leaves for the MSMs over the same scalar vector (msm_impl.hpp)
// An assignment that arrived in compact form (Prover::set_witness*), as the witness MSMs' sort (msm.cuh: k_wsort_tagged) wants it: device pointers, valid for
// the run that follows
struct WitnessTags {
  const uint8_t *tags = nullptr;        // one byte per variable (variable 0 = ONE): 0 the value is zero, 1 it is one, 2 anything else
  const uint32_t *other_vars = nullptr; // the variables tagged 2, ascending
  uint32_t n_other = 0;                // the list's length — or, with n_other_dev set, an upper bound of it (it sizes the launch)
  const uint32_t *n_other_dev = nullptr; // the length in device memory, where the list was made on the device (k_classify_witness): no trip to the host
  // indexed queries (B): position of a variable in the query's index list, 0xffffffff if it has no point; null for plain queries
  const uint32_t *var_pos = nullptr;
  uint32_t base = 0;                    // plain query: point i belongs to variable base + i; indexed query: first position of this slice of the index list
};
// test entry points of the three-launch witness path (zkgpu_test_msm_wpath), both groups: out[0..19] = fused (0 / 1), c, W, NB | slots a bucket (WsortBuffers::cap), any
// point at infinity, result slots, leader (1) or follower (0) of its sort | the sort is shared, the flag word of the last synchronised fused run (MsmCounters::pad[0],
// read before a fallback: bit 0 a bucket overflowed, bit 1 a degenerate sum, G1 with its result slots from bit 8 on), that run's ones-list length, bucket lanes in use
// (lane_off[NB]) | its slice length T, WFUSED_BUCKET_LANES, WFUSED_ONES_LANES, WFUSED_MIN_SLICE | bucket arrays, stream (0 main, 1..4 auxiliary), top = log2(NB), WTAIL_SLOTS.
// test_w_state, after a synchronised fused run that did not fall back: what = 0 the current parity's fill (NB words), 1 lane_off (NB + 1), 2 the ones list, 3 every
// bucket's entries end to end (min(fill, cap) words each).  Returns the words written; throws if cap_words is too small or the object is not on that path.
constexpr int MSM_WPATH_WORDS = 20;
class MsmG1 {
 public:
  // tables: precompute 2^(cw) P if the size cap allows; uniform: one-pass sort with overflow fallback (msm_impl.hpp)
  MsmG1(const G1AffineRaw *host_points, size_t n, int window_bits, bool filter_ones, bool fixed_base_tables = true, bool uniform_scalars = false);
  // shares the peer's resident points / fixed-base table (immutable); owns only its workspace
  MsmG1(const MsmG1 &peer, bool filter_ones, bool uniform_scalars);
  ~MsmG1();
  // scalars_dev: Fr (Montgomery) on the device.  scalar_index_dev: optional gather map (point i uses scalars[index[i]]).
  // Enqueues the kernels; result() synchronises and finishes the combine on the host.
  void run(const Fe32 *scalars_dev, const uint32_t *scalar_index_dev);
  // the same with the whole assignment z_all (variable 0 = ONE) and its tags: the three-launch witness path then sorts from the tags (other paths read the
  // scalars as run() does)
  void run_tagged(const Fe32 *z_all_dev, const WitnessTags &wt, const uint32_t *scalar_index_dev);
  // scalars a_i * b_i * z (z: one element, or a table of n) formed inside the sort kernel; only when one_pass_sort() (uniform-scalar MSM with fixed-base
  // tables)
  bool one_pass_sort() const; void run_product(const Fe32 *a_dev, const Fe32 *b_dev, const Fe32 *z_dev, bool z_is_table);
  void set_crowded(bool other_proofs_in_flight);   // uniform-scalar path: longer accumulation runs while the chip is shared with other proofs (msm_impl.hpp: h_run_crowded)
  host::HG1 result();
  // MSMs over the same scalar vector (same length, same window) can share one sort of its digits: the follower must be run after the leader, on the leader's
  // stream or on another one (it then waits for the leader's event). false if either side is not on the three-launch witness path.
  std::shared_ptr<WsortBuffers> sort_handle() const; bool share_sort_with(const std::shared_ptr<WsortBuffers> &leader);
  // split: the scalar-one sum runs on a stream of its own beside the bucket path
  size_t size() const;
  const G1AffineRaw *points_dev() const;
  void set_label(const char *l);
  void set_stream(int aux /* -1 main, 0..3 auxiliary */);
  void split_ones_path();
  // test entry points (zkgpu_test_msm_*): what the constructor decided — out[0..23] = one_pass_sort, c, W, NB | HsortShape groups, low_bits, idx_bits, region |
  // h_run, h_maxp, htail29, lane exponent of the last combine | the run in effect (crowded or not), any point at infinity, WB, result slots | HtailShape top,
  // lo_bits, hi_bits, row_chunks | workgroup size of k_hmarg29, its workgroups, marginal records, the flag word of the last one-pass run (MsmCounters::pad[0]: bit 0 an
  // overflow or a degenerate bucket sum, bit 1 a degenerate sum of the tail with its result slots from bit 8 on) — and what the last synchronised one-pass run left on the
  // device: what = 0 counts, 1 offsets (a word a bucket), 2 entries of each group, 3 the sorted entries (groups x region), 4 the bucket sums (Point29Rec, 48 words
  // a bucket).  Returns the number of words written; throws if `cap_words` is too small or the object has no such state.
  static constexpr int TEST_PATH_WORDS = 24;
  void test_path(uint32_t out[TEST_PATH_WORDS]) const; size_t test_h_state(int what, uint32_t *out, size_t cap_words);
  void test_wpath(uint32_t out[MSM_WPATH_WORDS]); size_t test_w_state(int what, uint32_t *out, size_t cap_words);
  struct Impl; std::unique_ptr<Impl> impl;
};
class MsmG2 {
 public:
  MsmG2(const G2AffineRaw *host_points, size_t n, int window_bits, bool filter_ones, bool fixed_base_tables = true, bool uniform_scalars = false);
  MsmG2(const MsmG2 &peer, bool filter_ones, bool uniform_scalars);
  ~MsmG2();
  void run(const Fe32 *scalars_dev, const uint32_t *scalar_index_dev);
  void run_tagged(const Fe32 *z_all_dev, const WitnessTags &wt, const uint32_t *scalar_index_dev);
  std::shared_ptr<WsortBuffers> sort_handle() const; bool share_sort_with(const std::shared_ptr<WsortBuffers> &leader);
  host::HG2 result(); void set_label(const char *l); void set_stream(int aux); void split_ones_path();
  void test_wpath(uint32_t out[MSM_WPATH_WORDS]); size_t test_w_state(int what, uint32_t *out, size_t cap_words);   // as MsmG1's
  struct Impl; std::unique_ptr<Impl> impl;
};

// Batched Groth16 verification on the GPU (kernel K9, pairing.cuh): one lane per proof, the key-dependent tables and the verification program resident in HBM.
class BatchVerifier {
 public:
  // all Montgomery, affine
  BatchVerifier(const host::HFq12 &alpha_g1_beta_g2, const G2AffineRaw &gamma_g2, const G2AffineRaw &delta_g2, const G1AffineRaw *ic, size_t n_ic);
  ~BatchVerifier();
  size_t num_inputs() const; size_t program_length() const;
  void counters(uint64_t out[2]) const;   // small calls taken / launches made for them (calls that meet share a launch)
  void path_counters(uint64_t out[4]) const;   // the two above, then launches of the large-batch branches: workgroup per proof, lane per proof
  // proofs_mont: n records of 256 bytes (A.x A.y | B.x.c0 B.x.c1 B.y.c0 B.y.c1 | C.x C.y, Montgomery); inputs: n * num_inputs() canonical field elements; ok[i]
  // = 1 accept / 0 reject
  void verify(const void *proofs_mont, const Fe32 *inputs_canonical, size_t n, uint8_t *ok);
  uint8_t trace(const void *proof_mont, const Fe32 *inputs_canonical, uint32_t every, std::vector<uint32_t> &values, uint8_t nacc_out[96]);   // tests (gpu_verify.hip)
  struct Impl; std::unique_ptr<Impl> impl;
};
// The device half of the randomized block check (gpu_verify_block.hip): one lane per record.  ic_x / ic_y: the prepared key's window tables of IC[1..]
// ([j][w*255 + d-1], affine Montgomery, (0,0) = infinity).
class BlockVerifier {
 public:
  BlockVerifier(const host::HFq *ic_x, const host::HFq *ic_y, size_t n_inputs, const G1AffineRaw &ic0);
  ~BlockVerifier();
  size_t num_inputs() const;
  // weights: n x 16 bytes (little-endian 128-bit r_i).  flags[i]: 1 in the equation, 0 rejected by the screen, 2 input accumulator at infinity.  prod = the product of
  // Miller(A_i, B_i)^{r_i}, sum_c = the sum of r_i C_i, both over the records flagged 1
  void run(const void *proofs_mont, const Fe32 *inputs_canonical, const uint8_t *weights, size_t n, uint8_t *flags, host::HFq12 &prod, host::HG1 &sum_c);
  // run() on arrays that already lie in device memory (RecordIngest below).  parsed_dev: one byte per record, ANDed into the screen — an unparsed record gets flag 0
  // whatever its zeroed points are.  sums: (num_inputs() + 1) x 7 words, the integers sum r_i and sum r_i x_ij over the records flagged 1 (k_block_scalar_sums), what
  // rlc_int_sums makes on the host.  The call's workspace is kept by the verifier and grown on demand: one caller at a time (the device mutex).
  void run_resident(const void *items_dev, const Fe32 *inputs_dev, const uint8_t *parsed_dev, const uint8_t *weights, size_t n, uint8_t *flags, host::HFq12 &prod,
      host::HG1 &sum_c, uint64_t *sums);
  struct Impl; std::unique_ptr<Impl> impl;
 private:
  void run_resident_unsynced(const void *items_dev, const Fe32 *inputs_dev, const uint8_t *parsed_dev, const uint8_t *weights, size_t n, uint8_t *flags,
      host::HFq12 &prod, host::HG1 &sum_c, uint64_t *sums);
};
// Device ingest of block records (gpu_verify_ingest.hip; include/zk_records.h): n records of ONE kind, 720 bytes each, written by the caller into stage(n) — pinned
// memory, kept and grown —, then run(): one upload and k_ingest_records on the main stream, no synchronisation.  What it leaves in device memory is what
// BlockVerifier::run uploads: 256-byte proof records (affine, Montgomery; all zero where the 512 characters are not a proof), record_num_inputs(kind) canonical field elements a
// record, and a `parsed` byte.  strict: a coordinate of q or more is not a proof (ZK_STRICT_PROOF_ENCODING).  One caller at a time (the device mutex).
size_t record_num_inputs(int kind);   // 4 / 5 / 6 / 4 packed inputs for mint / send / deposit / redeem (832 / 1,024 / 1,440 / 832 bits), 0 for an unknown kind
class RecordIngest {
 public:
  RecordIngest(); ~RecordIngest();
  uint8_t *stage(size_t n);
  void run(size_t n, int kind, bool strict);
  const void *items_dev() const; const Fe32 *inputs_dev() const; const uint8_t *parsed_dev() const;
  void download(size_t first, size_t count, void *items, Fe32 *inputs, uint8_t *parsed);   // any of the three may be null; synchronises the main stream
  struct Impl; std::unique_ptr<Impl> impl;
};
// k_block_scalar_sums on the main stream: out = (n_inputs + 1) x 7 words in device memory; partials: block_scalar_sums_scratch(n_inputs) words of scratch
size_t block_scalar_sums_scratch(size_t n_inputs);
void block_scalar_sums_dev(const Fe32 *inputs, size_t n_inputs, const uint8_t *weights, const uint8_t *flags, size_t n, uint64_t *partials, uint64_t *out);

// The commitment tree of the deposit circuit, resident in HBM (gpu_tree.hip): an append-only SHA-256 Merkle tree of depth 1..32 with all-zero unseen leaves,
// the tree of notes.cpp:tree_levels.  Leaves, siblings and roots are 32-byte blobs in blob byte order.  One mutex per tree: append, root, path, find, snapshot and the
// past-state entries are each atomic with respect to the others, and each runs on the main stream under the device mutex.
class CommitmentTree {
 public:
  // one state of the tree seen under one lock: a proof must never pair the path of one state with the root of another
  struct Snapshot { uint64_t index = 0, size = 0; uint8_t root[32]; std::vector<uint8_t> path /* depth x 32, leaf level first */; std::vector<bool> index_bits; };
  explicit CommitmentTree(int depth);
  ~CommitmentTree();
  int depth() const; uint64_t size() const;
  bool append(const uint8_t *leaves, size_t n);                      // false: the tree would hold more than 2^depth leaves; nothing changed
  void root(uint8_t out[32]);
  bool path(uint64_t index, uint8_t *siblings /* depth x 32 */);      // false: no such leaf
  bool find(const uint8_t leaf[32], uint64_t &index);                // the first leaf equal to the blob; false: none
  bool snapshot(const uint8_t leaf[32], Snapshot &out);              // false: the leaf is not in the tree (size and root are filled all the same)
  uint64_t launches() const;                                         // append kernels launched so far (tests: a small append is one launch)
  // Past states (DESIGN.md "Past states of the commitment tree"): state m = the tree of the first m leaves, 0 <= m <= size().  Each entry checks its arguments
  // before anything is queued — false: a size above size(), an index not below its size, a null pointer; nothing is written and nothing changes then — and is at
  // most two kernel launches and one download whatever q is.
  bool roots_at(const uint64_t *sizes, size_t q, uint8_t *out /* q x 32 */);                       // one launch; sizes may repeat and come in any order
  // match_out[i] = the lowest a with root(sizes[a]) == RT i, or -1 (DESIGN.md "A block against the resident tree").  rts: q x 32 bytes in blob order, or
  // (hash_order) as the bytes of the common.Hash.  One upload, two launches — roots_at's kernel, then the compare, which reads the roots from device memory — and
  // q x 4 bytes back; q = 0 or m = 0 launches nothing (m = 0: all -1).  false also for m >= 2^31.
  bool match_roots(const uint64_t *sizes, size_t m, const uint8_t *rts, size_t q, bool hash_order, int32_t *match_out);
  // match_roots with a window a record (DESIGN.md "A stretch of the chain"): only anchors a with lo[i] <= a < hi[i] count for record i, and a workgroup loads only
  // the roots its records' windows cover.  The same upload (with lo and hi behind the RTs), launches and download.  false also for lo[i] > hi[i] or hi[i] > m.
  bool match_roots_window(const uint64_t *sizes, size_t m, const uint8_t *rts, size_t q, const uint32_t *lo, const uint32_t *hi, bool hash_order, int32_t *match_out);
  bool paths_at(uint64_t size, const uint64_t *indices, size_t q, uint8_t *siblings /* q x depth x 32 */, uint8_t *root /* 32, or null */);
  bool find_at(uint64_t size, const uint8_t leaf[32], uint64_t &index);                           // the first of the first `size` leaves equal to the blob
  bool snapshot_at(uint64_t size, const uint8_t leaf[32], Snapshot &out);                          // snapshot() of state `size`; false also if the tree is smaller
  bool rewind(uint64_t size);                                        // the tree becomes state `size`: the leaves from `size` on are gone (a reorganisation)
  uint64_t state_launches() const;                                   // kernels launched by the five entries above (tests)
  struct Impl; std::unique_ptr<Impl> impl;
};

// The set of spent serial numbers resident in HBM (gpu_snset.hip; DESIGN.md "Spent serial numbers"): an append-only log of distinct 20-byte keys in insertion order
// and an open-addressing index over it; state m = the first m log entries.  An optional exempt key is never in conflict and never inserted.  One mutex per set (taken
// before the device mutex): spend, query, rewind and read_log are each atomic with respect to the others.  false = a bad argument (a size above size(), a null
// pointer, a log that would reach 2^32 - 2 entries): nothing is written and nothing changes.  There is no host set.
class SpentSet {
 public:
  explicit SpentSet(const uint8_t *exempt /* 20 bytes, or null */, int log2_slots = 0 /* tests: a table of 2^4 slots or more; 0 = 2^10 */, const uint64_t *seed = nullptr /* tests; null = getrandom */);
  ~SpentSet();
  uint64_t size() const;
  bool exempt_key(uint8_t out[20]) const;                                     // false: the set has none (out is left alone)
  // the reference's check-then-insert loop in record order (keys: n x 20 bytes; mask: n bytes or null = all in): conflict[i] = 0 skipped (masked out, exempt) or
  // fresh, 1 the key was in the set before the call, 2 an earlier masked-in record of the call has it.  commit: the fresh keys are appended in record order;
  // otherwise the set is afterwards what it was, bit for bit.  One upload, at most one rebuild, three launches and one download whatever n is.
  bool spend(const uint8_t *keys, const uint8_t *mask, size_t n, bool commit, uint8_t *conflict, uint64_t *size_out /* or null */);
  // The same loop with up to two keys a record (keys: n x 2 x 20 bytes, k1 then k2; nkeys[i] = 0 masked out, 1 or 2; more is a bad argument).  The exempt key applies
  // to k1 only.  conflict[i] = 1 a key of the record was in the set before the call, or k2 is the exempt key; else 2 an earlier ACCEPTED record of the call has one of
  // its keys, or k1 == k2; else 0 accepted: with commit its keys are appended, k1 before k2.  A rejected record inserts nothing.  Decided in parallel rounds (DESIGN.md
  // "Two keys a record"): four launches a round whatever n is, one round without conflicts inside the batch; after the round cap the host decides the live records.
  // With commit, a slot that a rejected record held in the last round is left as a tombstone.  Needs n_old + 2n < 2^32 - 2.
  bool spend_pairs(const uint8_t *keys, const uint8_t *nkeys, size_t n, bool commit, uint8_t *conflict, uint64_t *size_out /* or null */);
  void set_round_cap(uint32_t rounds);                                        // tests: the round cap of this set; 0 = the default
  static void rounds(uint64_t &rounds, uint64_t &host_finishes);              // rounds run and host finishes made by all sets of the process so far (tests)
  bool query(uint64_t size, const uint8_t *keys, size_t q, uint64_t *index, bool current = false);   // index[i] = the key's position in the log if below `size` (current: below size()), else 2^64 - 1
  bool rewind(uint64_t size);                                                 // the set becomes state `size`
  bool read_log(uint64_t first, uint64_t count, uint8_t *out);                // keys first .. first + count - 1 of the log, 20 bytes each
  void table(std::vector<uint32_t> &slots, uint64_t &seed, uint64_t &tombstones);   // tests: the index as it lies in device memory
  static uint64_t launches();                                                 // kernels launched by all sets of the process so far (tests)
  struct Impl; std::unique_ptr<Impl> impl;
};

// spend_pairs after the round cap (capi_zk.cpp: host code, so the sanitizer builds cover it): the sequential loop on what the rounds left.  keys: n x 2 x 20 bytes,
// active: 2n flags.  The keys of the accepted records go into a host set; the live records (status 0) are walked in order and become accepted (1), or rejected (2)
// with code 2 where a key is in that set or k1 == k2.  No live record has a resident key: the first round rejected those.
void snset_pairs_finish_host(const uint8_t *keys, const uint8_t *active, size_t n, uint8_t *status, uint8_t *code);

// The account table resident in HBM (gpu_accounts.hip; DESIGN.md "Account table"): a map from a 20-byte address to a 32-byte value as an append-only log of (address,
// value, prev) entries and the spent set's index over it, a slot holding the address's latest entry; state m = the first m log entries, and the value of an address
// at state m is that of its latest entry below m, or 32 zero bytes.  One mutex per table (taken before the device mutex): every entry is atomic with respect to the
// others.  false = a bad argument (a size above size(), a null pointer with a count, a log that would reach 2^32 - 2 entries): nothing is written and nothing
// changes.  Records are zk_block_record (include/zk_records.h) as bytes, 720 each; a record whose kind is above 3 takes no part.  There is no host table.
class AccountTable {
 public:
  explicit AccountTable(int log2_slots = 0 /* tests: a table of 2^4 slots or more; 0 = 2^10 */, const uint64_t *seed = nullptr /* tests; null = getrandom */);
  ~AccountTable();
  uint64_t size() const;
  // unconditional and in order (addrs: n x 20 bytes, values: n x 32): every record becomes a log entry, a repeated address ends at its last record's value
  bool set(const uint8_t *addrs, const uint8_t *values, size_t n, uint64_t *size_out /* or null */);
  bool get(const uint8_t *addrs, size_t q, int64_t at_size /* -1 = current */, uint8_t *out /* q x 32 */);   // read-only, one launch
  // the OLD slot of every record (and nothing else of it) becomes the sender's value: the table's current one, or — chained — the NEW slot of the closest earlier
  // record of the call with the same sender.  The table is afterwards what it was, index included.
  bool fill(const uint8_t *addrs, uint8_t *recs, size_t n, bool chained, bool tiled = false /* the segment entries: the tiled predecessor search */);
  bool commit_chain(const uint8_t *addrs, const uint8_t *recs, size_t n, uint64_t *size_out /* or null */, bool tiled = false);   // set() with the values read from the records' NEW slots
  // a stretch of the chain: what fill(chained) writes and what commit_chain appends, by the tiled search, whose list walks are bounded by the batch's tiles
  // (ceil(n / 256) nodes), not by a sender's records
  bool fill_segment(const uint8_t *addrs, uint8_t *recs, size_t n) { return fill(addrs, recs, n, true, true); }
  bool commit_segment(const uint8_t *addrs, const uint8_t *recs, size_t n, uint64_t *size_out /* or null */) { return commit_chain(addrs, recs, n, size_out, true); }
  bool rewind(uint64_t size);                                                 // the table becomes state `size`
  bool read_log(uint64_t first, uint64_t count, uint8_t *out);                // entries first .. first + count - 1: 56 bytes each — address 20, value 32, prev as a little-endian word
  void table(std::vector<uint32_t> &slots, uint64_t &seed, uint64_t &tombstones);   // tests: the index as it lies in device memory
  void set_chain_cap(uint32_t cap);                                           // tests: the list walk's cap of this table; 0 = the default
  static void launches(uint64_t &launches, uint64_t &host_finishes);          // kernels launched and predecessor searches finished on the host, by all tables of the process (tests)
  struct Impl; std::unique_ptr<Impl> impl;
};

// The proof cache (gpu_proof_cache.hip; DESIGN.md "Proof cache").  The key of a record is the first 20 bytes of SHA-256(salt[32] || vktag[32] || record[720]).
// record_digests_dev: the keys of n records on the device (k_record_digest).  mid: the SHA-256 states after the block salt || vktag, eight words for each of the kinds
// 0..3; kinds: bit k set = kind k has a key; a record of any other kind gets 20 zero bytes.  The caller holds the device mutex; runs on the main stream and returns
// after it has been synchronised.  One process-wide workspace, kept and grown.
void record_digests_dev(const uint8_t *recs, size_t n, const uint32_t mid[32], uint32_t kinds, uint8_t *out20);
uint64_t record_digest_launches();   // digest kernels launched so far, process-wide (tests: a small call takes the host model)
// The cache itself: two generations of keys, `young` and `old`, each a SpentSet without an exempt key.  One mutex per cache, taken before a set's mutex and the device
// mutex; lookup and insert are one critical section each, and the caller verifies between them without the cache's mutex.  Every entry throws GpuError on failure.
class ProofCache {
 public:
  explicit ProofCache(uint64_t capacity /* entries, 2 or more */, const uint8_t *salt = nullptr /* 32 bytes (tests); null = getrandom */);
  ~ProofCache();
  const uint8_t *salt() const;
  void lookup(const uint8_t *keys, size_t q, uint8_t *hit);   // hit[i] = 1 if key i (q x 20 bytes) is in either generation as it is now; a hit in `old` is not refreshed
  // young.spend(keys, mask, commit) over n x 20 bytes.  Before it: more than capacity / 2 masked-in records are cut to the first capacity / 2 in record order, and
  // if young would then grow past capacity / 2, old is dropped, young becomes old and a fresh set becomes young.  The two never hold more than `capacity` keys.
  void insert(const uint8_t *keys, const uint8_t *mask, size_t n);
  void clear();                                                // both generations empty; the counters go on
  void stats(uint64_t out[4]);                                 // hits, misses, keys stored, entries held now
  struct Impl; std::unique_ptr<Impl> impl;
};

// The roots of many independent commitment lists (gpu_list_roots.hip): list i = leaves[first .. first + count) of one shared array, roots[i] = the root of the tree
// above over that list alone (notes.cpp: merkle_root), in the caller's order.  hash_order: leaves and roots as the bytes of the common.Hash instead of blob order.
// The caller has checked the arguments (depth 1..32, every range inside the array, count <= 2^depth) and holds the device mutex; runs on the main stream and
// returns after it has been synchronised.  One process-wide workspace, kept and grown.
struct LeafRange { uint64_t first, count; };
void list_roots_dev(int depth, const uint8_t *leaves, size_t n_leaves, const LeafRange *lists, size_t n_lists, bool hash_order, uint8_t *roots);
uint64_t list_roots_launches();   // root kernels launched so far, process-wide (tests: the count does not grow with the number of lists)

// Evaluation domain of size m = 2^k or 2^k + 2^r (libfqfft get_evaluation_domain, get_evaluation_domain.tcc:33-52) with
// its twiddle / coset tables resident in HBM.
struct R1csHost;
class Domain {
 public:
  explicit Domain(size_t min_size); explicit Domain(const Domain &peer); ~Domain();   // the copy shares the twiddle / coset tables and owns its scratch space
  size_t m() const; bool is_step() const;
  // in place on `batch` device vectors of m elements each, `stride` elements apart (Montgomery form)
  void fft(Fe32 *data, int batch, size_t stride); void ifft(Fe32 *data, int batch, size_t stride);
  void coset_fft(Fe32 *data, int batch, size_t stride); void icoset_fft(Fe32 *data, int batch, size_t stride);
  // = ifft(); coset_fft(); on a step domain the passes between the two transforms are one kernel
  void ifft_then_coset_fft(Fe32 *data, int batch, size_t stride);
 private: void fft_with_factors(Fe32 *data, int batch, size_t stride, const Fe32 *factors); public:
  // key load: the H query (n_in = m - 1 affine points) re-expressed so that sum_j v_j out_j = sum_i icosetFFT(v)_i h_i: the prover then skips the last
  // transform (ecntt.cuh)
  bool supports_h_lagrange() const; void h_query_to_coset_lagrange(const G1AffineRaw *h, size_t n_in, G1AffineRaw *out /* m points */);
  // key load, radix-2 domains: out (n_vars + 1 points) = the L query extended to all variables minus the C polynomial's share of the H term; the prover then
  // transforms A and B only (ecntt.cuh)
  bool supports_c_fold() const;
  void fold_c_into_l(const G1AffineRaw *h_lagrange /* m */, const R1csHost &cs, const G1AffineRaw *L /* n_vars - n_inputs */, G1AffineRaw *out);
  // a = (a*b - c) / Z on the coset (c may be null: a = a*b / Z); zinv_dev(): 1/Z on the coset, one element or (step domains) a table of m
  const Fe32 *zinv_dev() const; bool zinv_is_table() const;
  void qap_pointwise(Fe32 *a, const Fe32 *b, const Fe32 *c);
  struct Impl; std::unique_ptr<Impl> impl;
};

// R1CS in CSR form resident in HBM (three matrices, coefficient table) — kernel K1
struct R1csHost {                               // as parsed from a key file or emitted by a circuit
  size_t n_inputs = 0, n_vars = 0, n_cons = 0;  // n_vars excludes ONE
  std::vector<uint32_t> rowptr[3], col[3]; std::vector<Fe32> coeff[3];   // coeff canonical (non-Montgomery), col 0 = ONE
};
class R1csDev {
 public:
  explicit R1csDev(const R1csHost &h); explicit R1csDev(const R1csDev &peer); ~R1csDev();   // the copy shares the CSR arrays and owns its failure word
  // z_dev: n_vars+1 Fr (Montgomery, z[0] = 1).  abc: 3 vectors of m (zero padded, aA[n_cons + i] = z_i for i <= n_inputs; r1cs_to_qap.tcc:227-230)
  // tags: one byte per variable (0 / 1 / 2 = other) when the assignment came in compact form; write_c = false: the C vector is not stored (it is folded into
  // the L query)
  void eval(const Fe32 *z_dev, Fe32 *abc, size_t m, const uint8_t *tags_dev = nullptr, bool write_c = true);
  bool satisfied(const Fe32 *abc, size_t m);    // synchronises
  // eval() also tests a*b == c row by row; true if the last eval() found every constraint satisfied (read after the main stream has been synchronised)
  bool check_result() const;
  uint32_t failed_row() const;   // a constraint the last eval() found violated (while check_result() is false)
  struct Impl; std::unique_ptr<Impl> impl;
};

void fr_to_mont_dev(Fe32 *a, size_t n); void fr_from_mont_dev(Fe32 *a, size_t n);
// compact assignment upload (ntt.cuh: k_expand_witness). packed = [ones bitmap | other bitmap | (canon bitmap, canon == 2) | block offsets | values at
// expand_values_offset()]; canon: 0 all values in Montgomery form, 1 all canonical, 2 the third bitmap says which are canonical. tags_out / other_vars_out: see
// WitnessTags
inline size_t expand_values_offset(size_t words, int canon) { return (((canon == 2 ? 28 : 20) * words + 31) / 32) * 32; }
// compact assignment upload (ntt.cuh: k_expand_witness)
void expand_witness_dev(const uint8_t *packed_dev, size_t words, const Fe32 &one_value, int canon, size_t n, Fe32 *out, uint8_t *tags_out = nullptr,
    uint32_t *other_vars_out = nullptr);
// the same tags and list from an assignment that already lies in device memory (ntt.cuh: k_classify_witness); counters = two words, alternating by parity
// a circuit board's hand-over (ntt.cuh: k_expand_board): tag bytes and the candidates' values already on the device -> z, tags, the list of other values
// (vals_by_var: cand_vals is the board's whole wide array — entry = variable number — instead of the gathered list)
void expand_board_dev(const uint8_t *board_tags, size_t n, const uint32_t *cand, const Fe32 *cand_vals, size_t n_cand, Fe32 *z, uint8_t *tags, uint32_t *other_vars,
    uint32_t *counters, int parity, bool vals_by_var = false);
// groups of variables with equal columns folded into one place each (ntt.cuh: k_merge_equal_columns); tags may be null; on the main stream
void merge_equal_columns_dev(Fe32 *z, uint8_t *tags, const uint32_t *grp_ptr, const uint32_t *grp_mem, size_t n_groups);
void classify_witness_dev(const Fe32 *z, size_t n, uint8_t *tags_out, uint32_t *other_vars_out, uint32_t *counters, int parity);

// Key loading: y-coordinates of compressed points (x Montgomery; flags bit0 = parity of canonical y, bit1 = point at infinity). Throws if an x is not on the
// curve.
void decompress_g1(const Fe32 *xs, const uint8_t *flags, size_t n, G1AffineRaw *out);
void decompress_g2(const Fe32 *xs /* 2 per point */, const uint8_t *flags, size_t n, G2AffineRaw *out);
// Key generation: out[i] = scalars[i] * base (scalars canonical), results affine Montgomery
void fixed_base_mul_g1(const host::HG1 &base, const Fe32 *scalars, size_t n, G1AffineRaw *out);
void fixed_base_mul_g2(const host::HG2 &base, const Fe32 *scalars, size_t n, G2AffineRaw *out);
// host memory the device reads in place: pins the pages of [p, p + bytes) and returns the device's address of p, or null if that is not possible (callers then stage);
// gpu_host_unregister(p) undoes it
void *gpu_host_register(void *p, size_t bytes);
void gpu_host_unregister(void *p);
void gpu_sync();            // all streams
void gpu_fork_aux();        // auxiliary streams wait for everything queued on the main stream so far
void gpu_fork_one(int aux); // the same for one auxiliary stream
// the two halves of a fork: record the point on the main stream once, let each auxiliary stream wait for it (from any thread)
void gpu_fork_record();
void gpu_fork_wait(int aux);
void gpu_join_aux();        // the main stream waits for everything queued on the auxiliary streams
bool profiling_enabled();
uint64_t general_path_repeats();   // how often a fast MSM path raised its flag and the MSM was repeated on the general path, process-wide (tests, soak runs)
void note_general_path_repeat();
// per-stage device timing (HIP events on the compute stream); report = JSON object {stage: {ms_total, count}}
void profile_enable(bool on); std::string profile_report();
// host work beside the device stages of the same report (wall-clock ms under `name`); a no-op while profiling is off
void profile_add_host(const char *name, double ms);
struct HostSpan { const char *name; bool on; double t0; explicit HostSpan(const char *n); ~HostSpan(); HostSpan(const HostSpan &) = delete; };

}  // namespace zk
