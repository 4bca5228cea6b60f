// The proof cache (DESIGN.md "Proof cache"; include/zk_proof_cache.h): the reference node verifies every zk transaction when it enters the pool
// (core/tx_pool.go:612-645) and again when its block is applied (core/state_processor.go:106-163).  A record whose proof this process has accepted before is known
// by a keyed digest, the first 20 bytes of SHA-256(salt[32] || vktag[32] || record[720]), and skips the pairing work the second time.
//   k_record_digest: the digests of a block's records, one lane per record.
//   ProofCache:      two generations of keys, each a SpentSet (gpu_snset.hip) with no exempt key.
// The digest kernel runs on the library's main stream (lane 0) under the device mutex, which the caller holds.  The cache has a mutex of its own, taken before a set's
// mutex and the device mutex.
#include <sys/random.h>
#include <atomic>
#include <cstring>
#include <mutex>
#include "gpu_internal.hpp"
#include "tree_sha256.cuh"

namespace zk {

// ---- k_record_digest -------------------------------------------------------------------------------------------------------------------------------------------
// The message is 784 bytes: thirteen blocks and the padding fits the last one.  Block 0, salt || vktag, is the same for every record of a kind: the host compresses
// it once (mid: four states of eight words, by kind) and a lane continues from there over blocks 1..11 = record bytes 0..703 and block 12 = bytes 704..719, 0x80,
// zeros and the bit length 6,272.
// A workgroup is one wave and takes 64 records.  They arrive as 45 coalesced 16-byte loads a record and are laid into LDS 181 words apart: with an odd stride the
// lanes that read word k of their own records all hit different banks (at 180 words, a multiple of four, it would be a 4-way conflict).  724 is no multiple of 16, so
// the staging stores are single words.
constexpr uint32_t DIG_THREADS = 64, DIG_VEC = 45 /* 16-byte pieces of a record */, DIG_STRIDE = 181 /* words between two records in LDS */, DIG_BITS = 8 * (64 + 720);
static_assert(DIG_VEC * 16 == 720 && (DIG_STRIDE & 1) == 1 && DIG_STRIDE * 4 >= 720, "record layout");

static __global__ void __launch_bounds__(DIG_THREADS) k_record_digest(const uint4 *__restrict__ recs, const uint32_t *__restrict__ mid /* 4 x 8 words */, uint32_t kinds /* bit k: kind k has a key */,
    uint32_t n, uint32_t *__restrict__ out /* n x 5 words */) {
  __shared__ uint32_t sh[DIG_THREADS * DIG_STRIDE]; __shared__ uint32_t sm[32];
  const uint32_t tid = threadIdx.x, r0 = blockIdx.x * DIG_THREADS, cnt = n - r0 < DIG_THREADS ? n - r0 : DIG_THREADS;
  for (uint32_t k = tid; k < cnt * DIG_VEC; k += DIG_THREADS) {
    const uint4 v = recs[(size_t)r0 * DIG_VEC + k]; const uint32_t r = k / DIG_VEC, c = k - r * DIG_VEC; uint32_t *d = sh + r * DIG_STRIDE + 4 * c;
    d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
  }
  if (tid < 32) sm[tid] = mid[tid];
  __syncthreads();
  if (tid >= cnt) return;
  const uint32_t *rw = sh + tid * DIG_STRIDE; const uint32_t kind = rw[0] & 0xffu; uint32_t *o = out + 5 * (size_t)(r0 + tid);
  if (kind > 3 || !((kinds >> kind) & 1u)) {                                                       // no key for this record: 20 zero bytes
#pragma unroll
    for (int j = 0; j < 5; j++) o[j] = 0;
    return;
  }
  uint32_t s[8], w[16];
#pragma unroll
  for (int j = 0; j < 8; j++) s[j] = sm[8 * kind + j];
#pragma unroll 1
  for (uint32_t b = 0; b < 11; b++) {
#pragma unroll
    for (int j = 0; j < 16; j++) w[j] = __builtin_bswap32(rw[16 * b + j]);
    tree_compress_chain(s, w);
  }
#pragma unroll
  for (int j = 0; j < 4; j++) w[j] = __builtin_bswap32(rw[176 + j]);
  w[4] = 0x80000000u;
#pragma unroll
  for (int j = 5; j < 15; j++) w[j] = 0;
  w[15] = DIG_BITS;
  tree_compress_chain(s, w);
#pragma unroll
  for (int j = 0; j < 5; j++) o[j] = __builtin_bswap32(s[j]);                                       // digest order: five big-endian words
}

static std::atomic<uint64_t> g_digest_launches{0};
uint64_t record_digest_launches() { return g_digest_launches.load(); }

namespace {
struct DigestWorkspace { DevBuf<uint8_t> in /* the four states, then the records */, out; size_t cap = 0; };
DigestWorkspace &digest_workspace() { static DigestWorkspace *w = new DigestWorkspace(); return *w; }
}  // namespace

void record_digests_dev(const uint8_t *recs, size_t n, const uint32_t mid[32], uint32_t kinds, uint8_t *out20) {
  if (!n) return;
  if (!recs || !out20 || n > (1u << 26)) throw GpuError("record digests: record count or a null pointer");
  LaneScope lane(0); DigestWorkspace &W = digest_workspace(); hipStream_t s = gpu().stream;
  if (n > W.cap) { const size_t cap = n + n / 4 + 64; W.in = DevBuf<uint8_t>(128 + cap * 720); W.out = DevBuf<uint8_t>(cap * 20); W.cap = cap; }
  SyncAtExit sync;
  HIP_CHECK(hipMemcpyAsync(W.in.get(), mid, 128, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(W.in.get() + 128, recs, n * 720, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_record_digest, dim3(cdiv(n, DIG_THREADS)), dim3(DIG_THREADS), 0, s, (const uint4 *)(W.in.get() + 128), (const uint32_t *)W.in.get(), kinds, (uint32_t)n, (uint32_t *)W.out.get());
  g_digest_launches.fetch_add(1); HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpyAsync(out20, W.out.get(), n * 20, hipMemcpyDeviceToHost, s)); HIP_CHECK(hipStreamSynchronize(s));
}

// ---- ProofCache ------------------------------------------------------------------------------------------------------------------------------------------------
// Two generations.  `young` takes every insert; when it would grow past capacity / 2 the old generation is dropped, young becomes old and a fresh set becomes young,
// so the two together never hold more than `capacity` keys and a key lives for at least capacity / 2 inserts after its own.  A hit in `old` is not refreshed.
struct ProofCache::Impl {
  std::mutex mu; uint64_t capacity = 0, half = 0, hits = 0, misses = 0, inserted = 0; uint8_t salt[32]; std::unique_ptr<SpentSet> young, old;
};
ProofCache::ProofCache(uint64_t capacity, const uint8_t *salt) : impl(new Impl) {
  Impl &d = *impl; if (capacity < 2 || capacity / 2 >= 0x7fffffffull) throw GpuError("proof cache: the capacity must lie between 2 and 2^32 - 2 entries");
  d.capacity = capacity; d.half = capacity / 2;
  if (salt) memcpy(d.salt, salt, 32); else if (getrandom(d.salt, 32, 0) != 32) throw GpuError("proof cache: getrandom gave no salt");
  d.young.reset(new SpentSet(nullptr)); d.old.reset(new SpentSet(nullptr));
}
ProofCache::~ProofCache() = default;
const uint8_t *ProofCache::salt() const { return impl->salt; }
void ProofCache::lookup(const uint8_t *keys, size_t q, uint8_t *hit) {
  Impl &d = *impl; std::lock_guard<std::mutex> lk(d.mu); if (!q) return;
  std::vector<uint64_t> at(q); memset(hit, 0, q);
  for (SpentSet *s : {d.young.get(), d.old.get()}) {
    if (!s->size()) continue;
    if (!s->query(0, keys, q, at.data(), true)) throw GpuError("proof cache: lookup");
    for (size_t i = 0; i < q; i++) hit[i] |= at[i] != UINT64_MAX;
  }
  uint64_t h = 0; for (size_t i = 0; i < q; i++) h += hit[i];
  d.hits += h; d.misses += q - h;
}
void ProofCache::insert(const uint8_t *keys, const uint8_t *mask, size_t n) {
  Impl &d = *impl; std::lock_guard<std::mutex> lk(d.mu);
  uint64_t cand = 0; for (size_t i = 0; i < n; i++) cand += mask[i] != 0;
  if (!cand) return;
  std::vector<uint8_t> cut, conflict(n);
  if (cand > d.half) {                                                                             // more than a generation holds: the first capacity / 2 in record order
    cut.assign(n, 0); uint64_t taken = 0;
    for (size_t i = 0; i < n && taken < d.half; i++) if (mask[i]) { cut[i] = 1; taken++; }
    mask = cut.data(); cand = d.half;
  }
  if (d.young->size() + cand > d.half) { std::unique_ptr<SpentSet> fresh(new SpentSet(nullptr)); d.old = std::move(d.young); d.young = std::move(fresh); }
  const uint64_t before = d.young->size(); uint64_t after = before;
  if (!d.young->spend(keys, mask, n, true, conflict.data(), &after)) throw GpuError("proof cache: insert");
  d.inserted += after - before;
}
void ProofCache::clear() {
  Impl &d = *impl; std::lock_guard<std::mutex> lk(d.mu);
  if (!d.young->rewind(0) || !d.old->rewind(0)) throw GpuError("proof cache: clear");
}
void ProofCache::stats(uint64_t out[4]) {
  Impl &d = *impl; std::lock_guard<std::mutex> lk(d.mu);
  out[0] = d.hits; out[1] = d.misses; out[2] = d.inserted; out[3] = d.young->size() + d.old->size();
}

}  // namespace zk
